"""Per-site convergence diagnostics, the parts that need no device: the state names in header and binding, ``SiteDiagnostics``
on sums built by a numpy restatement of the device's update rule against the direct batch-means computation on the draws
themselves (synthetic AR(1) series), R-hat on chains that do and do not share a law, the edge cases, ``diagnostics_batch``,
the refusals of the probit sampler and of a sampler with a Python ``step``, ``post.site_diagnostics`` from a stand-in engine
with its call order written out, and the silence of the default."""
import os
import re

import numpy as np
import pytest

from ._launch_text import assert_launched_only_while_on, unit_text
from .conftest import ROOT, load_golden
from .test_api_cpu import _inputs
from .test_cpu_abi import cpu_abi  # noqa: F401  (the oracle's build of the C ABI, which does not know the conv_* names)

CONV_NAMES = ('conv_stats', 'conv_count', 'conv_sums')
MESSAGE = r'site_diagnostics must be True, False or a batch length from 1 to 2\^30'


@pytest.fixture(scope='module')
def small():
    return _inputs(load_golden('ref_queen150_ragged'))[:4]   # 150 sites, 100 surveyed, p = 3, q = 2


def sums_of(draws, L):
    """The eleven slots (11, n) after the update rule of DESIGN 21 ran over draws (N, n) of psi AND of eta (the same series
    for both quantities, the second shifted by 2 and scaled by 3), iteration by iteration."""
    N, n = draws.shape
    out = np.zeros((11, n))
    for first, v in ((1, draws), (6, 2.0 + 3.0 * draws)):
        ref, s1, s2, run, bsq = (out[first + k] for k in range(5))
        for m in range(N):
            if m == 0:
                ref[:] = v[0]
            d = v[m] - ref
            s1 += d
            s2 += d * d
            run += d
            if (m + 1) % L == 0:
                bsq += run * run
                run[:] = 0.0
    out[0] = N
    return out


def ar1(rng, N, n, rho, mean=0.0, sd=1.0):
    """n independent stationary AR(1) series of length N, marginal N(mean, sd^2)."""
    x = np.empty((N, n))
    x[0] = rng.standard_normal(n)
    eps = rng.standard_normal((N, n)) * np.sqrt(1.0 - rho * rho)
    for t in range(1, N):
        x[t] = rho * x[t - 1] + eps[t]
    return mean + sd * x


def direct(draws, L):
    """ESS, MCSE, R-hat, mean and W of draws (chains, N, sites) by their textbook formulas."""
    C, N, n = draws.shape
    a = N // L
    means = draws.mean(axis=1)
    W = draws.var(axis=1, ddof=1).mean(axis=0)
    bm = draws[:, :a * L].reshape(C, a, L, n).mean(axis=2)
    sigma2 = (L * bm.var(axis=1, ddof=1)).mean(axis=0)
    rhat = np.sqrt(((N - 1) / N * W + means.var(axis=0, ddof=1)) / W) if C > 1 else np.full(n, np.nan)
    return {'mean': means.mean(axis=0), 'var': W, 'ess': C * N * W / sigma2, 'mcse': np.sqrt(sigma2 / (C * N)), 'rhat': rhat}


# ---- names ---------------------------------------------------------------------------------------------------------
def test_every_conv_state_name_is_in_header_and_binding():
    from occuspytial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    comments = ' '.join(re.findall(r'/\*.*?\*/', header, flags=re.S))
    documented = set(re.findall(r'\b(conv_[a-z0-9]+)\b', comments))
    assert set(CONV_NAMES) == documented, set(CONV_NAMES) ^ documented
    assert tuple(_lib.CONV_FIELDS) == CONV_NAMES
    assert re.search(r'#define OCC_ABI_VERSION 7\b', header) and _lib.ABI_VERSION == 7   # no new function, no layout change
    assert not [name for name, _, _ in _lib.SYMBOLS if 'conv' in name]
    # the switch is a word of the handle and the kernel is launched behind the z update: the planner does not know of it
    assert 'conv_' not in open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'occ_plan.hpp')).read()
    makefile = open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'Makefile')).read()
    # (the translation units are named once, in UNITS: the library and the stamps build compile them, SRC makes both depend on them)
    units = re.search(r'^UNITS := (.*)$', makefile, flags=re.M).group(1).split()
    assert units[:4] == ['occ_gibbs.hip', 'occ_spatial.hip', 'occ_hist.hip', 'occ_conv.hip']
    assert len(re.findall(r'-shared -o \$@ \$\(UNITS\)$', makefile, flags=re.M)) == 2
    assert re.search(r'^SRC := \$\(UNITS\) .*\bocc_conv\.hpp\b', makefile, flags=re.M)


def test_the_kernel_is_launched_only_while_a_switch_is_on():
    """Read off launch_kind: the one call of conv_launch stands behind `if (s->conv.any)`, next to hist_launch in the branch of
    the z update; the word starts at 0, only switch_set raises it -- the one place that does, for every feature behind the z
    update -- and occ_profile clears it for its scope.  A run with the switch never touched enqueues what it enqueued before.
    The unit has one kernel, no atomics and no LDS."""
    assert_launched_only_while_on('conv')
    unit = unit_text('occ_conv.hip')
    assert 'atomic' not in unit.lower() and '__shared__' not in unit and len(re.findall(r'__global__', unit)) == 1
    assert re.search(r'return a\.on\[chain\] != 0u && a\.sums != nullptr && after == t \+ 1u && sc\.err == 0 && rel >= sc\.burnin;', unit)
    hist = unit_text('occ_hist.hip')
    assert re.search(r'return a\.on\[chain\] != 0u && a\.cnt != nullptr && after == t \+ 1u && sc\.err == 0 && rel >= sc\.burnin;', hist)


# ---- 1: synthetic AR(1) series ----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def series():
    """400 independent AR(1) series, rho = 0.5, N = 10 000, mean 0.3, seed 7; their sums at L = 100."""
    draws = ar1(np.random.default_rng(7), 10_000, 400, 0.5, mean=0.3, sd=0.1)
    return draws, sums_of(draws, 100)


def test_ess_and_mcse_equal_the_direct_batch_means_computation(series):
    from occuspytial_amd.convergence import SiteDiagnostics
    draws, sums = series
    sd = SiteDiagnostics(sums[None], 100)
    assert sd.n_draws.tolist() == [10_000] and sd.batch == 100 and sd.n_batches.tolist() == [100] and sd.n_sites == 400
    for q, held in (('psi', draws), ('eta', 2.0 + 3.0 * draws)):
        want = direct(held[None], 100)
        for what in ('mean', 'var', 'ess', 'mcse'):
            rel = np.abs(getattr(sd, what)(q) - want[what]) / np.abs(want[what])
            assert rel.max() <= 1e-9, (q, what, float(rel.max()))
        assert np.all(np.isnan(sd.rhat(q)))                                     # one chain
    assert np.allclose(sd.ess('psi'), sd.ess('eta'), rtol=1e-9)                 # (ESS does not see a shift or a scale)


def test_the_median_ess_is_that_of_the_ar1_law(series):
    """ESS of an AR(1) series is N (1 - rho) / (1 + rho) = 3 333; the batch-means estimate at 100 batches has a spread of its own
    (with this seed: median 3 411, 5th and 95th percentile over the series 2 752 and 4 246); its median is within 10 %."""
    from occuspytial_amd.convergence import SiteDiagnostics
    ess = SiteDiagnostics(series[1][None], 100).ess('psi')
    med, lo, hi = np.median(ess), np.percentile(ess, 5), np.percentile(ess, 95)
    print('median ESS %.0f, 5th and 95th percentile %.0f, %.0f' % (med, lo, hi))
    assert abs(med - 10_000 / 3) <= 0.1 * 10_000 / 3


def test_an_unfinished_batch_is_left_out_of_sigma2():
    """N = 1 037 with L = 100: ten batches, 37 values in `run`; T = s1 - run is the sum over the finished batches."""
    from occuspytial_amd.convergence import SiteDiagnostics
    draws = ar1(np.random.default_rng(11), 1037, 30, 0.3, mean=0.5, sd=0.05)
    sums = sums_of(draws, 100)
    assert sums[4].all()                                                        # (psi's run)
    sd = SiteDiagnostics(sums[None], 100)
    want = direct(draws[None], 100)
    assert sd.n_batches.tolist() == [10]
    for what in ('ess', 'mcse', 'var', 'mean'):
        assert (np.abs(getattr(sd, what)('psi') - want[what]) / np.abs(want[what])).max() <= 1e-9


# ---- 2: R-hat --------------------------------------------------------------------------------------------------------
def test_rhat_tells_a_shifted_chain_from_chains_of_one_law():
    from occuspytial_amd.convergence import SiteDiagnostics
    rng = np.random.default_rng(5)
    chains = np.stack([ar1(rng, 2000, 50, 0.5, mean=0.4, sd=0.05) for _ in range(4)])
    same = SiteDiagnostics(np.stack([sums_of(c, 40) for c in chains]), 40)
    shifted = chains.copy()
    shifted[3] += 3 * 0.05                                                      # one chain 3 sd away
    apart = SiteDiagnostics(np.stack([sums_of(c, 40) for c in shifted]), 40)
    for q in ('psi', 'eta'):
        assert np.all(same.rhat(q) < 1.05) and np.all(apart.rhat(q) > 1.2)
    held = direct(shifted, 40)
    assert (np.abs(apart.rhat('psi') - held['rhat']) / held['rhat']).max() <= 1e-9
    assert (np.abs(apart.ess('psi') - held['ess']) / held['ess']).max() <= 1e-9
    assert (np.abs(apart.mean('psi') - held['mean']) / held['mean']).max() <= 1e-9
    assert apart.worst('psi', 3).tolist() == np.argsort(-held['rhat'], kind='stable')[:3].tolist()


# ---- 3: edge cases ---------------------------------------------------------------------------------------------------
def test_edge_cases():
    from occuspytial_amd.convergence import SiteDiagnostics
    rng = np.random.default_rng(2)
    draws = ar1(rng, 30, 6, 0.2, mean=0.5, sd=0.1)
    other = ar1(rng, 30, 6, 0.2, mean=0.5, sd=0.1)
    # fewer than two batches: ESS and MCSE are NaN, the mean, the variance and R-hat are not
    for L, a in ((30, 1), (16, 1), (31, 0)):
        sd = SiteDiagnostics(np.stack([sums_of(draws, L), sums_of(other, L)]), L)
        assert sd.n_batches.tolist() == [a, a]
        assert np.all(np.isnan(sd.ess('psi'))) and np.all(np.isnan(sd.mcse('eta')))
        assert np.all(np.isfinite(sd.rhat('psi'))) and np.allclose(sd.mean('psi'), (draws.mean(axis=0) + other.mean(axis=0)) / 2, rtol=1e-12)
    # one chain: R-hat is NaN and the worst sites are those of smallest ESS
    one = SiteDiagnostics(sums_of(draws, 5)[None], 5)
    assert np.all(np.isnan(one.rhat('eta'))) and np.all(np.isfinite(one.ess('eta')))
    assert one.worst('eta', 2).tolist() == np.argsort(one.ess('eta'), kind='stable')[:2].tolist()
    assert one.worst('eta', 100).shape == (6,) and one.worst('eta', 0).shape == (0,)
    # chains of unequal length: R-hat raises, the pooled figures weigh by N
    two = SiteDiagnostics(np.stack([sums_of(draws, 5), sums_of(draws[:20], 5)]), 5)
    assert two.n_draws.tolist() == [30, 20] and two.n_batches.tolist() == [6, 4]
    with pytest.raises(ValueError, match='chains of one length'):
        two.rhat('psi')
    assert np.allclose(two.mean('psi'), np.concatenate([draws, draws[:20]]).mean(axis=0), rtol=1e-12)
    assert np.all(np.isfinite(two.ess('psi')))
    # a site that never moved: W = 0 gives R-hat 1 and ESS NaN; the others are untouched
    still = draws.copy()
    still[:, 2] = other[:, 2] = 0.25
    sd = SiteDiagnostics(np.stack([sums_of(still, 5), sums_of(other, 5)]), 5)
    assert sd.var('psi')[2] == 0.0 and sd.rhat('psi')[2] == 1.0 and np.isnan(sd.ess('psi')[2]) and sd.mcse('psi')[2] == 0.0
    assert np.all(np.isfinite(np.delete(sd.ess('psi'), 2))) and np.all(np.delete(sd.rhat('psi'), 2) > 0)
    order = sd.worst('psi', 6)
    assert sorted(order.tolist()) == list(range(6)) and np.all(np.diff(sd.rhat('psi')[order]) <= 0)   # (worst first)
    # no draw at all
    none = SiteDiagnostics(np.zeros((2, 11, 4)), 5)
    assert none.n_draws.tolist() == [0, 0] and np.all(np.isnan(none.ess('psi'))) and np.all(np.isnan(none.mean('eta')))
    # refused inputs
    good = sums_of(draws, 5)
    for bad in (good, np.zeros((0, 11, 6)), np.zeros((1, 10, 6)), good[None][..., None]):
        with pytest.raises(ValueError, match='shape'):
            SiteDiagnostics(bad, 5)
    for L in (0, -1, 2 ** 30 + 1, 2.5, True, None):
        with pytest.raises(ValueError, match='batch length'):
            SiteDiagnostics(good[None], L)
    for cnt in (-1.0, 0.5):
        w = good[None].copy()
        w[0, 0] = cnt
        with pytest.raises(ValueError, match='one whole number'):
            SiteDiagnostics(w, 5)
    w = good[None].copy()
    w[0, 0, 1] += 1
    with pytest.raises(ValueError, match='one whole number'):
        SiteDiagnostics(w, 5)
    with pytest.raises(ValueError, match="'psi' or 'eta'"):
        one.ess('z')


# ---- 4: keyword handling ---------------------------------------------------------------------------------------------
def test_diagnostics_batch():
    from occuspytial_amd.convergence import diagnostics_batch
    assert diagnostics_batch(False) == 0 and diagnostics_batch(np.bool_(False), 100) == 0
    assert diagnostics_batch(True, 40) == 6 and diagnostics_batch(np.bool_(True), 10_000) == 100
    assert diagnostics_batch(True, 1) == 1 and diagnostics_batch(True, 0) == 1 and diagnostics_batch(True, 3) == 1
    assert diagnostics_batch(True, 99) == 9 and diagnostics_batch(True, 100) == 10
    assert diagnostics_batch(1, 40) == 1 and diagnostics_batch(np.int64(15), 40) == 15 and diagnostics_batch(2 ** 30) == 2 ** 30
    for bad in (None, 0, -1, 2 ** 30 + 1, 'yes', 15.0, 2.5, [True]):
        with pytest.raises(ValueError, match=MESSAGE):
            diagnostics_batch(bad, 40)


def test_site_diagnostics_argument_is_validated_and_refused_before_an_engine_exists(small, monkeypatch):
    from occuspytial_amd import LogitICARGibbs, LogitRSRGibbs, ProbitRSRGibbs, _engine
    from occuspytial_amd.gibbs.base import GibbsBase

    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(_engine.Engine, '__init__', no_engine)
    for sampler in (LogitICARGibbs(*small, random_state=1), LogitRSRGibbs(*small, random_state=1, q=10),
                    ProbitRSRGibbs(*small, random_state=1, q=10)):
        for value in (None, 0, -3, 2 ** 30 + 1, 'yes', 64.0, 2.5, [True], np.ones(3, dtype=bool)):
            with pytest.raises(ValueError, match=MESSAGE):
                sampler.sample(5, chains=1, progressbar=False, site_diagnostics=value)
            with pytest.raises(ValueError, match=MESSAGE):
                sampler.resume({'n_chains': 1}, 5, progressbar=False, site_diagnostics=value)
    probit = ProbitRSRGibbs(*small, random_state=1, q=10)
    for value in (True, 16):
        with pytest.raises(NotImplementedError, match='site diagnostics are not available for the probit model'):
            probit.sample(5, chains=1, progressbar=False, site_diagnostics=value)
        with pytest.raises(NotImplementedError, match='site diagnostics are not available for the probit model'):
            probit.resume({'n_chains': 1}, 5, progressbar=False, site_diagnostics=value)

    class PyStep(GibbsBase):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._configure(a[0], None)

        def step(self):
            raise AssertionError('step was called')

    with pytest.raises(NotImplementedError, match='Python'):
        PyStep(*small, random_state=1).sample(5, site_diagnostics=True)
    with pytest.raises(ValueError, match=MESSAGE):                                        # (the argument is looked at first)
        PyStep(*small, random_state=1).sample(5, site_diagnostics=None)


class StandIn:
    """An object with the Engine interface whose sums are its own: while the switch is on, every iteration past a ``run``'s
    burn-in draws a value per chain and site, as the device does; switching on zeroes.  ``log`` keeps the calls in order,
    ``held`` the draws that were counted."""

    def __init__(self, prob, n_chains, seed=5):
        self.prob, self.n_chains = prob, n_chains
        self.rng = np.random.default_rng(seed)
        self._sums_on = {}
        self._conv_batch = 0
        self.log, self.held = [], [[] for _ in range(n_chains)]

    def set_keys(self, keys):
        pass

    def set_start(self, chain, alpha, beta, tau, eta):
        pass

    def set(self, name, value, chain=0):
        pass

    def get(self, name, chain=0):
        p = self.prob
        sizes = dict(alpha=p.q, beta=p.p, eta=p.n, z=p.n, omega_b=p.n, omega_a=p.R, theta=10)
        if name == 'tau':
            return 1.0
        if name == 'exists':
            return np.ones(p.S)
        return np.ones(sizes[name])

    def conv_stats(self, batch):
        self.log.append(('on', int(batch)) if batch else 'off')
        if batch:
            self.held = [[] for _ in range(self.n_chains)]
            self.L = int(batch)
        self._conv_batch = int(batch)

    def conv_sums(self, chain=0):
        return {'batch': self.L, 'count': len(self.held[chain]), 'sums': sums_of(np.stack(self.held[chain]), self.L)}

    def run(self, n_iter, burnin=0):
        keep, C, p = n_iter - burnin, self.n_chains, self.prob
        self.log.append(('run', n_iter, burnin, self._conv_batch))
        for c in range(C):
            for _ in range(keep if self._conv_batch else 0):
                self.held[c].append(self.rng.uniform(size=p.n) ** (1 + c))
        return np.zeros((C, keep, p.q)), np.zeros((C, keep, p.p)), np.ones((C, keep))


@pytest.mark.parametrize('progressbar', [False, True])
@pytest.mark.parametrize('asked, L', [(True, 6), (5, 5)])
def test_post_site_diagnostics_from_a_stand_in_engine(small, progressbar, asked, L):
    """60 iterations, 20 of them burn-in, 3 chains: True is L = floor(sqrt(40)) = 6.  With the progress bar the call runs in
    chunks of 16: one whole chunk of burn-in with the switch off, the switch on before the chunk that straddles the boundary,
    and the engine's own window rule (counted past the chunk's burn-in) does the rest."""
    from occuspytial_amd import LogitICARGibbs
    from occuspytial_amd.convergence import SiteDiagnostics
    s = LogitICARGibbs(*small, random_state=3)
    prob = s._problem
    fake = StandIn(prob, 3)
    s.__dict__['_get_engine'] = lambda keys: fake
    out = s.sample(60, burnin=20, chains=3, progressbar=progressbar, site_diagnostics=asked)
    if progressbar:
        assert fake.log == ['off', ('run', 16, 15, 0), ('on', L), ('run', 16, 4, L), ('run', 16, 0, L), ('run', 12, 0, L)]
    else:
        assert fake.log == ['off', ('on', L), ('run', 60, 20, L)]
    sd = out.site_diagnostics
    assert isinstance(sd, SiteDiagnostics) and sd.batch == L and sd.n_sites == prob.n and sd.n_draws.tolist() == [40, 40, 40]
    want = direct(np.stack([np.stack(h) for h in fake.held]), L)
    for what in ('mean', 'var', 'ess', 'mcse', 'rhat'):
        assert (np.abs(getattr(sd, what)('psi') - want[what]) / np.abs(want[what])).max() <= 1e-9, what
    # post.summary and the chains are what they are without the keyword
    assert sorted(out.data) == ['alpha', 'beta', 'tau'] and sorted(s.chain._names) == ['alpha', 'beta', 'tau']
    fake0 = StandIn(prob, 2)
    s.__dict__['_get_engine'] = lambda keys: fake0
    plain = s.sample(10, burnin=2, chains=2, progressbar=False)
    assert plain.site_diagnostics is None and fake0.log == [('run', 10, 2, 0)]
    fake0._conv_batch = 6                                                       # (a reused engine that an earlier call left on)
    s.sample(10, burnin=2, chains=2, progressbar=False)
    assert fake0.log[1:] == ['off', ('run', 10, 2, 0)]


def test_posterior_parameter_has_the_attribute():
    from occuspytial_amd.posterior import PosteriorParameter
    assert PosteriorParameter.site_diagnostics is None


def test_engine_binding_names():
    from occuspytial_amd._engine import Engine, EngineGroup
    for cls in (Engine, EngineGroup):
        assert callable(cls.conv_stats) and callable(cls.conv_sums)


def test_a_library_without_the_feature_is_refused_and_the_default_asks_nothing(cpu_abi, small, monkeypatch):  # noqa: F811
    """Every occ_get_state / occ_set_state call goes through a recording wrapper: with the default none names conv_*."""
    from occuspytial_amd import LogitICARGibbs
    asked = []

    def recording(fn):
        def call(handle, chain, name, *rest):
            asked.append(name.decode())
            return fn(handle, chain, name, *rest)
        return call
    monkeypatch.setattr(cpu_abi, 'occ_get_state', recording(cpu_abi.occ_get_state))
    monkeypatch.setattr(cpu_abi, 'occ_set_state', recording(cpu_abi.occ_set_state))
    s = LogitICARGibbs(*small, random_state=3)
    out = s.sample(5, chains=1, progressbar=False)
    assert out.site_diagnostics is None and out['alpha'].shape[:2] == (1, 5)
    ckpt = s.checkpoint()
    assert not [key for key in ckpt if key.startswith('conv_')]
    s.resume(ckpt, 3, progressbar=False)
    assert asked and not [name for name in asked if name.startswith('conv_')]      # (the wrapper saw the other calls)
    with pytest.raises(ValueError, match=r'has no site diagnostics .*rebuild it'):
        LogitICARGibbs(*small, random_state=3).sample(5, chains=1, progressbar=False, site_diagnostics=True)
    assert [name for name in asked if name.startswith('conv_')] == ['conv_stats']
    with pytest.raises(ValueError, match=r'has no site diagnostics .*rebuild it'):
        s.resume(ckpt, 3, progressbar=False, site_diagnostics=16)
