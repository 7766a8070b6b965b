"""Per-site intervals, the parts that need no device: the state names in header and binding, ``interval_bins``,
``SiteIntervals`` against plain numpy on the draws themselves (brackets, interpolated quantiles, exceedance, the merge of
chains of unequal length, the edge cases), the validation of ``site_intervals=``, the refusals of the probit sampler and of a
sampler with a Python ``step``, ``post.site_intervals`` from a stand-in engine with its call order written out, and the
silence of the default."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from ._launch_text import assert_launched_only_while_on, unit_text
from .conftest import ROOT, load_golden
from .test_api_cpu import _inputs
from .test_cpu_abi import cpu_abi  # noqa: F401  (the oracle's build of the C ABI, which does not know the hist_* names)

HIST_NAMES = ('hist_stats', 'hist_count', 'hist_counts')
MESSAGE = 'site_intervals must be True, False or a number of bins from 4 to 1024'


@pytest.fixture(scope='module')
def small():
    return _inputs(load_golden('ref_queen150_ragged'))[:4]   # 150 sites, 100 surveyed, p = 3, q = 2


def test_every_hist_state_name_is_in_header_and_binding():
    from occuspytial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    comments = ' '.join(re.findall(r'/\*.*?\*/', header, flags=re.S))
    documented = set(re.findall(r'\b(hist_[a-z0-9]+)\b', comments))
    assert set(HIST_NAMES) == documented, set(HIST_NAMES) ^ documented
    assert tuple(_lib.HIST_FIELDS) == HIST_NAMES
    assert re.search(r'#define OCC_ABI_VERSION 7\b', header) and _lib.ABI_VERSION == 7   # no new function, no layout change
    assert not [name for name, _, _ in _lib.SYMBOLS if 'hist' in name]
    # the switch is a word of the handle and the kernel is launched behind the z update: the planner does not know of it
    assert 'hist' not in open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'occ_plan.hpp')).read()
    makefile = open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'Makefile')).read()
    # (the translation units are named once, in UNITS: the library and the stamps build compile them, SRC makes both depend on them)
    units = re.search(r'^UNITS := (.*)$', makefile, flags=re.M).group(1).split()
    assert units[:3] == ['occ_gibbs.hip', 'occ_spatial.hip', 'occ_hist.hip']
    assert len(re.findall(r'-shared -o \$@ \$\(UNITS\)$', makefile, flags=re.M)) == 2
    assert re.search(r'^SRC := \$\(UNITS\) .*\bocc_hist\.hpp\b', makefile, flags=re.M)


def test_the_kernel_is_launched_only_while_a_switch_is_on():
    """occ_get_stats counts no launches per kernel, so this is read off launch_kind: the one call of hist_launch stands behind
    `if (s->hist.any)`, next to sp_launch in the branch of the z update; the word starts at 0, only switch_set raises it -- the
    one place that does, for every feature behind the z update -- and occ_profile clears it for its scope.  A run with the
    switch never touched enqueues what it enqueued before."""
    assert_launched_only_while_on('hist')
    unit = unit_text('occ_hist.hip')
    assert 'atomic' not in unit.lower() and '__shared__' not in unit and len(re.findall(r'__global__', unit)) == 1


def test_interval_bins():
    from occuspytial_amd.intervals import interval_bins
    assert interval_bins(False) == 0 and interval_bins(True) == 64 and interval_bins(np.bool_(True)) == 64
    assert interval_bins(np.bool_(False)) == 0
    for b in (4, 5, 64, 1024, np.int64(128), np.int32(4)):
        assert interval_bins(b) == int(b) and type(interval_bins(b)) is int
    for bad in (None, 0, 1, 3, 1025, -64, 64.0, 2.5, '64', [64], np.ones(3, dtype=bool), np.float64(64)):
        with pytest.raises(ValueError, match=MESSAGE):
            interval_bins(bad)


# ---- SiteIntervals against numpy on the draws ----------------------------------------------------------------------
N_SITES, LENGTHS = 37, (41, 7, 112)


def _draws(seed=11):
    """Random psi for 37 sites x 3 chains of unequal length; every site has a centre and a spread of its own."""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-3.0, 3.0, N_SITES)
    spread = rng.uniform(0.05, 1.5, N_SITES)
    return [1.0 / (1.0 + np.exp(-(centre + spread * rng.standard_normal((T, N_SITES))))) for T in LENGTHS]


def _histogram(psi, B):
    """(B, n) counts of (T, n) draws, binned as the device bins them: b = min(B - 1, (int)(psi B))."""
    b = np.minimum(B - 1, (psi * B).astype(np.int64))
    out = np.zeros((B, psi.shape[1]), dtype=np.int64)
    np.add.at(out, (b, np.broadcast_to(np.arange(psi.shape[1]), b.shape)), 1)
    return out


@pytest.fixture(scope='module')
def draws():
    return _draws()


@pytest.mark.parametrize('B', [4, 5, 64, 1024])
def test_site_intervals_against_numpy(draws, B):
    from occuspytial_amd.intervals import SiteIntervals
    counts = np.stack([_histogram(psi, B) for psi in draws])
    si = SiteIntervals(counts)
    pooled = np.sort(np.concatenate(draws), axis=0)          # (N, n), every site's pooled draws in order
    N = pooled.shape[0]
    assert si.bins == B and si.n_sites == N_SITES and si.resolution == 1.0 / B
    assert si.n_draws.tolist() == list(LENGTHS) and si.n_draws.shape == (3,)
    assert np.array_equal(si.per_chain_counts, counts)
    # the chains' merge is the histogram of the concatenated draws
    assert np.array_equal(si.per_chain_counts.sum(axis=0), _histogram(np.concatenate(draws), B))
    for frac in (Fraction(1, 40), Fraction(1, 2), Fraction(39, 40), Fraction(1, N), Fraction(1)):
        q = float(frac)
        k = max(1, math.ceil(frac * N))                      # (in whole numbers: no rounding of q N)
        kth = pooled[k - 1]
        lo, hi = si.bounds(q)
        assert lo.shape == hi.shape == (N_SITES,)
        assert np.all(lo <= kth) and np.all(kth < hi), (B, q)
        assert np.allclose(hi - lo, 1.0 / B, rtol=0, atol=1e-15)
        got = si.quantile(q)
        assert np.all(lo <= got) and np.all(got <= hi)
        assert np.abs(got - kth).max() < 1.0 / B, (B, q)
    assert np.array_equal(si.median, si.quantile(0.5))
    lo95, hi95 = si.interval()
    assert np.array_equal(lo95, si.quantile(0.025)) and np.array_equal(hi95, si.quantile(0.975))
    assert np.array_equal(si.width(), hi95 - lo95) and np.all(si.width() >= 0)
    lo50, hi50 = si.interval(0.5)
    assert np.array_equal(lo50, si.quantile(0.25)) and np.array_equal(hi50, si.quantile(0.75))
    allpsi = np.concatenate(draws)
    for j in range(B + 1):
        t = j / B
        direct = np.count_nonzero(np.minimum(B - 1, (allpsi * B).astype(np.int64)) >= j, axis=0) / N
        assert np.array_equal(si.prob_above(t), direct), (B, j)
    # between two edges: linear inside t's bin, so between the two exact neighbours
    mid = si.prob_above(0.3 / B + 2.0 / B)
    assert np.all(mid <= si.prob_above(2.0 / B)) and np.all(mid >= si.prob_above(3.0 / B))
    want = si.prob_above(3.0 / B) + 0.7 * (si.prob_above(2.0 / B) - si.prob_above(3.0 / B))
    assert np.abs(mid - want).max() < 1e-12
    assert 'SiteIntervals' in repr(si) and 'bins=%d' % B in repr(si) and str(list(LENGTHS)) in repr(si)


def test_site_intervals_edge_cases():
    from occuspytial_amd.intervals import SiteIntervals
    B, n = 8, 3
    # site 0: no draw at all; site 1: every draw in bin 5; site 2: psi exactly 1.0, which belongs to the last bin
    psi = np.column_stack([np.full(10, 0.5), np.full(10, 5.5 / B), np.ones(10)])
    counts = _histogram(psi, B)[None].copy()
    counts[0, :, 0] = 0
    si = SiteIntervals(counts)
    assert counts[0, B - 1, 2] == 10
    for q in (0.0, 0.025, 0.5, 1.0):
        lo, hi = si.bounds(q)
        assert np.isnan(lo[0]) and np.isnan(hi[0]) and np.isnan(si.quantile(q)[0])
        assert (lo[1], hi[1]) == (5 / B, 6 / B) and (lo[2], hi[2]) == ((B - 1) / B, 1.0)
    # ten draws in one bin: the k-th of them is put at (k - 1/2) / 10 of the bin
    assert si.quantile(0.5)[1] == 5 / B + (5 - 0.5) / 10 / B
    assert si.quantile(1.0)[2] == (B - 1) / B + 9.5 / 10 / B
    assert np.isnan(si.prob_above(0.5)[0]) and np.isnan(si.width()[0]) and np.isnan(si.median[0])
    assert si.prob_above(5 / B)[1] == 1.0 and si.prob_above(6 / B)[1] == 0.0 and abs(si.prob_above(5.25 / B)[1] - 0.75) < 1e-15
    assert si.prob_above(1.0)[2] == 0.0 and si.prob_above((B - 1) / B)[2] == 1.0 and si.prob_above(0.0)[2] == 1.0
    assert si.n_draws.tolist() == [10]
    empty = SiteIntervals(np.zeros((2, B, n)))
    assert empty.n_draws.tolist() == [0, 0] and np.all(np.isnan(empty.quantile(0.5))) and np.all(np.isnan(empty.prob_above(0.5)))
    assert 'SiteIntervals' in repr(empty)
    assert SiteIntervals(np.ones((1, B, n), dtype=np.uint32)).n_draws.tolist() == [B]         # (what the engine hands over)
    assert SiteIntervals(np.full((1, B, n), 3.0)).per_chain_counts.dtype == np.int64          # (whole numbers held in doubles)
    for bad in (np.zeros((B, n)), np.zeros((2, B, n, 1)), np.zeros((0, B, n)), np.zeros((1, 3, n)), np.zeros((1, 1025, n)),
                -np.ones((1, B, n)), np.full((1, B, n), 0.5), np.full((1, B, n), np.nan), np.zeros((1, B, n), dtype=object)):
        with pytest.raises(ValueError):
            SiteIntervals(bad)
    for q in (-0.1, 1.1):
        with pytest.raises(ValueError):
            si.quantile(q)
        with pytest.raises(ValueError):
            si.prob_above(q)
    for prob in (0.0, 1.0):
        with pytest.raises(ValueError):
            si.interval(prob)


# ---- sampler plumbing ----------------------------------------------------------------------------------------------
def test_site_intervals_argument_is_validated_and_refused_before_an_engine_exists(small, monkeypatch):
    from occuspytial_amd import LogitICARGibbs, LogitRSRGibbs, ProbitRSRGibbs, _engine
    from occuspytial_amd.gibbs.base import GibbsBase

    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(_engine.Engine, '__init__', no_engine)
    for sampler in (LogitICARGibbs(*small, random_state=1), LogitRSRGibbs(*small, random_state=1, q=10),
                    ProbitRSRGibbs(*small, random_state=1, q=10)):
        for value in (None, 1, 0, 3, 1025, 'yes', 64.0, 2.5, [True], np.ones(3, dtype=bool)):
            with pytest.raises(ValueError, match=MESSAGE):
                sampler.sample(5, chains=1, progressbar=False, site_intervals=value)
            with pytest.raises(ValueError, match=MESSAGE):
                sampler.resume({'n_chains': 1}, 5, progressbar=False, site_intervals=value)
        with pytest.raises(ValueError, match=MESSAGE):                                    # (looked at before anything else)
            sampler.sample(5, burnin=9, chains=0, progressbar=False, site_intervals=None)
    probit = ProbitRSRGibbs(*small, random_state=1, q=10)
    for value in (True, 16):
        with pytest.raises(NotImplementedError, match='site intervals are not available for the probit model'):
            probit.sample(5, chains=1, progressbar=False, site_intervals=value)
        with pytest.raises(NotImplementedError, match='site intervals are not available for the probit model'):
            probit.resume({'n_chains': 1}, 5, progressbar=False, site_intervals=value)

    class PyStep(GibbsBase):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._configure(a[0], None)

        def step(self):
            raise AssertionError('step was called')

    with pytest.raises(NotImplementedError, match='Python'):
        PyStep(*small, random_state=1).sample(5, site_intervals=True)
    with pytest.raises(ValueError, match=MESSAGE):                                        # (the argument is looked at first)
        PyStep(*small, random_state=1).sample(5, site_intervals=None)


class StandIn:
    """An object with the Engine interface whose histograms are its own: while the switch is on, every iteration past a
    ``run``'s burn-in draws a psi per chain and site and adds it to the chain's (B, n) counts, as the device does; switching
    on zeroes.  ``log`` keeps the calls in order, ``psi`` the draws that were counted."""

    def __init__(self, prob, n_chains, seed=5):
        self.prob, self.n_chains = prob, n_chains
        self.rng = np.random.default_rng(seed)
        self._sums_on = {}
        self._hist_bins = 0
        self.log, self.psi, self.counts = [], [[] for _ in range(n_chains)], None

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

    def hist_stats(self, bins):
        self.log.append(('on', int(bins)) if bins else 'off')
        if bins:
            self.counts = np.zeros((self.n_chains, int(bins), self.prob.n), dtype=np.uint32)
            self.psi = [[] for _ in range(self.n_chains)]
        self._hist_bins = int(bins)

    def hist_counts(self, chain=0):
        return {'bins': self.counts.shape[1], 'count': len(self.psi[chain]), 'counts': self.counts[chain]}

    def run(self, n_iter, burnin=0):
        keep, C, p = n_iter - burnin, self.n_chains, self.prob
        self.log.append(('run', n_iter, burnin, self._hist_bins))
        for c in range(C):
            for _ in range(keep if self._hist_bins else 0):
                psi = self.rng.uniform(size=p.n) ** (1 + c)
                self.psi[c].append(psi)
                self.counts[c] += _histogram(psi[None], self._hist_bins).astype(np.uint32)
        return np.zeros((C, keep, p.q)), np.zeros((C, keep, p.p)), np.ones((C, keep))


@pytest.mark.parametrize('progressbar', [False, True])
@pytest.mark.parametrize('asked, B', [(True, 64), (5, 5)])
def test_post_site_intervals_from_a_stand_in_engine(small, progressbar, asked, B):
    """60 iterations, 20 of them burn-in, 3 chains.  With the progress bar the call runs in chunks of 16: one whole chunk of
    burn-in with the switch off, the switch on before the chunk that straddles the boundary, and the engine's own window
    rule (counted past the chunk's burn-in) does the rest."""
    from occuspytial_amd import LogitICARGibbs
    from occuspytial_amd.intervals import SiteIntervals
    s = LogitICARGibbs(*small, random_state=3)
    prob = s._problem
    fake = StandIn(prob, 3)
    s.__dict__['_get_engine'] = lambda keys: fake
    out = s.sample(60, burnin=20, chains=3, progressbar=progressbar, site_intervals=asked)
    if progressbar:
        assert fake.log == ['off', ('run', 16, 15, 0), ('on', B), ('run', 16, 4, B), ('run', 16, 0, B), ('run', 12, 0, B)]
    else:
        assert fake.log == ['off', ('on', B), ('run', 60, 20, B)]
    si = out.site_intervals
    assert isinstance(si, SiteIntervals) and si.bins == B and si.n_sites == prob.n and si.n_draws.tolist() == [40, 40, 40]
    assert np.array_equal(si.per_chain_counts, fake.counts)
    pooled = np.sort(np.concatenate([np.stack(fake.psi[c]) for c in range(3)]), axis=0)
    assert pooled.shape == (120, prob.n)
    for q in (0.025, 0.5, 0.975):
        kth = pooled[{0.025: 3, 0.5: 60, 0.975: 117}[q] - 1]                    # k = ceil(q 120)
        lo, hi = si.bounds(q)
        assert np.all(lo <= kth) and np.all(kth < hi) and np.abs(si.quantile(q) - kth).max() < 1.0 / B
    # post.summary and the chains are what they are without the keyword
    assert sorted(out.data) == ['alpha', 'beta', 'tau'] and sorted(s.chain._names) == ['alpha', 'beta', 'tau']
    fake0 = StandIn(prob, 2)
    s.__dict__['_get_engine'] = lambda keys: fake0
    plain = s.sample(10, burnin=2, chains=2, progressbar=False)
    assert plain.site_intervals is None and fake0.log == [('run', 10, 2, 0)]
    fake0._hist_bins = 64                                                       # (a reused engine that an earlier call left on)
    s.sample(10, burnin=2, chains=2, progressbar=False)
    assert fake0.log[1:] == ['off', ('run', 10, 2, 0)]


def test_posterior_parameter_has_the_attribute():
    from occuspytial_amd.posterior import PosteriorParameter
    assert PosteriorParameter.site_intervals is None


def test_engine_binding_names():
    from occuspytial_amd._engine import Engine, EngineGroup
    for cls in (Engine, EngineGroup):
        assert callable(cls.hist_stats) and callable(cls.hist_counts)


def test_a_library_without_the_feature_is_refused_and_the_default_asks_nothing(cpu_abi, small, monkeypatch):  # noqa: F811
    """Every occ_get_state / occ_set_state call goes through a recording wrapper: with the default none names hist_*."""
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
    assert out.site_intervals is None and out['alpha'].shape[:2] == (1, 5)
    ckpt = s.checkpoint()
    assert not [key for key in ckpt if key.startswith('hist_')]
    s.resume(ckpt, 3, progressbar=False)
    assert asked and not [name for name in asked if name.startswith('hist_')]      # (the wrapper saw the other calls)
    with pytest.raises(ValueError, match=r'has no site intervals .*rebuild it'):
        LogitICARGibbs(*small, random_state=3).sample(5, chains=1, progressbar=False, site_intervals=True)
    assert [name for name in asked if name.startswith('hist_')] == ['hist_stats']
    with pytest.raises(ValueError, match=r'has no site intervals .*rebuild it'):
        s.resume(ckpt, 3, progressbar=False, site_intervals=16)
