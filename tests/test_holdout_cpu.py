"""Held-out predictive scoring, the parts that need no device: the state names in header and binding, ``HoldoutScore``,
``compare`` and ``combine`` on synthetic sums against direct numpy, ``split``, ``holdout_arg``'s packing and its refusals, the
refusals of the probit sampler and of a sampler with a Python ``step``, ``post.holdout`` from a stand-in engine with its call
order written out, and the silence of the default."""
import os
import re

import numpy as np
import pytest
from scipy.special import logsumexp

from ._launch_text import assert_launched_only_while_on, unit_text
from .conftest import ROOT, load_golden
from .test_api_cpu import _inputs
from .test_cpu_abi import cpu_abi  # noqa: F401  (the oracle's build of the C ABI, which does not know the holdout_* names)

HOLDOUT_NAMES = ('holdout_data', 'holdout_stats', 'holdout_count', 'holdout_sums')


@pytest.fixture(scope='module')
def small():
    return _inputs(load_golden('ref_queen150_ragged'))[:4]   # 150 sites, 100 surveyed, p = 3, q = 2


def withheld(small, k=12, seed=0):
    """``k`` of the fixture's unsurveyed sites with withheld visits of 1 to 5 rows -> (W_test, y_test)."""
    Q, W, X, y = small
    rng = np.random.default_rng(seed)
    free = [i for i in range(X.shape[0]) if i not in W]
    Wt, yt = {}, {}
    for s in free[:k]:
        v = int(rng.integers(1, 6))
        w = rng.uniform(-2, 2, size=(v, 2))
        w[:, 0] = 1.0
        Wt[s], yt[s] = w, rng.binomial(1, 0.4, size=v)
    return Wt, yt


def synthetic(rng, C, N, H):
    """Log-likelihood draws (C, N, H) and detection probabilities of the same shape -> per chain the five slots (5, H)."""
    ll = -np.abs(rng.standard_normal((C, N, H)) * 2.0 + rng.uniform(0.5, 6.0, size=H))
    pd = rng.uniform(0, 1, size=(C, N, H)) * rng.uniform(0.1, 1.0, size=H)
    sums = [np.stack([np.full(H, float(N)), np.exp(ll[c]).sum(axis=0), ll[c].sum(axis=0), (ll[c] ** 2).sum(axis=0), pd[c].sum(axis=0)])
            for c in range(C)]
    return ll, pd, sums


def brute_auc(score, label):
    pos, neg = score[label], score[~label]
    wins = sum(float(p > n) + 0.5 * float(p == n) for p in pos for n in neg)
    return wins / (pos.size * neg.size)


# ---- names ---------------------------------------------------------------------------------------------------------
def test_every_holdout_state_name_is_in_header_and_binding():
    from occuspytial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    comments = ' '.join(re.findall(r'/\*.*?\*/', header, flags=re.S))
    documented = set(re.findall(r'\b(holdout_[a-z0-9]+)\b', comments))
    assert set(HOLDOUT_NAMES) == documented, set(HOLDOUT_NAMES) ^ documented
    assert tuple(_lib.HOLDOUT_FIELDS) == HOLDOUT_NAMES
    assert re.search(r'#define OCC_ABI_VERSION 7\b', header) and _lib.ABI_VERSION == 7   # no new function, no layout change
    assert not [name for name, _, _ in _lib.SYMBOLS if 'holdout' in name]
    # the switch is a word of the handle and the kernel is launched behind the z update: the planner does not know of it
    assert 'holdout' not in open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'occ_plan.hpp')).read()
    makefile = open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'Makefile')).read()
    # (the translation units are named once, in UNITS: the library and the stamps build compile them, SRC makes both depend on them)
    units = re.search(r'^UNITS := (.*)$', makefile, flags=re.M).group(1).split()
    assert units[:5] == ['occ_gibbs.hip', 'occ_spatial.hip', 'occ_hist.hip', 'occ_conv.hip', 'occ_holdout.hip']
    assert len(re.findall(r'-shared -o \$@ \$\(UNITS\)$', makefile, flags=re.M)) == 2
    assert re.search(r'^SRC := \$\(UNITS\) .*\bocc_holdout\.hpp\b', makefile, flags=re.M)


def test_the_kernel_is_launched_only_while_a_switch_is_on():
    """Read off launch_kind: the one call of holdout_launch stands behind `if (s->holdout.any)`, next to conv_launch in the
    branch of the z update; the word starts at 0, only switch_set raises it -- the one place that does, for every feature
    behind the z update -- and occ_profile clears it for its scope.  A run with the switch never touched enqueues what it
    enqueued before.  The unit has one kernel, no atomics and no LDS, and its guard is written as conv_counts_now writes it."""
    assert_launched_only_while_on('holdout')
    unit = unit_text('occ_holdout.hip')
    assert 'atomic' not in unit.lower() and '__shared__' not in unit and len(re.findall(r'__global__', unit)) == 1
    guard = r'return a\.on\[chain\] != 0u && a\.sums != nullptr && after == t \+ 1u && sc\.err == 0 && rel >= sc\.burnin;'
    assert re.search(guard, unit) and re.search(guard, unit_text('occ_conv.hip'))


# ---- HoldoutScore, compare, combine ---------------------------------------------------------------------------------
def test_score_equals_direct_numpy_on_synthetic_sums():
    from occuspytial_amd.holdout import HoldoutScore
    rng = np.random.default_rng(4)
    C, N, H = 3, 500, 41
    ll, pd, sums = synthetic(rng, C, N, H)
    sites = rng.permutation(1000)[:H]
    detected = rng.binomial(1, 0.5, size=H)
    hs = HoldoutScore(sums, sites, detected)
    pooled = ll.reshape(C * N, H)
    elpd_i = logsumexp(pooled, axis=0) - np.log(C * N)
    assert np.allclose(hs.elpd_i, elpd_i, rtol=1e-12, atol=0) and np.isclose(hs.elpd, elpd_i.sum(), rtol=1e-12)
    assert np.isclose(hs.se, np.sqrt(H * np.var(elpd_i, ddof=1)), rtol=1e-10)
    assert np.allclose(hs.mean_loglik_i, pooled.mean(axis=0), rtol=1e-12)
    p = pd.reshape(C * N, H).mean(axis=0)
    assert np.allclose(hs.p_detect, p, rtol=1e-12) and np.isclose(hs.brier, np.mean((p - detected) ** 2), rtol=1e-12)
    assert np.isclose(hs.auc, brute_auc(p, detected.astype(bool)), rtol=1e-12)
    assert hs.n_draws.tolist() == [N] * C and hs.n_sites == H and np.array_equal(hs.sites, sites) and hs.detected.dtype == bool
    assert np.all(hs.elpd_i >= hs.mean_loglik_i)                                 # Jensen
    # the dicts Engine.holdout_sums returns are taken as they are; chains pool by adding sums
    again = HoldoutScore([{'count': N, 'sums': s} for s in sums], sites, detected)
    assert np.array_equal(again.elpd_i, hs.elpd_i) and np.array_equal(hs.sums, np.sum(sums, axis=0))


def test_auc_ties_and_edge_cases():
    from occuspytial_amd.holdout import HoldoutScore, _auc
    score = np.array([0.1, 0.4, 0.4, 0.4, 0.8, 0.8, 0.2])
    label = np.array([0, 1, 0, 1, 1, 0, 0], dtype=bool)
    assert np.isclose(_auc(score, label), brute_auc(score, label))
    assert _auc(np.array([0.1, 0.9]), np.array([False, True])) == 1.0 and _auc(np.array([0.9, 0.1]), np.array([False, True])) == 0.0
    assert _auc(np.full(4, 0.5), np.array([0, 1, 0, 1], dtype=bool)) == 0.5       # all tied
    assert np.isnan(_auc(score, np.ones(7, dtype=bool))) and np.isnan(_auc(score, np.zeros(7, dtype=bool)))
    # every L underflowed at an entry: elpd_i is -inf there, and so is the total; the sum is not shifted
    sums = np.array([[10.0, 10.0], [0.0, 2.5], [-8000.0, -20.0], [6.4e6, 50.0], [1.0, 4.0]])
    hs = HoldoutScore([sums], [3, 9], [1, 0])
    assert hs.elpd_i[0] == -np.inf and np.isfinite(hs.elpd_i[1]) and hs.elpd == -np.inf and hs.mean_loglik_i[0] == -800.0
    one = HoldoutScore([sums[:, :1]], [3], [1])                                   # one entry: no standard error, no AUC
    assert np.isnan(one.se) and np.isnan(one.auc) and one.n_sites == 1
    for bad, match in (([sums[:4]], r'one \(5, H\) array'), ([sums, sums[:, :1]], r'one \(5, H\) array'), ([], r'one \(5, H\) array')):
        with pytest.raises(ValueError, match=match):
            HoldoutScore(bad, [3, 9], [1, 0])
    for cnt in ([10.0, 9.0], [0.5, 0.5], [-1.0, -1.0]):
        w = sums.copy()
        w[0] = cnt
        with pytest.raises(ValueError, match='cnt row'):
            HoldoutScore([w], [3, 9], [1, 0])
    with pytest.raises(ValueError, match='one 0 / 1 flag'):
        HoldoutScore([sums], [3, 9], [1, 2])
    with pytest.raises(ValueError, match='appears twice'):
        HoldoutScore([sums], [3, 3], [1, 0])


def test_compare_and_combine():
    from occuspytial_amd.holdout import HoldoutScore, combine, compare
    rng = np.random.default_rng(9)
    H = 30
    sites = np.arange(100, 100 + H)
    detected = rng.binomial(1, 0.5, size=H)
    ids = rng.integers(0, 2 ** 62, size=H).astype(np.uint64)
    _, _, sa = synthetic(rng, 2, 200, H)
    _, _, sb = synthetic(rng, 2, 200, H)
    a, b = HoldoutScore(sa, sites, detected, ids), HoldoutScore(sb, sites, detected, ids)
    cmp = compare(a, b)
    d = a.elpd_i - b.elpd_i
    assert np.isclose(cmp['elpd_diff'], d.sum(), rtol=1e-12) and np.isclose(cmp['se_diff'], np.sqrt(H * np.var(d, ddof=1)), rtol=1e-12)
    assert compare(b, a)['elpd_diff'] == -cmp['elpd_diff'] and sorted(cmp) == ['elpd_diff', 'se_diff']
    with pytest.raises(ValueError, match='different sites or different withheld data'):
        compare(a, HoldoutScore(sb, sites + 1, detected, ids))
    with pytest.raises(ValueError, match='different sites or different withheld data'):
        compare(a, HoldoutScore([s[:, :-1] for s in sb], sites[:-1], detected[:-1], ids[:-1]))
    with pytest.raises(ValueError, match='different sites or different withheld data'):
        compare(a, HoldoutScore(sb, sites, 1 - detected, ids))                   # the same sites, other histories
    other = ids.copy()
    other[4] ^= np.uint64(1)
    with pytest.raises(ValueError, match='different sites or different withheld data'):
        compare(a, HoldoutScore(sb, sites, detected, other))
    # combine: three disjoint folds, given out of order, equal the score of all entries at once, in ascending order of site
    cut = [slice(20, 30), slice(0, 7), slice(7, 20)]
    folds = [HoldoutScore([s[:, c] for s in sa], sites[c], detected[c], ids[c]) for c in cut]
    whole = combine(folds)
    assert np.array_equal(whole.sites, sites) and np.array_equal(whole.elpd_i, a.elpd_i) and np.array_equal(whole.data_ids, ids)
    assert whole.elpd == pytest.approx(a.elpd, rel=1e-13) and whole.se == pytest.approx(a.se, rel=1e-13)
    assert whole.brier == pytest.approx(a.brier, rel=1e-13) and whole.auc == pytest.approx(a.auc, rel=1e-13) and whole.n_sites == H
    assert whole.n_draws.tolist() == [200] * 6 and compare(whole, b)['elpd_diff'] == pytest.approx(cmp['elpd_diff'], rel=1e-12)
    with pytest.raises(ValueError, match='folds overlap'):
        combine([folds[0], folds[1], folds[0]])
    with pytest.raises(ValueError, match='at least one score'):
        combine([])


# ---- split ------------------------------------------------------------------------------------------------------------
def test_split_is_disjoint_covering_deterministic_and_keeps_blocks_whole(small):
    from occuspytial_amd.holdout import split
    _, W, _, y = small
    sites = sorted(W)
    for k, seed in ((5, 0), (3, None), (7, 12)):
        folds = list(split(W, y, k, seed=seed))
        assert len(folds) == k
        tests = [sorted(f[2]) for f in folds]
        assert sorted(s for t in tests for s in t) == sites                      # disjoint and covering
        assert max(map(len, tests)) - min(map(len, tests)) <= 1
        for Wtr, ytr, Wte, yte in folds:
            assert sorted(Wtr) == sorted(ytr) and sorted(Wte) == sorted(yte) and sorted(list(Wtr) + list(Wte)) == sites
            assert all(Wte[s] is W[s] and yte[s] is y[s] for s in Wte)
        assert [sorted(f[2]) for f in split(W, y, k, seed=seed)] == tests         # deterministic
    assert [sorted(f[2]) for f in split(W, y, 5, seed=0)] != [sorted(f[2]) for f in split(W, y, 5, seed=1)]
    blocks = {s: s // 10 for s in sites}                                          # spatial blocks of ten site numbers
    for blk in (blocks, np.arange(150) // 10):
        folds = list(split(W, y, 4, seed=3, blocks=blk))
        where = {}
        for f, (_, _, Wte, _) in enumerate(folds):
            for s in Wte:
                assert where.setdefault(blocks[s], f) == f                        # a block lies in one fold
        assert sorted(s for _, _, Wte, _ in folds for s in Wte) == sites
    for k in (1, 0, len(sites) + 1):
        with pytest.raises(ValueError, match='k must lie between 2 and the number of sites'):
            list(split(W, y, k))
    with pytest.raises(ValueError, match='k must lie between 2 and the number of blocks'):
        list(split(W, y, 16, blocks=blocks))
    with pytest.raises(ValueError, match='same sites as keys'):
        list(split(W, {s: y[s] for s in sites[1:]}, 3))


# ---- holdout_arg ------------------------------------------------------------------------------------------------------
def test_holdout_arg_packs_and_refuses(small):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.holdout import holdout_arg, unpack
    prob = FlatProblem(*small)
    Wt, yt = withheld(small)
    packed = holdout_arg((Wt, yt), prob)
    sites = sorted(Wt)
    H, R = len(sites), sum(len(yt[s]) for s in sites)
    assert packed.dtype == np.float64 and packed.size == 2 + 2 * H + 1 + R + R * 2 and packed[0] == H and packed[1] == R
    site, ptr, y, W = unpack(packed, 2)
    assert site.tolist() == sites and ptr.tolist() == np.concatenate([[0], np.cumsum([len(yt[s]) for s in sites])]).tolist()
    assert np.array_equal(y, np.concatenate([yt[s] for s in sites])) and np.array_equal(W, np.vstack([Wt[s] for s in sites]))
    shuffled = {s: Wt[s] for s in reversed(sites)}                               # the order of the keys does not matter
    assert np.array_equal(holdout_arg((shuffled, yt), prob), packed)
    assert np.array_equal(holdout_arg(({np.int64(s): Wt[s] for s in sites}, {np.int64(s): yt[s] for s in sites}), prob), packed)

    def refused(W, y, match):
        with pytest.raises(ValueError, match=match):
            holdout_arg((W, y), prob)
    s0 = sites[0]
    surveyed = int(prob.site_id[0])
    refused({**Wt, surveyed: Wt[s0]}, {**yt, surveyed: yt[s0]}, 'is surveyed in the fitted problem')
    refused(Wt, {s: yt[s] for s in sites[1:]}, 'same sites as keys')
    refused({**Wt, s0: np.ones((len(yt[s0]), 3))}, yt, 'must have 2 columns')
    refused({**Wt, s0: np.ones(len(yt[s0]))}, yt, 'must have 2 columns')
    refused(Wt, {**yt, s0: np.full(len(yt[s0]), 2)}, 'must hold 0 and 1 only')
    refused(Wt, {**yt, s0: np.full(len(yt[s0]), 0.5)}, 'must hold 0 and 1 only')
    refused(Wt, {**yt, s0: np.zeros(len(yt[s0]) + 1)}, 'same number of visits')
    refused({**Wt, s0: np.zeros((0, 2))}, {**yt, s0: np.zeros(0)}, 'same number of visits')
    refused({**Wt, s0: np.full((len(yt[s0]), 2), np.inf)}, yt, 'must be finite')
    refused({**Wt, 150: Wt[s0]}, {**yt, 150: yt[s0]}, r'outside \[0, 150\)')
    refused({**Wt, -1: Wt[s0]}, {**yt, -1: yt[s0]}, r'outside \[0, 150\)')
    refused({**Wt, 'a': Wt[s0]}, {**yt, 'a': yt[s0]}, 'integer site number')
    refused({}, {}, 'non-empty dicts')
    for bad in (None, 5, (Wt,), (Wt, yt, yt), (packed, packed), 'ab'):
        with pytest.raises(ValueError, match='pair .W_test, y_test.'):
            holdout_arg(bad, prob)
    with pytest.raises(ValueError, match='wrong length'):
        unpack(packed[:-1], 2)


# ---- the samplers ---------------------------------------------------------------------------------------------------------
def test_holdout_is_validated_and_refused_before_an_engine_exists(small, monkeypatch):
    from occuspytial_amd import LogitICARGibbs, LogitRSRGibbs, ProbitRSRGibbs, _engine
    from occuspytial_amd.gibbs.base import GibbsBase

    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(_engine.Engine, '__init__', no_engine)
    Wt, yt = withheld(small)
    surveyed = sorted(small[1])[0]
    for sampler in (LogitICARGibbs(*small, random_state=1), LogitRSRGibbs(*small, random_state=1, q=10)):
        for value, match in ((5, 'pair'), ((Wt,), 'pair'), (({}, {}), 'non-empty'), (({surveyed: Wt[sorted(Wt)[0]]}, {surveyed: [0]}), 'is surveyed')):
            with pytest.raises(ValueError, match=match):
                sampler.sample(5, chains=1, progressbar=False, holdout=value)
            with pytest.raises(ValueError, match=match):
                sampler.resume({'n_chains': 1}, 5, progressbar=False, holdout=value)
    probit = ProbitRSRGibbs(*small, random_state=1, q=10)
    with pytest.raises(NotImplementedError, match='held-out scoring is not available for the probit model'):
        probit.sample(5, chains=1, progressbar=False, holdout=(Wt, yt))
    with pytest.raises(NotImplementedError, match='held-out scoring is not available for the probit model'):
        probit.resume({'n_chains': 1}, 5, progressbar=False, holdout=(Wt, yt))

    class PyStep(GibbsBase):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._configure(a[0], None)

        def step(self):
            raise AssertionError('step was called')

    with pytest.raises(NotImplementedError, match='Python'):
        PyStep(*small, random_state=1).sample(5, holdout=(Wt, yt))


class StandIn:
    """An object with the Engine interface whose sums are its own: while the switch is on, every iteration past a ``run``'s
    burn-in adds one to every slot; setting the data or switching on zeroes.  ``log`` keeps the calls in order."""

    def __init__(self, prob, n_chains):
        self.prob, self.n_chains = prob, n_chains
        self._sums_on = {}
        self._holdout, self._holdout_on = None, False
        self.log, self.count = [], 0

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

    def holdout_data(self, W, y=None):
        assert y is None
        self.log.append(('data', int(W[0])))
        self._holdout, self._holdout_on, self.count = np.array(W), False, 0

    def holdout_stats(self, on):
        self.log.append('on' if on else 'off')
        self._holdout_on = bool(on)
        if on:
            self.count = 0

    def holdout_sums(self, chain=0):
        H = int(self._holdout[0])
        sums = np.full((5, H), float(self.count))
        sums[1] *= 0.5
        sums[2:4] *= -1.0
        return {'count': self.count, 'sums': sums}

    def run(self, n_iter, burnin=0):
        keep, C, p = n_iter - burnin, self.n_chains, self.prob
        self.log.append(('run', n_iter, burnin, self._holdout_on))
        if self._holdout_on:
            self.count += keep
        return np.zeros((C, keep, p.q)), np.zeros((C, keep, p.p)), np.ones((C, keep))


@pytest.mark.parametrize('progressbar', [False, True])
def test_post_holdout_from_a_stand_in_engine(small, progressbar):
    """60 iterations, 20 of them burn-in, 3 chains.  The data are set first, with every chain off.  With the progress bar the call
    runs in chunks of 16: one whole chunk of burn-in with the switch off, the switch on before the chunk that straddles the
    boundary, and the engine's own window rule (counted past the chunk's burn-in) does the rest."""
    from occuspytial_amd import LogitICARGibbs
    from occuspytial_amd.holdout import HoldoutScore
    s = LogitICARGibbs(*small, random_state=3)
    prob = s._problem
    Wt, yt = withheld(small)
    fake = StandIn(prob, 3)
    s.__dict__['_get_engine'] = lambda keys: fake
    out = s.sample(60, burnin=20, chains=3, progressbar=progressbar, holdout=(Wt, yt))
    if progressbar:
        assert fake.log == [('data', 12), ('run', 16, 15, False), 'on', ('run', 16, 4, True), ('run', 16, 0, True), ('run', 12, 0, True)]
    else:
        assert fake.log == [('data', 12), 'on', ('run', 60, 20, True)]
    hs = out.holdout
    assert isinstance(hs, HoldoutScore) and hs.n_sites == 12 and hs.n_draws.tolist() == [40, 40, 40] and hs.sites.tolist() == sorted(Wt)
    assert hs.detected.tolist() == [bool(np.any(yt[k])) for k in sorted(Wt)] and hs.data_ids.shape == (12,)
    assert np.allclose(hs.elpd_i, np.log(0.5)) and np.allclose(hs.p_detect, 1.0) and np.allclose(hs.mean_loglik_i, -1.0)
    # post.summary and the chains are what they are without the keyword
    assert sorted(out.data) == ['alpha', 'beta', 'tau'] and sorted(s.chain._names) == ['alpha', 'beta', 'tau']
    fake0 = StandIn(prob, 2)
    s.__dict__['_get_engine'] = lambda keys: fake0
    plain = s.sample(10, burnin=2, chains=2, progressbar=False)
    assert plain.holdout is None and fake0.log == [('run', 10, 2, False)]
    fake0._holdout_on = True                                                    # (a reused engine that an earlier call left on)
    s.sample(10, burnin=2, chains=2, progressbar=False)
    assert fake0.log[1:] == ['off', ('run', 10, 2, False)]


def test_posterior_parameter_and_engine_binding_names():
    from occuspytial_amd._engine import Engine, EngineGroup
    from occuspytial_amd.posterior import PosteriorParameter
    assert PosteriorParameter.holdout is None
    for cls in (Engine, EngineGroup):
        assert callable(cls.holdout_data) and callable(cls.holdout_stats) and callable(cls.holdout_sums)


def test_a_library_without_the_feature_is_refused_and_the_default_asks_nothing(cpu_abi, small, monkeypatch):  # noqa: F811
    """Every occ_get_state / occ_set_state call goes through a recording wrapper: with the default none names holdout_*."""
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
    assert out.holdout is None and out['alpha'].shape[:2] == (1, 5)
    ckpt = s.checkpoint()
    assert not [key for key in ckpt if key.startswith('holdout_')]
    s.resume(ckpt, 3, progressbar=False)
    assert asked and not [name for name in asked if name.startswith('holdout_')]      # (the wrapper saw the other calls)
    held = withheld(small)
    with pytest.raises(ValueError, match=r'has no held-out scoring .*rebuild it'):
        LogitICARGibbs(*small, random_state=3).sample(5, chains=1, progressbar=False, holdout=held)
    assert [name for name in asked if name.startswith('holdout_')] == ['holdout_data']
    with pytest.raises(ValueError, match=r'has no held-out scoring .*rebuild it'):
        s.resume(ckpt, 3, progressbar=False, holdout=held)
