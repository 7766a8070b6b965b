"""Spatial residual check, the parts that need no device: the state names in header and binding, the Philox stream, the
validation of ``spatial_check=``, the refusals of the probit sampler and of a sampler with a Python ``step``,
``post.spatial_check`` from a stand-in engine against direct numpy (ties in the p-value included), Moran's I from the four
sums against the directly centred formula, and the silence of the default."""
import os
import re

import numpy as np
import pytest
from scipy import sparse

from .conftest import ROOT, load_golden
from .test_api_cpu import _inputs
from .test_cpu_abi import cpu_abi  # noqa: F401  (the oracle's build of the C ABI, which does not know the moran_* names)

MORAN_NAMES = ('moran_stats', 'moran_draws')


@pytest.fixture(scope='module')
def small():
    return _inputs(load_golden('ref_queen150_ragged'))[:4]   # 150 sites, 100 surveyed, p = 3, q = 2


def test_every_moran_state_name_is_in_header_and_binding():
    from occuspytial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    comments = ' '.join(re.findall(r'/\*.*?\*/', header, flags=re.S))
    documented = set(re.findall(r'\b(moran_[a-z0-9]+)\b', comments))
    assert set(MORAN_NAMES) == documented, set(MORAN_NAMES) ^ documented
    assert tuple(_lib.MORAN_FIELDS) == MORAN_NAMES
    assert re.search(r'#define OCC_ABI_VERSION 7\b', header) and _lib.ABI_VERSION == 7   # no new function, no layout change
    assert not [name for name, _, _ in _lib.SYMBOLS if 'moran' in name or 'spatial' in name]
    assert re.search(r'\b14 \(STREAM_SPATIAL\)', comments)
    rng_hpp = open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'occ_rng.hpp')).read()
    assert re.search(r'STREAM_SPATIAL = 14\b', rng_hpp)
    streams = [int(v) for v in re.findall(r'STREAM_[A-Z_]+ = (\d+)', rng_hpp)]
    assert len(streams) == len(set(streams))                                             # (14 was free)
    # the switch is a word of the handle: not a fifth row of the z update's outputs
    assert not re.findall(r"moran_stats\(1\)\s+the chain's switch, 0 / 1", header)
    assert 'moran' not in open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'occ_plan.hpp')).read()


def test_spatial_check_argument_is_validated_and_refused_before_an_engine_exists(small, monkeypatch):
    from occuspytial_amd import LogitICARGibbs, LogitRSRGibbs, ProbitRSRGibbs, _engine
    from occuspytial_amd.gibbs.base import GibbsBase
    from occuspytial_amd.spatial import spatial_flag

    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(_engine.Engine, '__init__', no_engine)
    assert spatial_flag(True) is True and spatial_flag(False) is False and spatial_flag(np.bool_(True)) is True
    for sampler in (LogitICARGibbs(*small, random_state=1), LogitRSRGibbs(*small, random_state=1, q=10),
                    ProbitRSRGibbs(*small, random_state=1, q=10)):
        for value in (None, 1, 0, 'yes', 1.0, [True], np.ones(3, dtype=bool)):
            with pytest.raises(ValueError, match='spatial_check must be True or False'):
                sampler.sample(5, chains=1, progressbar=False, spatial_check=value)
            with pytest.raises(ValueError, match='spatial_check must be True or False'):
                sampler.resume({'n_chains': 1}, 5, progressbar=False, spatial_check=value)
    probit = ProbitRSRGibbs(*small, random_state=1, q=10)
    with pytest.raises(NotImplementedError, match='the spatial residual check is not available for the probit model'):
        probit.sample(5, chains=1, progressbar=False, spatial_check=True)
    with pytest.raises(NotImplementedError, match='not available for the probit model'):
        probit.resume({'n_chains': 1}, 5, progressbar=False, spatial_check=True)

    class PyStep(GibbsBase):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._configure(a[0], None)

        def step(self):
            raise AssertionError('step was called')

    with pytest.raises(NotImplementedError, match='Python'):
        PyStep(*small, random_state=1).sample(5, spatial_check=True)
    with pytest.raises(ValueError, match='spatial_check must be True or False'):      # (the argument is looked at first)
        PyStep(*small, random_state=1).sample(5, spatial_check=None)


def _lattice_weights(rows, cols):
    from occuspytial_amd.utils import rand_precision_mat
    Q = sparse.csr_matrix(rand_precision_mat(rows, cols))
    W = -Q.toarray()
    np.fill_diagonal(W, 0.0)
    return Q, W


def _weighted_graph(n=60, seed=4):
    rng = np.random.default_rng(seed)
    W = np.zeros((n, n))
    for i in range(n):
        for j in rng.choice(n, size=4, replace=False):
            if i != j:
                W[i, j] = W[j, i] = rng.uniform(0.2, 3.0)
    Q = sparse.csr_matrix(np.diag(W.sum(axis=1)) - W)
    return Q, W


def _sums(W, r):
    return r @ (W @ r), W.sum(axis=1) @ r, r.sum(), r @ r


def _moran_direct(W, r):
    d = r - r.mean()
    return len(r) / W.sum() * (d @ (W @ d)) / (d @ d)


@pytest.mark.parametrize('graph', ['lattice', 'weighted'])
def test_morans_i_from_the_four_sums_equals_the_centred_formula(graph):
    from occuspytial_amd.spatial import moran_from_sums, weights_total
    Q, W = _lattice_weights(9, 11) if graph == 'lattice' else _weighted_graph()
    n = W.shape[0]
    S0 = weights_total(Q)
    assert abs(S0 - W.sum()) <= 1e-12 * W.sum() and abs(weights_total(Q.toarray()) - S0) <= 1e-12 * S0
    rng = np.random.default_rng(1)
    for _ in range(20):
        psi = rng.uniform(0.05, 0.95, n)
        r = (rng.uniform(size=n) < psi) - psi + 0.2 * rng.standard_normal()      # (a mean well away from zero)
        got = float(moran_from_sums(*_sums(W, r), n, S0))
        assert abs(got - _moran_direct(W, r)) < 1e-12


class StandIn:
    """An object with the Engine interface whose rows are its own: every ``run`` makes up (keep, 8) rows per chain exactly
    when the switch is on -- the eight sums of residuals it draws itself, on a coarse grid so that ties happen; ``log`` keeps
    the calls in order."""

    def __init__(self, prob, W, n_chains, seed=5):
        self.prob, self.W, self.n_chains = prob, W, n_chains
        self.rng = np.random.default_rng(seed)
        self._sums_on = {}
        self._moran_on = False
        self.log, self.kept, self.resid, self._draws = [], [[] for _ in range(n_chains)], [[] for _ in range(n_chains)], None

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

    def moran_stats(self, on):
        self.log.append('on' if on else 'off')
        self._moran_on = bool(on)

    def moran_draws(self, chain=0):
        return self._draws[chain]

    def run(self, n_iter, burnin=0):
        keep, C, p = n_iter - burnin, self.n_chains, self.prob
        self.log.append(('run', n_iter, burnin, self._moran_on))
        self._draws = [np.zeros((0, 8)) for _ in range(C)]
        for c in range(C):
            if self._moran_on:
                rows = np.zeros((keep, 8))
                for t in range(keep):
                    r = self.rng.integers(-2, 3, p.n) / 4.0
                    rs = r if self.rng.uniform() < 0.3 else self.rng.integers(-2, 3, p.n) / 4.0   # (sometimes the same: a tie)
                    rows[t] = _sums(self.W, r) + _sums(self.W, rs)
                    self.resid[c].append((r, rs))
                self._draws[c] = rows
                self.kept[c].append(rows)
        return np.zeros((C, keep, p.q)), np.zeros((C, keep, p.p)), np.ones((C, keep))


@pytest.mark.parametrize('progressbar', [False, True])
def test_post_spatial_check_from_a_stand_in_engine(small, progressbar):
    """60 iterations, 20 of them burn-in, 3 chains.  With the progress bar the call runs in chunks of 16: one whole chunk of
    burn-in with the switch off, the switch on before the chunk that straddles the boundary, every chunk's rows appended."""
    from occuspytial_amd import LogitICARGibbs
    from occuspytial_amd.spatial import SpatialCheck
    s = LogitICARGibbs(*small, random_state=3)
    prob = s._problem
    W = -prob.Q.toarray()
    np.fill_diagonal(W, 0.0)
    fake = StandIn(prob, W, 3)
    s.__dict__['_get_engine'] = lambda keys: fake
    out = s.sample(60, burnin=20, chains=3, progressbar=progressbar, spatial_check=True)
    runs = [e for e in fake.log if isinstance(e, tuple)]
    if progressbar:
        assert runs == [('run', 16, 15, False), ('run', 16, 4, True), ('run', 16, 0, True), ('run', 12, 0, True)]
        assert fake.log[:3] == ['off', runs[0], 'on']
    else:
        assert fake.log == ['off', 'on', ('run', 60, 20, True)]
    sc = out.spatial_check
    assert isinstance(sc, SpatialCheck) and sc.n_draws == 120 and sc.n == prob.n and sc.expected == -1.0 / (prob.n - 1)
    assert abs(sc.S0 - W.sum()) <= 1e-12 * W.sum()
    assert sc.moran_obs.shape == (3, 40) and sc.moran_rep.shape == (3, 40)
    direct = np.array([[[_moran_direct(W, r), _moran_direct(W, rs)] for r, rs in fake.resid[c]] for c in range(3)])
    assert np.abs(sc.moran_obs - direct[:, :, 0]).max() < 1e-12 and np.abs(sc.moran_rep - direct[:, :, 1]).max() < 1e-12
    obs, rep = sc.moran_obs.ravel(), sc.moran_rep.ravel()
    ties = np.count_nonzero(rep == obs)
    assert ties > 0                                                            # (they count half)
    assert sc.p_value == (np.count_nonzero(rep > obs) + 0.5 * ties) / 120
    assert sc.excess == float(np.mean(sc.moran_obs) - np.mean(sc.moran_rep))
    assert 'p_value=%.3f' % sc.p_value in repr(sc) and 'excess' in repr(sc)
    # post.summary and the chains are what they are without the keyword
    assert sorted(out.data) == ['alpha', 'beta', 'tau'] and sorted(s.chain._names) == ['alpha', 'beta', 'tau']
    fake0 = StandIn(prob, W, 2)
    s.__dict__['_get_engine'] = lambda keys: fake0
    plain = s.sample(10, burnin=2, chains=2, progressbar=False)
    assert plain.spatial_check is None and fake0.log == [('run', 10, 2, False)]
    fake0._moran_on = True                                                     # (a reused engine that an earlier call left on)
    s.sample(10, burnin=2, chains=2, progressbar=False)
    assert fake0.log[1:] == ['off', ('run', 10, 2, False)]


def test_spatial_check_on_rows_with_ties_and_bad_shapes():
    from occuspytial_amd.spatial import SpatialCheck
    Q, W = _lattice_weights(4, 5)
    n, S0 = 20, W.sum()
    rng = np.random.default_rng(2)
    r = [rng.standard_normal(n) for _ in range(4)]
    rows = np.zeros((2, 2, 8))
    rows[0, 0] = _sums(W, r[0]) + _sums(W, r[0])          # a tie
    rows[0, 1] = _sums(W, r[1]) + _sums(W, r[2])
    rows[1, 0] = _sums(W, r[2]) + _sums(W, r[1])
    rows[1, 1] = _sums(W, r[3]) + _sums(W, r[3])          # a tie
    sc = SpatialCheck(rows, n, S0)
    assert sc.n_draws == 4 and sc.p_value == (1 + 0.5 * 2) / 4
    assert abs(sc.excess) < 1e-15
    empty = SpatialCheck(np.zeros((2, 0, 8)), n, S0)
    assert empty.n_draws == 0 and np.isnan(empty.p_value) and np.isnan(empty.excess) and 'SpatialCheck' in repr(empty)
    for bad in (np.zeros((2, 3)), np.zeros((2, 3, 4))):
        with pytest.raises(ValueError):
            SpatialCheck(bad, n, S0)


def test_engine_binding_names_and_checkpoint_key():
    from occuspytial_amd._engine import Engine, EngineGroup
    for cls in (Engine, EngineGroup):
        assert callable(cls.moran_stats) and callable(cls.moran_draws)


def test_a_library_without_the_feature_is_refused_and_the_default_asks_nothing(cpu_abi, small, monkeypatch):  # noqa: F811
    """Every occ_get_state / occ_set_state call goes through a recording wrapper: with the default none names moran_*."""
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
    assert out.spatial_check is None and out['alpha'].shape[:2] == (1, 5)
    ckpt = s.checkpoint()
    assert 'moran_stats' not in ckpt
    s.resume(ckpt, 3, progressbar=False)
    assert asked and not [name for name in asked if name.startswith('moran_')]    # (the wrapper saw the other calls)
    with pytest.raises(ValueError, match=r'has no spatial residual check .*rebuild it'):
        LogitICARGibbs(*small, random_state=3).sample(5, chains=1, progressbar=False, spatial_check=True)
    assert [name for name in asked if name.startswith('moran_')] == ['moran_stats']
