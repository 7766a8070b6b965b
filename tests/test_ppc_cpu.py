"""Posterior predictive check, the parts that need no device: the state names in header and binding, the validation of
``ppc=``, the refusals of the probit sampler and of a sampler with a Python ``step``, ``post.ppc`` from a stand-in engine
against direct numpy on synthetic rows (ties in the p-value included), and the silence of the default."""
import os
import re

import numpy as np
import pytest

from .conftest import ROOT, load_golden
from .test_api_cpu import _inputs
from .test_cpu_abi import cpu_abi  # noqa: F401  (the oracle's build of the C ABI, which does not know the ppc_* names)

PPC_NAMES = ('ppc_stats', 'ppc_draws')


@pytest.fixture(scope='module')
def small():
    return _inputs(load_golden('ref_queen150_ragged'))[:4]   # 150 sites, 100 surveyed, p = 3, q = 2


def test_every_ppc_state_name_is_in_header_and_binding():
    from occuspytial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    comments = ' '.join(re.findall(r'/\*.*?\*/', header, flags=re.S))
    documented = set(re.findall(r'\b(ppc_[a-z0-9]+)\b', comments))
    assert set(PPC_NAMES) == documented, set(PPC_NAMES) ^ documented
    assert tuple(_lib.PPC_FIELDS) == PPC_NAMES
    assert re.search(r'#define OCC_ABI_VERSION 7\b', header) and _lib.ABI_VERSION == 7   # no new function, no layout change
    assert not [name for name, _, _ in _lib.SYMBOLS if 'ppc' in name]
    assert 'STREAM_PPC' in comments and re.search(r'\b13 \(STREAM_PPC\)', comments)
    rng_hpp = open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'occ_rng.hpp')).read()
    assert re.search(r'STREAM_PPC = 13\b', rng_hpp)
    streams = [int(v) for v in re.findall(r'STREAM_[A-Z_]+ = (\d+)', rng_hpp)]
    assert len(streams) == len(set(streams))                                             # (13 was free)


def test_ppc_argument_is_validated_and_refused_before_an_engine_exists(small, monkeypatch):
    from occuspytial_amd import LogitICARGibbs, LogitRSRGibbs, ProbitRSRGibbs, _engine
    from occuspytial_amd.gibbs.base import GibbsBase
    from occuspytial_amd.ppc import ppc_flag

    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(_engine.Engine, '__init__', no_engine)
    assert ppc_flag(True) is True and ppc_flag(False) is False and ppc_flag(np.bool_(True)) is True
    for sampler in (LogitICARGibbs(*small, random_state=1), LogitRSRGibbs(*small, random_state=1, q=10),
                    ProbitRSRGibbs(*small, random_state=1, q=10)):
        for value in (None, 1, 0, 'yes', 1.0, [True], np.ones(3, dtype=bool)):
            with pytest.raises(ValueError, match='ppc must be True or False'):
                sampler.sample(5, chains=1, progressbar=False, ppc=value)
            with pytest.raises(ValueError, match='ppc must be True or False'):
                sampler.resume({'n_chains': 1}, 5, progressbar=False, ppc=value)
    probit = ProbitRSRGibbs(*small, random_state=1, q=10)
    with pytest.raises(NotImplementedError, match='posterior predictive checks are not available for the probit model'):
        probit.sample(5, chains=1, progressbar=False, ppc=True)
    with pytest.raises(NotImplementedError, match='not available for the probit model'):
        probit.resume({'n_chains': 1}, 5, progressbar=False, ppc=True)

    class PyStep(GibbsBase):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._configure(a[0], None)

        def step(self):
            raise AssertionError('step was called')

    with pytest.raises(NotImplementedError, match='Python'):
        PyStep(*small, random_state=1).sample(5, ppc=True)
    with pytest.raises(ValueError, match='ppc must be True or False'):      # (the argument is looked at first)
        PyStep(*small, random_state=1).sample(5, ppc=None)


class StandIn:
    """An object with the Engine interface whose rows are its own: every ``run`` makes up (keep, 4) rows per chain exactly
    when the switch is on; ``log`` keeps the calls in order."""

    def __init__(self, prob, n_chains, seed=5):
        self.prob, self.n_chains = prob, n_chains
        self.rng = np.random.default_rng(seed)
        self._sums_on = {}
        self._ppc_on = False
        self.log, self.kept, self._draws = [], [[] for _ in range(n_chains)], None

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

    def ppc_stats(self, on):
        self.log.append('on' if on else 'off')
        self._ppc_on = bool(on)

    def ppc_draws(self, chain=0):
        return self._draws[chain]

    def run(self, n_iter, burnin=0):
        keep, C, p = n_iter - burnin, self.n_chains, self.prob
        self.log.append(('run', n_iter, burnin, self._ppc_on))
        self._draws = [np.zeros((0, 4)) for _ in range(C)]
        for c in range(C):
            if self._ppc_on:
                # discrepancies on a coarse grid, so that ties happen; counts around the observed constants
                rows = np.column_stack([self.rng.integers(0, 6, keep) / 4.0, self.rng.integers(0, 6, keep) / 4.0,
                                        self.rng.integers(100, 140, keep), self.rng.integers(40, 60, keep)]).astype(float)
                self._draws[c] = rows
                self.kept[c].append(rows)
        return np.zeros((C, keep, p.q)), np.zeros((C, keep, p.p)), np.ones((C, keep))


@pytest.mark.parametrize('progressbar', [False, True])
def test_post_ppc_from_a_stand_in_engine(small, progressbar):
    """60 iterations, 20 of them burn-in, 3 chains.  With the progress bar the call runs in chunks of 16: one whole chunk of
    burn-in with the switch off, the switch on before the chunk that straddles the boundary, every chunk's rows appended."""
    from occuspytial_amd import LogitICARGibbs
    from occuspytial_amd.ppc import PredictiveCheck
    s = LogitICARGibbs(*small, random_state=3)
    prob = s._problem
    fake = StandIn(prob, 3)
    s.__dict__['_get_engine'] = lambda keys: fake
    out = s.sample(60, burnin=20, chains=3, progressbar=progressbar, ppc=True)
    runs = [e for e in fake.log if isinstance(e, tuple)]
    if progressbar:
        assert runs == [('run', 16, 15, False), ('run', 16, 4, True), ('run', 16, 0, True), ('run', 12, 0, True)]
        assert fake.log[:3] == ['off', runs[0], 'on']
    else:
        assert fake.log == ['off', 'on', ('run', 60, 20, True)]
    rows = np.stack([np.concatenate(fake.kept[c]) for c in range(3)])          # (chains, 40, 4): the stand-in's own history
    pc = out.ppc
    assert isinstance(pc, PredictiveCheck) and pc.n_draws == 120
    for k, name in enumerate(('ft_obs', 'ft_rep', 'detections_rep', 'sites_detected_rep')):
        assert getattr(pc, name).shape == (3, 40) and np.array_equal(getattr(pc, name), rows[:, :, k])
    y_total, sites = int(np.count_nonzero(prob.y)), len(prob.obs)
    assert pc.detections == y_total and pc.sites_detected == sites
    obs, rep = rows[:, :, 0].ravel(), rows[:, :, 1].ravel()
    ties = np.count_nonzero(rep == obs)
    assert ties > 0                                                            # (the grid makes ties: they count half)
    assert pc.p_value == (np.count_nonzero(rep > obs) + 0.5 * ties) / 120
    assert pc.c_hat == obs.mean() / rep.mean()
    det, sit = rows[:, :, 2].ravel(), rows[:, :, 3].ravel()
    assert pc.p_detections == (np.count_nonzero(det > y_total) + 0.5 * np.count_nonzero(det == y_total)) / 120
    assert pc.p_sites_detected == (np.count_nonzero(sit > sites) + 0.5 * np.count_nonzero(sit == sites)) / 120
    assert 'p_value=%.3f' % pc.p_value in repr(pc) and 'c_hat' in repr(pc)
    # post.summary and the chains are what they are without the keyword
    assert sorted(out.data) == ['alpha', 'beta', 'tau'] and sorted(s.chain._names) == ['alpha', 'beta', 'tau']
    fake0 = StandIn(prob, 2)
    s.__dict__['_get_engine'] = lambda keys: fake0
    plain = s.sample(10, burnin=2, chains=2, progressbar=False)
    assert plain.ppc is None and fake0.log == [('run', 10, 2, False)]
    fake0._ppc_on = True                                                       # (a reused engine that an earlier call left on)
    s.sample(10, burnin=2, chains=2, progressbar=False)
    assert fake0.log[1:] == ['off', ('run', 10, 2, False)]


def test_predictive_check_on_rows_with_ties():
    from occuspytial_amd.ppc import PredictiveCheck, tail_probability
    rows = np.zeros((2, 3, 4))
    rows[0] = [[1.0, 2.0, 5, 2], [1.0, 1.0, 7, 3], [2.0, 1.0, 6, 3]]
    rows[1] = [[0.5, 0.5, 6, 4], [3.0, 4.0, 9, 1], [1.5, 0.25, 6, 3]]
    pc = PredictiveCheck(rows, detections=6, sites_detected=3)
    assert pc.n_draws == 6
    assert pc.p_value == (2 + 0.5 * 2) / 6
    assert pc.c_hat == (9.0 / 6) / (8.75 / 6)
    assert pc.p_detections == (2 + 0.5 * 3) / 6
    assert pc.p_sites_detected == (1 + 0.5 * 3) / 6
    assert tail_probability([1, 2, 3], 2) == 0.5 and np.isnan(tail_probability(np.zeros((2, 0)), 1))
    empty = PredictiveCheck(np.zeros((2, 0, 4)), 6, 3)
    assert empty.n_draws == 0 and np.isnan(empty.p_value) and np.isnan(empty.c_hat) and 'PredictiveCheck' in repr(empty)
    for bad in (np.zeros((2, 3)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError):
            PredictiveCheck(bad, 6, 3)


def test_a_library_without_the_feature_is_refused_and_the_default_asks_nothing(cpu_abi, small, monkeypatch):  # noqa: F811
    """Every occ_get_state / occ_set_state call goes through a recording wrapper: with the default none names ppc_*."""
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
    assert out.ppc is None and out['alpha'].shape[:2] == (1, 5)
    ckpt = s.checkpoint()
    assert 'ppc_stats' not in ckpt
    s.resume(ckpt, 3, progressbar=False)
    assert asked and not [name for name in asked if name.startswith('ppc_')]    # (the wrapper saw the other calls)
    with pytest.raises(ValueError, match=r'has no posterior predictive check .*rebuild it'):
        LogitICARGibbs(*small, random_state=3).sample(5, chains=1, progressbar=False, ppc=True)
    assert [name for name in asked if name.startswith('ppc_')] == ['ppc_stats']
