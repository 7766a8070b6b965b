"""Occupied sites per region and draw, the parts that need no device: the state names in header and binding, the validation
of ``regions=``, the refusal of a sampler with a Python ``step``, ``post['occupied']`` / ``post.regions`` / ``summary`` from a
stand-in engine against direct numpy, and the silence of the default."""
import os
import re

import numpy as np
import pytest

from .conftest import ROOT, load_golden
from .test_api_cpu import _inputs
from .test_cpu_abi import cpu_abi  # noqa: F401  (the oracle's build of the C ABI, which does not know the region_* names)

REGION_NAMES = ('region_id', 'region_stats', 'region_draws')


@pytest.fixture(scope='module')
def small():
    return _inputs(load_golden('ref_queen150_ragged'))[:4]   # 150 sites, 100 surveyed, p = 3, q = 2


def test_every_region_state_name_is_in_header_and_binding():
    from occuspytial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    comments = ' '.join(re.findall(r'/\*.*?\*/', header, flags=re.S))
    documented = set(re.findall(r'\b(region_[a-z0-9]+)\b', comments))
    assert set(REGION_NAMES) == documented, set(REGION_NAMES) ^ documented
    assert tuple(_lib.REGION_FIELDS) == REGION_NAMES
    assert re.search(r'#define OCC_ABI_VERSION 7\b', header) and _lib.ABI_VERSION == 7   # no new function, no layout change
    assert not [name for name, _, _ in _lib.SYMBOLS if 'region' in name]


def test_regions_argument_is_validated_before_an_engine_exists(small, monkeypatch):
    from occuspytial_amd import LogitICARGibbs, LogitRSRGibbs, ProbitRSRGibbs, _engine
    from occuspytial_amd.regions import region_ids

    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(_engine.Engine, '__init__', no_engine)
    n = small[2].shape[0]
    assert region_ids(None, n) is None
    assert np.array_equal(region_ids(True, n), np.zeros(n, dtype=np.int64))
    ids = np.arange(n) % 7 - 1
    assert np.array_equal(region_ids(ids.astype(np.int16), n), ids)
    assert np.array_equal(region_ids(ids.tolist(), n), ids)
    bad = [False, 3, 'all', ids.astype(float), ids[:-1], np.zeros((n, 1), dtype=int), ids == 0,
           np.full(n, -2), np.full(n, 256), [None] * n]
    for sampler in (LogitICARGibbs(*small, random_state=1), LogitRSRGibbs(*small, random_state=1, q=10),
                    ProbitRSRGibbs(*small, random_state=1, q=10)):
        for value in bad:
            with pytest.raises(ValueError, match='region'):
                sampler.sample(5, chains=1, progressbar=False, regions=value)
            with pytest.raises(ValueError, match='region'):
                sampler.resume({'n_chains': 1}, 5, progressbar=False, regions=value)
    assert np.array_equal(region_ids(np.full(n, 255), n), np.full(n, 255))


def test_a_python_step_sampler_refuses_regions(small, monkeypatch):
    """Raised before any engine exists: creating one here would need a device."""
    from occuspytial_amd import _engine
    from occuspytial_amd.gibbs.base import GibbsBase

    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(_engine.Engine, '__init__', no_engine)

    class PyStep(GibbsBase):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._configure(a[0], None)

        def step(self):
            raise AssertionError('step was called')

    with pytest.raises(NotImplementedError, match='Python'):
        PyStep(*small, random_state=1).sample(5, regions=True)
    with pytest.raises(ValueError, match='region'):      # (the argument is looked at first)
        PyStep(*small, random_state=1).sample(5, regions=False)


class StandIn:
    """An object with the Engine interface whose z history is its own: every ``run`` draws z per kept iteration (1 at the
    sites with a detection) and counts it by region exactly when the switch is on; ``log`` keeps the calls in order."""

    def __init__(self, prob, n_chains, seed=5):
        self.prob, self.n_chains = prob, n_chains
        self.rng = np.random.default_rng(seed)
        self._sums_on = {}
        self._regions, self._region_on = None, False
        self.log, self.z_kept, self._draws = [], [[] for _ in range(n_chains)], None
        self.det = np.zeros(prob.n, dtype=bool)
        self.det[np.asarray(prob.obs, dtype=int)] = True

    def set_keys(self, keys):
        pass

    def set_start(self, chain, alpha, beta, tau, eta):
        pass

    def set(self, name, value, chain=0):
        pass

    def get(self, name, chain=0):
        p = self.prob
        sizes = dict(alpha=p.q, beta=p.p, eta=p.n, z=p.n, omega_b=p.n, omega_a=p.R, theta=10, eps=p.n)
        if name == 'tau':
            return 1.0
        if name == 'exists':
            return np.ones(p.S)
        return np.ones(sizes[name])

    def regions(self, ids):
        assert not self._region_on
        self.log.append('map')
        self._regions = np.asarray(ids).copy()

    def region_stats(self, on):
        self.log.append('on' if on else 'off')
        self._region_on = bool(on)

    def region_draws(self, chain=0):
        return self._draws[chain]

    def run(self, n_iter, burnin=0):
        keep, C, p = n_iter - burnin, self.n_chains, self.prob
        self.log.append(('run', n_iter, burnin, self._region_on))
        G = int(self._regions.max()) + 1 if self._regions is not None else 1
        self._draws = [np.zeros((0, G)) for _ in range(C)]
        for c in range(C):
            z = (self.rng.uniform(size=(keep, p.n)) < 0.2 + 0.1 * c) | self.det
            if self._region_on:
                ids = self._regions
                self._draws[c] = np.stack([np.bincount(ids[(ids >= 0) & zt], minlength=G) for zt in z]).astype(float)
                self.z_kept[c].append(z)
        return np.zeros((C, keep, p.q)), np.zeros((C, keep, p.p)), np.ones((C, keep))


@pytest.mark.parametrize('progressbar', [False, True])
def test_occupied_regions_and_summary_from_a_stand_in_engine(small, progressbar):
    """60 iterations, 20 of them burn-in, 3 chains, 7 regions with every tenth site in none.  With the progress bar the call
    runs in chunks of 16: one whole chunk of burn-in with the switch off, the switch on before the chunk that straddles the
    boundary, every chunk's rows appended."""
    from occuspytial_amd import LogitICARGibbs
    s = LogitICARGibbs(*small, random_state=3)
    prob = s._problem
    n = prob.n
    ids = np.where(np.arange(n) % 10 == 9, -1, np.arange(n) % 7)
    fake = StandIn(prob, 3)
    s.__dict__['_get_engine'] = lambda keys: fake
    out = s.sample(60, burnin=20, chains=3, progressbar=progressbar, regions=ids)
    runs = [e for e in fake.log if isinstance(e, tuple)]
    if progressbar:
        assert runs == [('run', 16, 15, False), ('run', 16, 4, True), ('run', 16, 0, True), ('run', 12, 0, True)]
        assert fake.log[:3] == ['map', runs[0], 'on']
    else:
        assert fake.log == ['map', 'on', ('run', 60, 20, True)]
    occ = out['occupied']
    assert occ.shape == (3, 40, 7) and occ.dtype == np.float64
    z = np.stack([np.concatenate(fake.z_kept[c]) for c in range(3)])          # (chains, 40, n): the stand-in's own history
    want = np.stack([[np.bincount(ids[(ids >= 0) & zt], minlength=7) for zt in z[c]] for c in range(3)])
    assert np.array_equal(occ, want)
    assert s.chain['occupied'].shape == (40, 7)
    r = out.regions
    sizes = np.array([np.count_nonzero(ids == g) for g in range(7)])
    det = np.array([np.count_nonzero((ids == g) & fake.det) for g in range(7)])
    assert r.n_regions == 7 and np.array_equal(r.ids, ids)
    assert np.array_equal(r.sizes, sizes) and sizes.sum() == n - n // 10
    assert np.array_equal(r.detected, det) and det.sum() > 0
    assert np.array_equal(r.pao, want / sizes)
    assert r.occupied is not None and np.array_equal(r.occupied, occ)
    assert np.all(occ >= det) and np.all(occ <= sizes)
    summ = out.summary
    rows = list(summ.index) if hasattr(summ, 'index') else list(summ)
    assert all(f'occupied[{g}]' in rows for g in range(7))
    row = summ.loc['occupied[2]'] if hasattr(summ, 'loc') else summ['occupied[2]']
    assert abs(float(row['mean']) - want[:, :, 2].mean()) <= 0.006   # (a table may round to 2 decimals)
    # one region keeps its dimension: (chains, keep, 1)
    fake1 = StandIn(prob, 2)
    s.__dict__['_get_engine'] = lambda keys: fake1
    one = s.sample(10, burnin=2, chains=2, progressbar=False, regions=True)
    assert one['occupied'].shape == (2, 8, 1)
    assert np.array_equal(one['occupied'][:, :, 0], np.stack([np.concatenate(fake1.z_kept[c]).sum(1) for c in range(2)]))
    assert np.array_equal(one.regions.sizes, [n]) and np.array_equal(one.regions.detected, [fake1.det.sum()])
    # and without the keyword nothing of it exists
    fake0 = StandIn(prob, 2)
    s.__dict__['_get_engine'] = lambda keys: fake0
    plain = s.sample(10, burnin=2, chains=2, progressbar=False)
    assert plain.regions is None and 'occupied' not in plain.data and fake0.log == [('run', 10, 2, False)]


def test_region_occupancy_refuses_counts_of_the_wrong_shape():
    from occuspytial_amd.regions import RegionOccupancy
    ids = np.array([0, 1, 1, -1, 2])
    r = RegionOccupancy(ids, [1, 3], np.ones((2, 4, 3)))
    assert np.array_equal(r.sizes, [1, 2, 1]) and np.array_equal(r.detected, [0, 1, 0])      # (site 3 is in no region)
    with pytest.raises(ValueError):
        RegionOccupancy(ids, [1], np.ones((2, 4, 2)))


def test_a_library_without_the_feature_is_refused_and_the_default_asks_nothing(cpu_abi, small, monkeypatch):  # noqa: F811
    """Every occ_get_state / occ_set_state call goes through a recording wrapper: with the default none names region_*."""
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
    assert out.regions is None and out['alpha'].shape[:2] == (1, 5)
    ckpt = s.checkpoint()
    assert 'region_id' not in ckpt and 'region_stats' not in ckpt
    s.resume(ckpt, 3, progressbar=False)
    assert asked and not [name for name in asked if name.startswith('region_')]    # (the wrapper saw the other calls)
    with pytest.raises(ValueError, match=r'does not count the occupied sites per region .*rebuild it'):
        LogitICARGibbs(*small, random_state=3).sample(5, chains=1, progressbar=False, regions=True)
    assert [name for name in asked if name.startswith('region_')] == ['region_id']
