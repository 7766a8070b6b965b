"""Per-site intervals, accumulated on the device (state names ``hist_stats``, ``hist_count``, ``hist_counts``;
csrc/occ_hist.hpp).

Per iteration past a call's burn-in one kernel behind the z update adds, per site of a chain whose switch is on, one count to
the bin of psi = expit(x beta + eta) among B equal bins on (0, 1).  Integer counts do not depend on path, placement or block
size, so every comparison between two ways of running the engine is equality, and so is the comparison with numpy away from
the bin edges: a (site, iteration) pair whose numpy psi lies within 1e-11 of an edge j / B -- ten times the project's 1e-12
bound on psi (tests/test_gpu_site_summaries.py) -- may fall into either neighbouring bin and is left out; the expected share
of such pairs is 2e-11 B <= 2e-8, the condition at most 1 in 10^4 per case, and every test prints how many it left out
(on one MI355X: 0 of the 82 728 pairs of the nine restatement cases, 0 of the 26 520 of the bracket test).
Workloads: 13x17 and 30x40 queen lattices, the weighted 300-node graph of the golden fixtures, 17x19 with nine covariates of
each kind (the generic kernels), the reduced-rank model at 40 columns.  Every test runs under its own time limit.
"""
import ctypes
import itertools

import numpy as np
import pytest
from scipy.special import expit

from ._outputs_gpu import engine_with, time_limit as _time_limit, two_calls  # noqa: F401 (autouse in this module)
from .test_gpu_parity import KEY, _problem_from_golden, _random_start
from .test_gpu_ppc import SCHED_KEYS
from .test_gpu_site_summaries import _rsr_problem, _workload_a, _workload_g

pytestmark = pytest.mark.gpu
EDGE = 1e-11


# ------------------------------------------------------------------ helpers
def _engine(prob, keys, starts, bins=64, **kw):
    return engine_with(prob, keys, starts, bins=bins, **kw)


def _hists(eng):
    return [eng.hist_counts(c) for c in range(eng.n_chains)]


def _two_calls(prob, keys, starts, split=((33, 4), (10, 0)), **kw):
    """run(33, 4) then run(10, 0) -> per chain the histograms of the 39 iterations past the calls' burn-in."""
    return two_calls(lambda: _engine(prob, keys, starts, **kw), _hists, split)


def _same(a, b):
    assert len(a) == len(b)
    for c, (u, v) in enumerate(zip(a, b)):
        assert u['bins'] == v['bins'] and u['count'] == v['count'], (c, u['count'], v['count'])
        assert u['counts'].dtype == np.uint32 and u['counts'].shape == v['counts'].shape
        assert np.array_equal(u['counts'], v['counts']), (c, np.count_nonzero(u['counts'] != v['counts']))


def _whole(hists, count):
    """Every chain counted `count` iterations, and every site's bins sum to that."""
    for h in hists:
        assert h['count'] == count and np.all(h['counts'].sum(axis=0, dtype=np.int64) == count)


def _psi(prob, eng, chain):
    """psi of the iteration the chain has just completed, from beta and eta read back (reduced rank: K theta as stored), as
    tests/test_gpu_site_summaries.py forms it."""
    return expit(prob.X @ eng.get('beta', chain) + eng.get('eta', chain))


def _bin(psi, B):
    """-> (the bin of every psi as the device takes it, whether psi lies within EDGE of an edge j / B)."""
    x = psi * B
    return np.minimum(B - 1, x.astype(np.int64)), np.abs(x - np.rint(x)) <= EDGE * B


def _lattice(rows, cols, chains, seed):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(rows, cols, visits=3, p=2, q=2, random_state=seed)
    prob = FlatProblem(Q, W, X, y)
    return prob, [KEY + 13 * c for c in range(chains)], [_random_start(prob, 40 + c) for c in range(chains)]


WORKLOADS = {
    'queen13x17': lambda chains: _lattice(13, 17, chains, 6),                       # 221 sites: one partial workgroup, no multiple of 64
    'queen30x40': lambda chains: _workload_a(chains),                               # 1 200 sites: five workgroups, the last partial
    'weighted300': lambda chains: (lambda pr: (pr[0], [KEY], [pr[1]]))(_problem_from_golden('ref_graph300_weighted')),
    'generic': lambda chains: _workload_g(),                                        # p = q = 9
    'rsr40': lambda chains: _rsr_problem(40),
}


# ------------------------------------------------------------------ 1: restatement
CASES = [('queen13x17', 1, 64), ('queen13x17', 2, 64), ('queen13x17', 4, 64), ('queen13x17', 2, 5), ('queen13x17', 2, 1024),
         ('queen30x40', 2, 64), ('weighted300', 1, 64), ('generic', 1, 64), ('rsr40', 2, 64)]


@pytest.mark.parametrize('name, chains, B', CASES)
def test_counts_equal_their_restatement_in_numpy(name, chains, B):
    """Twelve iterations as twelve run(1, 0) calls.  After each, beta and eta of every chain are read back, psi is formed in
    numpy and binned, and the bins are accumulated.  At the end hist_counts equals the accumulation exactly at every site
    without a pair within 1e-11 of an edge; a site with such pairs may hold each of them in either neighbouring bin.  The
    same twelve iterations as one run(12, 0) give equal counts."""
    prob, keys, starts = WORKLOADS[name](chains)
    n, C = prob.n, len(keys)
    eng = _engine(prob, keys, starts, bins=B)
    assert [eng.get('hist_stats', c)[0] for c in range(C)] == [float(B)] * C
    sure = np.zeros((C, B, n), dtype=np.int64)       # pairs away from every edge
    slack = np.zeros((C, B, n), dtype=np.int64)      # pairs within EDGE of one: both neighbouring bins may hold them
    site = np.arange(n)
    left_out = 0
    for _ in range(12):
        eng.run(1, 0)
        for c in range(C):
            psi = _psi(prob, eng, c)
            assert np.all((psi >= 0) & (psi <= 1))
            b, near = _bin(psi, B)
            np.add.at(sure[c], (b[~near], site[~near]), 1)
            j = np.rint(psi[near] * B).astype(np.int64)
            for side in (np.clip(j - 1, 0, B - 1), np.clip(j, 0, B - 1)):
                np.add.at(slack[c], (side, site[near]), 1)
            left_out += int(near.sum())
    print(name, chains, B, 'pairs left out for lying within 1e-11 of a bin edge: %d of %d' % (left_out, 12 * C * n))
    assert left_out * 10 ** 4 <= 12 * C * n
    stepped = _hists(eng)
    eng.close()
    _whole(stepped, 12)
    for c in range(C):
        got = stepped[c]['counts'].astype(np.int64)
        assert stepped[c]['bins'] == B and got.shape == (B, n)
        clean = slack[c].sum(axis=0) == 0
        assert np.array_equal(got[:, clean], sure[c][:, clean]), (name, c, np.count_nonzero(got[:, clean] != sure[c][:, clean]))
        assert np.all(got >= sure[c]) and np.all(got <= sure[c] + slack[c])
    assert sum(int(np.count_nonzero(h['counts'])) for h in stepped) > C * n       # (psi moves: more than one bin per site on average)
    one = _engine(prob, keys, starts, bins=B)
    one.run(12, 0)
    _same(_hists(one), stepped)
    one.close()


# ------------------------------------------------------------------ 2: the bracket
def test_bounds_bracket_the_order_statistics_of_the_draws():
    """Sixty iterations on the 13x17 lattice, two chains, psi of every one kept on the host.  SiteIntervals.bounds(q) from the
    device's counts brackets the k-th smallest pooled draw, k = ceil(120 q), at every site whose draws all lie away from the
    edges, and quantile(q) is within 1 / B of it."""
    from occuspytial_amd.intervals import SiteIntervals
    prob, keys, starts = WORKLOADS['queen13x17'](2)
    B = 64
    eng = _engine(prob, keys, starts, bins=B)
    draws = []
    for _ in range(60):
        eng.run(1, 0)
        draws += [_psi(prob, eng, c) for c in range(2)]
    si = SiteIntervals.from_engine(eng)
    eng.close()
    draws = np.sort(np.stack(draws), axis=0)
    near = _bin(draws, B)[1]
    print('pairs left out for lying within 1e-11 of a bin edge: %d of %d' % (near.sum(), near.size))
    assert near.sum() * 10 ** 4 <= near.size
    clean = ~near.any(axis=0)
    assert si.n_draws.tolist() == [60, 60] and si.bins == B and si.n_sites == prob.n
    for q, k in ((0.025, 3), (0.5, 60), (0.975, 117)):
        kth = draws[k - 1]
        lo, hi = si.bounds(q)
        assert np.all(lo[clean] <= kth[clean]) and np.all(kth[clean] < hi[clean]), q
        assert np.abs(si.quantile(q) - kth)[clean].max() < 1.0 / B
    assert np.all(si.width() >= 0) and np.all(si.prob_above(0.0) == 1.0)


# ------------------------------------------------------------------ 3: bit-equal counts whatever the path
@pytest.fixture(scope='module')
def ref_a():
    """Workload A, two chains, run(33, 4) then run(10, 0), on the default path: computed once, never changed."""
    prob, keys, starts = _workload_a(2)
    ref = _two_calls(prob, keys, starts)
    _whole(ref, 39)
    for h in ref:
        h['counts'].setflags(write=False)
    return ref


def test_differently_split_calls_give_the_same_counts(ref_a):
    prob, keys, starts = _workload_a(2)
    _same(ref_a, _two_calls(prob, keys, starts, split=((5, 4), (28, 0), (3, 0), (7, 0))))
    _same(ref_a, _two_calls(prob, keys, starts, split=((5, 4), (1, 0), (37, 0))))     # (a call of one iteration)


def test_occ_step_counts():
    """occ_step's window has burn-in 0: eager steps count like the iterations of a replayed graph, also between two runs."""
    prob, keys, starts = _workload_a(2)
    eng = _engine(prob, keys, starts)
    eng.run(4, 4 - 1)                 # (the three iterations of burn-in are not counted, the fourth is)
    for _ in range(9):
        eng.step()
    eng.run(29, 0)
    got = _hists(eng)
    eng.close()
    prob, keys, starts = _workload_a(2)
    other = _two_calls(prob, keys, starts, split=((4, 3), (38, 0)))
    _whole(got, 39)
    _same(got, other)


@pytest.mark.parametrize('env', [{'OCC_EVENT_SYNC': '1'}, {'OCC_EVENT_SYNC': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_CU_SPLIT': '0'},
                                 {'OCC_DEBUG_STREAMS_SERIALISED': '1'},
                                 {'OCC_NO_SIDE_STREAM': '1'}, {'OCC_EAGER_ONLY': '1'}, {'OCC_NO_XCD_LOCAL': '1'},
                                 {'OCC_NO_XCD_LOCAL': '1', 'OCC_CU_SPLIT': '0'},
                                 {'OCC_NO_PERSISTENT': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_NO_PERSISTENT': '1', 'OCC_NO_SIDE_STREAM': '1'}])
def test_every_scheduling_mode_gives_the_same_counts(monkeypatch, env):
    """Graph replay against eager stepping (OCC_EAGER_ONLY) and every other way of scheduling an iteration."""
    prob, keys, starts = _workload_a(2)
    for k in SCHED_KEYS:
        monkeypatch.delenv(k, raising=False)
    ref = _two_calls(prob, keys, starts)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _same(ref, _two_calls(prob, keys, starts))


@pytest.mark.parametrize('name', ['generic', 'rsr40', 'weighted300'])
def test_graph_replay_equals_eager_stepping_on_the_other_kernels(monkeypatch, name):
    prob, keys, starts = WORKLOADS[name](2)
    monkeypatch.delenv('OCC_EAGER_ONLY', raising=False)
    ref = _two_calls(prob, keys, starts)
    _whole(ref, 39)
    monkeypatch.setenv('OCC_EAGER_ONLY', '1')
    _same(ref, _two_calls(prob, keys, starts))


def test_tile_looping_kernel_gives_the_counts_of_launch_per_step(monkeypatch):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(61, 67, visits=3, p=2, q=2, random_state=5)
    prob = FlatProblem(Q, W, X, y)
    keys = [KEY + 7 * c for c in range(2)]
    starts = [_random_start(prob, 11 + c) for c in range(2)]
    monkeypatch.setenv('OCC_FORCE_TILES', '1')
    out = {}
    for mode in ('tiles', 'launch_per_step'):
        monkeypatch.delenv('OCC_NO_PERSISTENT', raising=False)
        if mode == 'launch_per_step':
            monkeypatch.setenv('OCC_NO_PERSISTENT', '1')
        eng = _engine(prob, keys, starts)
        assert eng.stats()['persistent_solve'] == (3 if mode == 'tiles' else 0)
        eng.run(24, 3)
        out[mode] = _hists(eng)
        assert eng.stats()['fused_fallbacks'] == 0
        eng.close()
    _whole(out['tiles'], 21)
    _same(out['tiles'], out['launch_per_step'])


def test_batched_chains_have_the_counts_of_single_chain_runs():
    prob, _ = _problem_from_golden('ref_graph300_weighted')
    keys = [KEY, KEY ^ 0xABCDEF, 12345]
    rng = np.random.default_rng(3)
    starts = [dict(alpha=rng.standard_normal(prob.q), beta=rng.standard_normal(prob.p), tau=1.0 + c,
                   eta=(lambda e: e - e.mean())(rng.standard_normal(prob.n))) for c in range(3)]
    batch = _engine(prob, keys, starts)
    batch.run(20, 4)
    both = _hists(batch)
    batch.close()
    _whole(both, 16)
    for c in range(3):
        solo = _engine(prob, [keys[c]], [starts[c]])
        solo.run(20, 4)
        _same([both[c]], _hists(solo))
        solo.close()


def test_engine_group_switches_everywhere_and_routes_by_chain():
    from occuspytial_amd._engine import Engine, EngineGroup
    prob, keys, starts = _workload_a(3)
    grp = EngineGroup(prob, keys, [0, 0], engine_factory=lambda pr, ks, dev: Engine(pr, ks, device=dev))
    for c in range(3):
        grp.set_start(c, **starts[c])
    assert grp._hist_bins == 0
    grp.hist_stats(64)
    assert grp._hist_bins == 64
    grp.run(20, 5)
    ck = grp.checkpoint()
    assert ck['hist_stats'].tolist() == [64.0] * 3 and ck['hist_count'].tolist() == [15] * 3
    assert ck['hist_counts'].shape == (3, 64, prob.n) and ck['hist_counts'].dtype == np.uint32
    grp.restore(ck)
    grp.run(10, 0)
    got = [grp.hist_counts(c) for c in range(3)]
    grp.close()
    _same(_two_calls(prob, keys, starts, split=((20, 5), (10, 0))), got)


SWITCHES = [combo for combo in itertools.product((False, True), repeat=5) if any(combo)]


@pytest.fixture(scope='module')
def ref_short():
    prob, keys, starts = _workload_a(2)
    return _two_calls(prob, keys, starts, split=((12, 3), (5, 0)))


@pytest.mark.parametrize('site, ll, regions, ppc, moran', SWITCHES)
def test_counts_are_the_same_beside_every_other_switch(ref_short, site, ll, regions, ppc, moran):
    prob, keys, starts = _workload_a(2)
    ids = (np.arange(prob.n) % 7).astype(np.int64) if regions else None
    eng = _engine(prob, keys, starts, site=site, ll=ll, ids=ids, ppc=ppc, moran=moran)
    eng.run(12, 3)
    eng.run(5, 0)
    got = _hists(eng)
    _same(ref_short, got)
    _whole(got, 14)
    if site:                         # both follow the rule of the site sums: every iteration past a call's burn-in
        assert [eng.site_sums(c)['count'] for c in range(2)] == [h['count'] for h in got]
    eng.close()


# ------------------------------------------------------------------ 4: a re-run call counts nothing twice
def _headline_counts(iters=10):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(100, 100, visits=5, p=2, q=2, random_state=0)
    prob = FlatProblem(Q, W, X, y)
    eng = _engine(prob, [KEY + 5 * c for c in range(4)], [_random_start(prob, 60 + c) for c in range(4)])
    eng.run(iters, 0)
    eng.run(7, 2)
    out = _hists(eng), eng.stats()
    eng.close()
    return out


def _rsr_counts():
    prob, keys, starts = _rsr_problem(40)
    eng = _engine(prob, keys, starts)
    eng.run(8, 0)
    eng.run(5, 1)
    out = _hists(eng), eng.stats()
    eng.close()
    return out


@pytest.fixture(scope='module')
def ref_headline():
    ref, st = _headline_counts()
    assert st['fused_fallbacks'] == 0
    _whole(ref, 15)
    return ref


def test_a_call_rerun_after_a_barrier_timeout_counts_no_iteration_twice(monkeypatch, ref_headline):
    """The knobs of tests/test_gpu_site_summaries.py's test of the same name, with the histograms on: a bounded wait gives up,
    the call is re-run from the snapshot, which holds the counts."""
    monkeypatch.setenv('OCC_CU_SPLIT', '32')
    monkeypatch.setenv('OCC_DEBUG_SKIP_RESIDENCY_PROBE', '1')
    monkeypatch.setenv('OCC_QUIET', '1')
    alt, st = _headline_counts()
    assert st['fused_fallbacks'] == 1
    _whole(alt, 15)
    _same(ref_headline, alt)


def test_a_call_rerun_after_a_broken_handover_counts_no_iteration_twice(monkeypatch, ref_headline):
    """Likewise with the broken hand-over: fused ICAR path and reduced-rank model."""
    monkeypatch.setenv('OCC_QUIET', '1')
    rsr_ref, _ = _rsr_counts()
    monkeypatch.setenv('OCC_DEBUG_BREAK_HANDOVER', '1')
    alt, st = _headline_counts()
    assert st['fused_fallbacks'] == 1
    _whole(alt, 15)
    _same(ref_headline, alt)
    rsr_alt, rst = _rsr_counts()
    assert rst['fused_fallbacks'] == 1
    _whole(rsr_alt, 12)
    _same(rsr_ref, rsr_alt)


# ------------------------------------------------------------------ 5: nothing else sees the switch
@pytest.mark.parametrize('name', ['queen30x40', 'generic', 'rsr40'])
def test_nothing_else_sees_the_switch(name):
    """alpha, beta, tau, eta, z, the site_* and ll_* sums, region_draws, ppc_draws and moran_draws are the same bits with
    hist_stats on and off."""
    prob, keys, starts = WORKLOADS[name](2)
    ids = (np.arange(prob.n) % 7).astype(np.int64)
    engines = {}
    for which in ('on', 'off'):
        eng = engines[which] = _engine(prob, keys, starts, bins=64 if which == 'on' else 0, site=True, ll=True, ids=ids, ppc=True,
                                       moran=True)
        eng.rec = eng.run(33, 4) + eng.run(10, 0)
    on, off = engines['on'], engines['off']
    for u, v in zip(on.rec, off.rec):
        assert np.array_equal(u, v)
    for c in range(len(keys)):
        for nm in ('alpha', 'beta', 'eta', 'z') + (('theta',) if name.startswith('rsr') else ()):
            assert np.array_equal(on.get(nm, c), off.get(nm, c)), nm
        assert on.get('tau', c) == off.get('tau', c)
        a, b = on.site_sums(c), off.site_sums(c)
        assert a['count'] == b['count'] == 39 and all(np.array_equal(a[k], b[k]) for k in ('psi', 'occ', 'z', 'eta', 'eta2'))
        a, b = on.loglik_sums(c), off.loglik_sums(c)
        assert a['count'] == b['count'] == 39 and all(np.array_equal(a[k], b[k]) for k in ('lik', 'log', 'log2'))
        assert np.array_equal(on.region_draws(c), off.region_draws(c)) and on.region_draws(c).shape == (10, 7)
        assert np.array_equal(on.ppc_draws(c), off.ppc_draws(c)) and on.ppc_draws(c).shape == (10, 4)
        assert np.array_equal(on.moran_draws(c), off.moran_draws(c)) and on.moran_draws(c).shape == (10, 8)
    _whole(_hists(on), 39)
    with pytest.raises(ValueError, match='set hist_stats first'):       # (the other handle never heard of them)
        off.get('hist_count')
    for eng in engines.values():
        eng.close()


# ------------------------------------------------------------------ 6: windows, switches per chain
def test_windows_and_a_chain_that_does_not_count():
    """120 iterations, 100 past the burn-in, four chains of which the last has its switch off; switching a chain on again
    zeroes its part alone; off keeps everything readable."""
    prob, keys, starts = _workload_a(4)
    eng = _engine(prob, keys, starts)
    eng.set('hist_stats', 0.0, 3)
    eng.run(120, 20)
    got = _hists(eng)
    _whole(got[:3], 100)
    _whole(got[3:], 0)
    assert [eng.get('hist_stats', c)[0] for c in range(4)] == [64.0, 64.0, 64.0, 0.0]
    eng.set('hist_stats', 64.0, 1)                    # on again: zeroes chain 1 alone
    after = _hists(eng)
    _whole(after[1:2], 0)
    _same([got[0], got[2]], [after[0], after[2]])
    eng.set('hist_stats', 0.0, 0)                     # off: stays readable, stops counting
    eng.set_start(1, **starts[1])                     # occ_set_start and occ_set_keys do not touch the switch
    eng.set_keys(keys)
    eng.run(6, 1)
    last = _hists(eng)
    _same([got[0]], [last[0]])
    _whole(last[1:2], 5)
    _whole(last[2:3], 105)
    eng.close()


# ------------------------------------------------------------------ 7: the interface
@pytest.mark.parametrize('name', ['queen13x17', 'rsr40'])
def test_refusals(name):
    prob, keys, starts = WORKLOADS[name](2)
    n = prob.n
    eng = _engine(prob, keys, starts, bins=0)
    v, ln = np.zeros(8), ctypes.c_int64(0)
    for nm in ('hist_stats', 'hist_count', 'hist_counts'):
        with pytest.raises(ValueError, match='set hist_stats first'):
            eng.get(nm)
        assert eng._lib.occ_get_state(eng._h, 0, nm.encode(), v.ctypes.data, 8, ctypes.byref(ln)) == -5      # OCC_E_STATE
    for nm in ('hist_count', 'hist_counts'):
        with pytest.raises(ValueError, match='set hist_stats first'):
            eng.set(nm, np.zeros(1))
        assert eng._lib.occ_set_state(eng._h, 0, nm.encode(), v.ctypes.data, 1) == -5
    for bad in (3.0, 1025.0, 2.5, 64.5, -64.0, 1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='hist_stats is 0 or a number of bins from 4 to 1024'):
            eng.set('hist_stats', bad)
        w = np.array([bad])
        assert eng._lib.occ_set_state(eng._h, 0, b'hist_stats', w.ctypes.data, 1) == -1                      # OCC_E_BADARG
    with pytest.raises(ValueError, match='wrong length'):
        eng.set('hist_stats', np.full(2, 64.0))
    eng.set('hist_stats', 0.0)                                         # (off before it was ever on: accepted, nothing allocated)
    with pytest.raises(ValueError, match='set hist_stats first'):      # (nothing of the refused values was kept)
        eng.get('hist_stats')
    eng.set('hist_stats', 16.0, 1)
    assert [eng.get('hist_stats', c)[0] for c in (0, 1)] == [0.0, 16.0] and eng.get('hist_counts', 0).shape == (16 * n,)
    # another number of bins while a chain is on: refused, and the message names the handle's
    for c in (0, 1):
        with pytest.raises(ValueError, match='have 16 bins while a chain is switched on'):
            eng.set('hist_stats', 64.0, c)
        w = np.array([64.0])
        assert eng._lib.occ_set_state(eng._h, c, b'hist_stats', w.ctypes.data, 1) == -1
    # writes: only while the chain's switch is on, whole numbers in [0, 2^32)
    with pytest.raises(ValueError, match='switched off for this chain'):
        eng.set('hist_count', 3.0, 0)
    with pytest.raises(ValueError, match='switched off for this chain'):
        eng.set('hist_counts', np.zeros(16 * n), 0)
    for bad in (0.5, -1.0, 2.0 ** 32, np.nan):
        with pytest.raises(ValueError, match=r'whole numbers in \[0, 2\^32\)'):
            eng.set('hist_count', bad, 1)
        w = np.zeros(16 * n)
        w[-1] = bad
        with pytest.raises(ValueError, match=r'whole numbers in \[0, 2\^32\)'):
            eng.set('hist_counts', w, 1)
        assert eng._lib.occ_set_state(eng._h, 1, b'hist_counts', w.ctypes.data, w.size) == -1
    with pytest.raises(ValueError, match='wrong length'):
        eng.set('hist_counts', np.zeros(16 * n - 1), 1)
    assert eng.hist_counts(1)['count'] == 0 and not eng.hist_counts(1)['counts'].any()       # (nothing of a refused write was kept)
    eng.run(3, 1)
    got = _hists(eng)
    _whole(got[:1], 0)
    _whole(got[1:], 2)
    # a written histogram is read back as written, and the next call goes on from it
    w = np.arange(16 * n, dtype=np.float64) % 7
    eng.set('hist_counts', w, 1)
    eng.set('hist_count', 2.0 ** 32 - 1 - 4, 1)
    assert np.array_equal(eng.get('hist_counts', 1), w) and eng.get('hist_count', 1)[0] == 2.0 ** 32 - 5
    # the counts are 32 bits wide: a call that could take one past 2^32 - 1 is refused, one that cannot is not
    with pytest.raises(ValueError, match=r'past 2\^32 - 1'):
        eng.run(6, 1)
    with pytest.raises(ValueError, match=r'past 2\^32 - 1'):
        eng.run(5, 0)
    eng.run(5, 1)
    assert eng.get('hist_count', 1)[0] == 2.0 ** 32 - 1
    assert np.array_equal(eng.get('hist_counts', 1).reshape(16, n).sum(axis=0), w.reshape(16, n).sum(axis=0) + 4)
    with pytest.raises(ValueError, match=r'past 2\^32 - 1'):
        eng.step()
    # with every chain off another number of bins frees and reallocates: every chain starts from zero
    eng.set('hist_stats', 0.0, 1)
    eng.step()
    eng.set('hist_stats', 5.0, 0)
    assert [eng.get('hist_stats', c)[0] for c in (0, 1)] == [5.0, 0.0]
    assert [h['counts'].shape for h in _hists(eng)] == [(5, n)] * 2
    _whole(_hists(eng), 0)
    eng.run(4, 0)
    got = _hists(eng)
    _whole(got[:1], 4)
    _whole(got[1:], 0)
    eng.close()


def test_a_change_of_bins_between_runs_equals_a_fresh_engine():
    """B = 64, a run, every chain off, B = 5, a run (the captured graphs of the first were dropped: B and the address travel
    by value): the counts of the second are what an engine that ran the first without histograms holds."""
    prob, keys, starts = WORKLOADS['queen13x17'](2)
    eng = _engine(prob, keys, starts, bins=64)
    eng.run(12, 2)
    eng.hist_stats(5)                                  # (Engine.hist_stats switches every chain off first)
    eng.run(9, 1)
    got = _hists(eng)
    eng.close()
    other = _engine(prob, keys, starts, bins=0)
    other.run(12, 2)
    other.hist_stats(5)
    other.run(9, 1)
    _same(got, _hists(other))
    other.close()
    _whole(got, 8)


def test_probit_handle_refuses():
    from .test_gpu_regions import _probit_problem
    from occuspytial_amd._engine import Engine
    prob, keys, starts = _probit_problem(2)
    eng = Engine(prob, keys)
    for nm in ('hist_stats', 'hist_count', 'hist_counts'):
        with pytest.raises(ValueError, match='per-site intervals are not available for the probit model'):
            eng.get(nm)
        with pytest.raises(ValueError, match='per-site intervals are not available for the probit model'):
            eng.set(nm, 64.0)
    v = np.full(1, 64.0)
    assert eng._lib.occ_set_state(eng._h, 0, b'hist_stats', v.ctypes.data, 1) == -5                        # OCC_E_STATE
    eng.close()


def test_checkpoint_and_restore_mid_run_equal_the_uninterrupted_run():
    prob, keys, starts = _workload_a(2)
    e1 = _engine(prob, keys, starts)
    e1.run(20, 5)
    ck = e1.checkpoint()
    assert ck['hist_stats'].tolist() == [64.0, 64.0] and ck['hist_count'].tolist() == [15, 15]
    assert ck['hist_counts'].dtype == np.uint32 and ck['hist_counts'].shape == (2, 64, prob.n)
    e1.close()
    e2 = _engine(prob, keys, starts, bins=0)             # a fresh engine that never heard of the histograms
    assert not [k for k in e2.checkpoint() if k.startswith('hist_')]
    e2.restore(ck)
    assert e2._hist_bins == 64 and [h['count'] for h in _hists(e2)] == [15, 15]
    e2.run(15, 0)
    got = _hists(e2)
    e2.restore({k: v for k, v in ck.items() if not k.startswith('hist_')})      # (a checkpoint without them: the switch goes off)
    assert e2._hist_bins == 0 and e2.get('hist_stats', 0)[0] == 0.0
    e2.close()
    _same(got, _two_calls(prob, keys, starts, split=((20, 5), (15, 0))))


def _sampler(cls_name='LogitICARGibbs', **kw):
    import occuspytial_amd
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(30, 40, visits=3, p=2, q=2, random_state=2)
    return getattr(occuspytial_amd, cls_name)(Q, W, X, y, random_state=7, **kw)


@pytest.mark.parametrize('cls_name, kw', [('LogitICARGibbs', {}), ('LogitRSRGibbs', dict(q=40))])
def test_sampler_returns_the_intervals_of_the_kept_draws(cls_name, kw):
    from occuspytial_amd.intervals import SiteIntervals
    s = _sampler(cls_name, **kw)
    chunked = s.sample(60, burnin=20, chains=3, progressbar=True, site_intervals=True)   # chunks of 16: one straddles the burn-in
    one = _sampler(cls_name, **kw).sample(60, burnin=20, chains=3, progressbar=False, site_intervals=True)
    plain = _sampler(cls_name, **kw).sample(60, burnin=20, chains=3, progressbar=False)
    assert plain.site_intervals is None and isinstance(one.site_intervals, SiteIntervals)
    assert sorted(one.data) == sorted(plain.data)                              # (post.summary and the chains are unchanged)
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(one[name], plain[name]) and np.array_equal(chunked[name], plain[name])
    si = one.site_intervals
    assert si.bins == 64 and si.n_sites == 1200 and si.n_draws.tolist() == [40, 40, 40]
    assert np.all(si.per_chain_counts.sum(axis=1) == 40)
    assert np.array_equal(si.per_chain_counts, chunked.site_intervals.per_chain_counts)
    lo, hi = si.interval()
    assert np.all((0 <= lo) & (lo <= si.median) & (si.median <= hi) & (hi <= 1)) and 'bins=64' in repr(si)
    # resume: the histograms go on from the checkpoint's, and end as those of an uninterrupted run
    ck = s.checkpoint()
    assert ck['hist_stats'].tolist() == [64.0] * 3 and ck['hist_counts'].dtype == np.uint32
    more = s.resume(ck, 30, progressbar=False, site_intervals=True)
    longer = _sampler(cls_name, **kw).sample(90, burnin=20, chains=3, progressbar=False, site_intervals=True)
    assert more.site_intervals.n_draws.tolist() == [70] * 3
    assert np.array_equal(more.site_intervals.per_chain_counts, longer.site_intervals.per_chain_counts)
    assert np.array_equal(more['alpha'], longer['alpha'][:, 40:])
    other = s.resume(ck, 30, progressbar=False, site_intervals=16)             # (another number of bins: from zero)
    assert other.site_intervals.bins == 16 and other.site_intervals.n_draws.tolist() == [30] * 3
    again = s.resume(ck, 5, progressbar=False)                                 # (not asked for: the checkpoint's switch goes off)
    assert again.site_intervals is None and not s._engine._hist_bins
