"""Per-site convergence diagnostics, accumulated on the device (state names ``conv_stats``, ``conv_count``, ``conv_sums``;
csrc/occ_conv.hpp).

Per iteration past a call's burn-in one kernel behind the z update updates, per site of a chain whose switch is on, eleven
float64 slots: the site's count, then for psi = expit(x beta + eta) and for eta the first counted value ``ref``, the sums
``s1`` and ``s2`` of d = v - ref and d d, the sum ``run`` over the unfinished batch and the sum ``bsq`` of the squared sums of
the finished batches of L iterations.  A column belongs to one thread and additions run in iteration order, so every
comparison between two ways of running the engine is equality of bits.  The comparison with numpy has bounds from the number
formats: eta is read back as the kernel read it, so its sums differ from numpy's by the compiler's freedom to contract
d d + s2 alone (4 N 2^-53 relative covers one rounding per addition); psi is held to the project's 1e-12
(tests/test_gpu_site_summaries.py), so with |d| < 1 its s1 and run are within N 2e-12 and its s2 and bsq within N L 4e-12.
Workloads: those of tests/test_gpu_intervals.py.  Every test runs under its own time limit.
"""
import ctypes

import numpy as np
import pytest

from ._outputs_gpu import engine_with, time_limit as _time_limit, two_calls  # noqa: F401 (autouse in this module)
from .test_gpu_intervals import WORKLOADS, _psi, _sampler
from .test_gpu_parity import KEY, _problem_from_golden, _random_start
from .test_gpu_ppc import SCHED_KEYS
from .test_gpu_site_summaries import _rsr_problem, _workload_a

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
CNT, PSI, ETA = 0, 1, 6
REF, S1, S2, RUN, BSQ = range(5)


# ------------------------------------------------------------------ helpers
def _engine(prob, keys, starts, L=5, **kw):
    return engine_with(prob, keys, starts, conv=L, **kw)


def _sums(eng):
    return [eng.conv_sums(c) for c in range(eng.n_chains)]


def _two_calls(prob, keys, starts, split=((33, 4), (10, 0)), **kw):
    """run(33, 4) then run(10, 0) -> per chain the sums of the 39 iterations past the calls' burn-in."""
    return two_calls(lambda: _engine(prob, keys, starts, **kw), _sums, split)


def _same(a, b):
    assert len(a) == len(b)
    for c, (u, v) in enumerate(zip(a, b)):
        assert u['batch'] == v['batch'] and u['count'] == v['count'], (c, u['count'], v['count'])
        assert u['sums'].dtype == np.float64 and u['sums'].shape == v['sums'].shape and u['sums'].shape[0] == 11
        assert np.array_equal(u['sums'], v['sums']), (c, np.count_nonzero(u['sums'] != v['sums']))


def _whole(sums, count, L=5):
    """Every chain counted `count` iterations, so did every site, and the unfinished batch is empty exactly when L divides it."""
    for s in sums:
        assert s['count'] == count and np.all(s['sums'][CNT] == count) and s['batch'] == L
        assert np.all(np.isfinite(s['sums']))
        if count and count % L == 0:
            assert not s['sums'][PSI + RUN].any() and not s['sums'][ETA + RUN].any()


def _restate(slots, v, first, closes):
    """The update rule of DESIGN 21 on one quantity's five slots (5, n), in place, operation by operation."""
    if first:
        slots[REF] = v
    d = v - slots[REF]
    slots[S1] += d
    slots[S2] += d * d
    slots[RUN] += d
    if closes:
        slots[BSQ] += slots[RUN] * slots[RUN]
        slots[RUN] = 0.0


# ------------------------------------------------------------------ 1: restatement
CASES = [('queen13x17', chains, L) for chains in (1, 2, 4) for L in (1, 4, 5)] + \
        [('queen30x40', 2, 4), ('weighted300', 1, 5), ('generic', 1, 4), ('rsr40', 2, 5)]


@pytest.mark.parametrize('name, chains, L', CASES)
def test_sums_equal_their_restatement_in_numpy(name, chains, L):
    """Thirteen iterations as thirteen run(1, 0) calls.  After each, beta and eta of every chain are read back, the update
    rule is restated in numpy and every slot is compared under the bounds of the module's docstring.  L = 4 and 5 leave
    three complete batches and one value in `run`, two and three; the same thirteen iterations as one run(13, 0) give equal
    bits."""
    prob, keys, starts = WORKLOADS[name](chains)
    n, C = prob.n, len(keys)
    eng = _engine(prob, keys, starts, L=L)
    assert [eng.get('conv_stats', c)[0] for c in range(C)] == [float(L)] * C
    want = np.zeros((C, 11, n))
    worst = {}
    for t in range(13):
        eng.run(1, 0)
        N = t + 1
        for c in range(C):
            eta = eng.get('eta', c)
            psi = _psi(prob, eng, c)
            _restate(want[c, PSI:PSI + 5], psi, t == 0, N % L == 0)
            _restate(want[c, ETA:ETA + 5], eta, t == 0, N % L == 0)
            want[c, CNT] = N
            got = eng.conv_sums(c)
            assert got['count'] == N and got['batch'] == L and got['sums'].shape == (11, n)
            g = got['sums']
            assert np.array_equal(g[CNT], want[c, CNT])
            assert np.array_equal(g[ETA + REF], want[c, ETA + REF])
            for k, nm in ((S1, 's1'), (S2, 's2'), (RUN, 'run'), (BSQ, 'bsq')):
                err = np.abs(g[ETA + k] - want[c, ETA + k])
                bound = 4 * N * EPS * np.abs(want[c, ETA + k])
                worst['eta ' + nm] = max(worst.get('eta ' + nm, 0.0), float(np.max(err / np.maximum(np.abs(want[c, ETA + k]), 1e-300))))
                assert np.all(err <= bound), (name, c, t, nm, float(err.max()))
            for k, nm, bound in ((REF, 'ref', 1e-12), (S1, 's1', N * 2e-12), (RUN, 'run', N * 2e-12), (S2, 's2', N * L * 4e-12),
                                 (BSQ, 'bsq', N * L * 4e-12)):
                err = float(np.abs(g[PSI + k] - want[c, PSI + k]).max())
                worst['psi ' + nm] = max(worst.get('psi ' + nm, 0.0), err)
                assert err <= bound, (name, c, t, nm, err, bound)
    print(name, chains, L, 'largest deviations (eta relative, psi absolute):', worst)
    stepped = _sums(eng)
    eng.close()
    _whole(stepped, 13, L)
    for s in stepped:
        assert np.all(s['sums'][ETA + S2] > 0) and np.all(s['sums'][ETA + BSQ] > 0)          # (eta moves at every site)
        if L > 1:
            assert s['sums'][ETA + RUN].all()                                                   # (13 = 3 L + 1 and 2 L + 3: a non-empty run)
    one = _engine(prob, keys, starts, L=L)
    one.run(13, 0)
    _same(_sums(one), stepped)
    one.close()


# ------------------------------------------------------------------ 2: host-held draws
def _direct(draws, L):
    """R-hat, ESS, MCSE, mean and W of draws (chains, N, sites) by their textbook formulas."""
    C, N, n = draws.shape
    a = N // L
    means = draws.mean(axis=1)
    W = draws.var(axis=1, ddof=1).mean(axis=0)
    bm = draws[:, :a * L].reshape(C, a, L, n).mean(axis=2)
    sigma2 = (L * bm.var(axis=1, ddof=1)).mean(axis=0)
    with np.errstate(divide='ignore', invalid='ignore'):
        rhat = np.sqrt(((N - 1) / N * W + means.var(axis=0, ddof=1)) / W) if C > 1 else np.full(n, np.nan)
        return {'mean': means.mean(axis=0), 'var': W, 'ess': C * N * W / sigma2, 'mcse': np.sqrt(sigma2 / (C * N)), 'rhat': rhat}


def test_diagnostics_equal_those_of_draws_held_on_the_host():
    """240 iterations on the 13x17 lattice, two chains, L = 15, psi and eta of every one kept on the host.  SiteDiagnostics
    from the device's sums equals the same formulas applied to the held draws -- the per-chain batch means computed directly,
    R-hat from the per-chain mean and variance -- to 1e-9 relative at every site with W > 0."""
    from occuspytial_amd.convergence import SiteDiagnostics
    prob, keys, starts = WORKLOADS['queen13x17'](2)
    L = 15
    eng = _engine(prob, keys, starts, L=L)
    held = {'psi': [], 'eta': []}
    for _ in range(240):
        eng.run(1, 0)
        held['psi'].append([_psi(prob, eng, c) for c in range(2)])
        held['eta'].append([eng.get('eta', c) for c in range(2)])
    sd = SiteDiagnostics.from_engine(eng)
    eng.close()
    assert sd.n_draws.tolist() == [240, 240] and sd.batch == L and sd.n_batches.tolist() == [16, 16] and sd.n_sites == prob.n
    for q in ('psi', 'eta'):
        want = _direct(np.stack(held[q]).transpose(1, 0, 2), L)
        moved = want['var'] > 0
        assert moved.all()
        for what in ('mean', 'var', 'ess', 'mcse', 'rhat'):
            got = getattr(sd, what)(q)
            rel = np.abs(got - want[what])[moved] / np.abs(want[what][moved])
            print(q, what, 'largest relative deviation %.3g' % rel.max())
            assert rel.max() <= 1e-9, (q, what, float(rel.max()))
        assert np.all(sd.ess(q) > 1) and np.all(sd.rhat(q) > 0.9)
        assert sd.worst(q, 5).tolist() == np.argsort(-want['rhat'], kind='stable')[:5].tolist()


# ------------------------------------------------------------------ 3: bit-equal sums whatever the path
@pytest.fixture(scope='module')
def ref_a():
    """Workload A, two chains, L = 5, run(33, 4) then run(10, 0), on the default path: computed once, never changed.  29
    iterations of the first call: its end falls inside a batch."""
    prob, keys, starts = _workload_a(2)
    ref = _two_calls(prob, keys, starts)
    _whole(ref, 39)
    for s in ref:
        s['sums'].setflags(write=False)
        assert s['sums'][ETA + RUN].all()
    return ref


def test_differently_split_calls_give_the_same_sums(ref_a):
    prob, keys, starts = _workload_a(2)
    _same(ref_a, _two_calls(prob, keys, starts, split=((5, 4), (28, 0), (3, 0), (7, 0))))     # (boundaries inside batches)
    _same(ref_a, _two_calls(prob, keys, starts, split=((5, 4), (1, 0), (37, 0))))            # (a call of one iteration)
    _same(ref_a, _two_calls(prob, keys, starts, split=((9, 4), (34, 0))))                    # (a boundary between batches)


def test_occ_step_counts():
    """occ_step's window has burn-in 0: eager steps count like the iterations of a replayed graph, also between two runs."""
    prob, keys, starts = _workload_a(2)
    eng = _engine(prob, keys, starts)
    eng.run(4, 4 - 1)                 # (the three iterations of burn-in are not counted, the fourth is)
    for _ in range(9):
        eng.step()
    eng.run(29, 0)
    got = _sums(eng)
    eng.close()
    _whole(got, 39)
    _same(got, _two_calls(prob, keys, starts, split=((4, 3), (38, 0))))


@pytest.mark.parametrize('env', [{'OCC_EVENT_SYNC': '1'}, {'OCC_EVENT_SYNC': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_CU_SPLIT': '0'},
                                 {'OCC_DEBUG_STREAMS_SERIALISED': '1'},
                                 {'OCC_NO_SIDE_STREAM': '1'}, {'OCC_EAGER_ONLY': '1'}, {'OCC_NO_XCD_LOCAL': '1'},
                                 {'OCC_NO_XCD_LOCAL': '1', 'OCC_CU_SPLIT': '0'},
                                 {'OCC_NO_PERSISTENT': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_NO_PERSISTENT': '1', 'OCC_NO_SIDE_STREAM': '1'}])
def test_every_scheduling_mode_gives_the_same_sums(monkeypatch, env):
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


def test_tile_looping_kernel_gives_the_sums_of_launch_per_step(monkeypatch):
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
        out[mode] = _sums(eng)
        assert eng.stats()['fused_fallbacks'] == 0
        eng.close()
    _whole(out['tiles'], 21)
    _same(out['tiles'], out['launch_per_step'])


def test_batched_chains_have_the_sums_of_single_chain_runs():
    prob, _ = _problem_from_golden('ref_graph300_weighted')
    keys = [KEY, KEY ^ 0xABCDEF, 12345]
    rng = np.random.default_rng(3)
    starts = [dict(alpha=rng.standard_normal(prob.q), beta=rng.standard_normal(prob.p), tau=1.0 + c,
                   eta=(lambda e: e - e.mean())(rng.standard_normal(prob.n))) for c in range(3)]
    batch = _engine(prob, keys, starts)
    batch.run(20, 4)
    both = _sums(batch)
    batch.close()
    _whole(both, 16)
    for c in range(3):
        solo = _engine(prob, [keys[c]], [starts[c]])
        solo.run(20, 4)
        _same([both[c]], _sums(solo))
        solo.close()


def test_engine_group_switches_everywhere_and_routes_by_chain():
    from occuspytial_amd._engine import Engine, EngineGroup
    prob, keys, starts = _workload_a(3)
    grp = EngineGroup(prob, keys, [0, 0], engine_factory=lambda pr, ks, dev: Engine(pr, ks, device=dev))
    for c in range(3):
        grp.set_start(c, **starts[c])
    assert grp._conv_batch == 0
    grp.conv_stats(5)
    assert grp._conv_batch == 5
    grp.run(20, 5)
    ck = grp.checkpoint()
    assert ck['conv_stats'].tolist() == [5.0] * 3 and ck['conv_count'].tolist() == [15] * 3
    assert ck['conv_sums'].shape == (3, 11, prob.n) and ck['conv_sums'].dtype == np.float64
    grp.restore(ck)
    grp.run(10, 0)
    got = [grp.conv_sums(c) for c in range(3)]
    grp.close()
    _same(_two_calls(prob, keys, starts, split=((20, 5), (10, 0))), got)


# ------------------------------------------------------------------ 4: beside the other outputs
def test_counts_agree_beside_every_other_output():
    """The four outputs of the z update, moran_stats and hist_stats on: the histograms and the sums count the same
    iterations, every site's own count is the chain's, and the sums are those of an engine with nothing else on."""
    prob, keys, starts = _workload_a(2)
    ids = (np.arange(prob.n) % 7).astype(np.int64)
    eng = _engine(prob, keys, starts, bins=64, site=True, ll=True, ids=ids, ppc=True, moran=True)
    eng.run(12, 3)
    eng.run(5, 0)
    got = _sums(eng)
    for c in range(2):
        assert eng.hist_counts(c)['count'] == got[c]['count'] == eng.site_sums(c)['count'] == 14
        assert np.all(got[c]['sums'][CNT] == got[c]['count'])
    eng.close()
    _whole(got, 14)
    _same(got, _two_calls(prob, keys, starts, split=((12, 3), (5, 0))))


# ------------------------------------------------------------------ 5: a re-run call counts nothing twice
def _headline_sums(iters=10):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(100, 100, visits=5, p=2, q=2, random_state=0)
    prob = FlatProblem(Q, W, X, y)
    eng = _engine(prob, [KEY + 5 * c for c in range(4)], [_random_start(prob, 60 + c) for c in range(4)], L=4)
    eng.run(iters, 0)
    eng.run(7, 2)
    out = _sums(eng), eng.stats()
    eng.close()
    return out


def _rsr_sums():
    prob, keys, starts = _rsr_problem(40)
    eng = _engine(prob, keys, starts, L=4)
    eng.run(8, 0)
    eng.run(5, 1)
    out = _sums(eng), eng.stats()
    eng.close()
    return out


@pytest.fixture(scope='module')
def ref_headline():
    ref, st = _headline_sums()
    assert st['fused_fallbacks'] == 0
    _whole(ref, 15, 4)
    return ref


def test_a_call_rerun_after_a_barrier_timeout_counts_no_iteration_twice(monkeypatch, ref_headline):
    """The knobs of tests/test_gpu_intervals.py's test of the same name, with the sums on: a bounded wait gives up, the call is
    re-run from the snapshot, which holds the sums."""
    monkeypatch.setenv('OCC_CU_SPLIT', '32')
    monkeypatch.setenv('OCC_DEBUG_SKIP_RESIDENCY_PROBE', '1')
    monkeypatch.setenv('OCC_QUIET', '1')
    alt, st = _headline_sums()
    assert st['fused_fallbacks'] == 1
    _whole(alt, 15, 4)
    _same(ref_headline, alt)


def test_a_call_rerun_after_a_broken_handover_counts_no_iteration_twice(monkeypatch, ref_headline):
    """Likewise with the broken hand-over: fused ICAR path and reduced-rank model."""
    monkeypatch.setenv('OCC_QUIET', '1')
    rsr_ref, _ = _rsr_sums()
    monkeypatch.setenv('OCC_DEBUG_BREAK_HANDOVER', '1')
    alt, st = _headline_sums()
    assert st['fused_fallbacks'] == 1
    _whole(alt, 15, 4)
    _same(ref_headline, alt)
    rsr_alt, rst = _rsr_sums()
    assert rst['fused_fallbacks'] == 1
    _whole(rsr_alt, 12, 4)
    _same(rsr_ref, rsr_alt)


# ------------------------------------------------------------------ 6: nothing else sees the switch
@pytest.mark.parametrize('name', ['queen30x40', 'generic', 'rsr40'])
def test_nothing_else_sees_the_switch(name):
    """alpha, beta, tau, eta, z, the site_* and ll_* sums, region_draws, ppc_draws, moran_draws and hist_counts are the same
    bits with conv_stats on and off."""
    prob, keys, starts = WORKLOADS[name](2)
    ids = (np.arange(prob.n) % 7).astype(np.int64)
    engines = {}
    for which in ('on', 'off'):
        eng = engines[which] = _engine(prob, keys, starts, L=5 if which == 'on' else 0, bins=64, site=True, ll=True, ids=ids, ppc=True,
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
        a, b = on.hist_counts(c), off.hist_counts(c)
        assert a['count'] == b['count'] == 39 and np.array_equal(a['counts'], b['counts'])
    _whole(_sums(on), 39)
    with pytest.raises(ValueError, match='set conv_stats first'):       # (the other handle never heard of them)
        off.get('conv_count')
    for eng in engines.values():
        eng.close()


def test_windows_and_a_chain_that_does_not_count():
    """120 iterations, 100 past the burn-in, four chains of which the last has its switch off; switching a chain on again
    zeroes its part alone; off keeps everything readable."""
    prob, keys, starts = _workload_a(4)
    eng = _engine(prob, keys, starts)
    eng.set('conv_stats', 0.0, 3)
    eng.run(120, 20)
    got = _sums(eng)
    _whole(got[:3], 100)
    assert got[3]['count'] == 0 and not got[3]['sums'].any()
    assert [eng.get('conv_stats', c)[0] for c in range(4)] == [5.0, 5.0, 5.0, 0.0]
    eng.set('conv_stats', 5.0, 1)                     # on again: zeroes chain 1 alone
    after = _sums(eng)
    assert after[1]['count'] == 0 and not after[1]['sums'].any()
    _same([got[0], got[2]], [after[0], after[2]])
    eng.set('conv_stats', 0.0, 0)                     # off: stays readable, stops counting
    eng.set_start(1, **starts[1])                     # occ_set_start and occ_set_keys do not touch the switch
    eng.set_keys(keys)
    eng.run(6, 1)
    last = _sums(eng)
    _same([got[0]], [last[0]])
    _whole(last[1:2], 5)
    _whole(last[2:3], 105)
    eng.close()


# ------------------------------------------------------------------ 7: the interface
@pytest.mark.parametrize('name', ['queen13x17', 'rsr40'])
def test_refusals(name):
    prob, keys, starts = WORKLOADS[name](2)
    n = prob.n
    eng = _engine(prob, keys, starts, L=0)
    v, ln = np.zeros(8), ctypes.c_int64(0)
    for nm in ('conv_stats', 'conv_count', 'conv_sums'):
        with pytest.raises(ValueError, match='set conv_stats first'):
            eng.get(nm)
        assert eng._lib.occ_get_state(eng._h, 0, nm.encode(), v.ctypes.data, 8, ctypes.byref(ln)) == -5      # OCC_E_STATE
    for nm in ('conv_count', 'conv_sums'):
        with pytest.raises(ValueError, match='set conv_stats first'):
            eng.set(nm, np.zeros(1))
        assert eng._lib.occ_set_state(eng._h, 0, nm.encode(), v.ctypes.data, 1) == -5
    for bad in (0.5, -1.0, 2.0 ** 30 + 1, 2.5, np.nan, np.inf):
        with pytest.raises(ValueError, match=r'conv_stats is 0 or a batch length from 1 to 2\^30'):
            eng.set('conv_stats', bad)
        w = np.array([bad])
        assert eng._lib.occ_set_state(eng._h, 0, b'conv_stats', w.ctypes.data, 1) == -1                      # OCC_E_BADARG
    with pytest.raises(ValueError, match='wrong length'):
        eng.set('conv_stats', np.full(2, 5.0))
    eng.set('conv_stats', 0.0)                                         # (off before it was ever on: accepted, nothing allocated)
    with pytest.raises(ValueError, match='set conv_stats first'):      # (nothing of the refused values was kept)
        eng.get('conv_stats')
    eng.set('conv_stats', 2.0 ** 30, 1)                                # (the largest batch length)
    eng.set('conv_stats', 0.0, 1)
    eng.set('conv_stats', 4.0, 1)                                      # (every chain was off: another L is accepted)
    assert [eng.get('conv_stats', c)[0] for c in (0, 1)] == [0.0, 4.0] and eng.get('conv_sums', 0).shape == (11 * n,)
    # another batch length while a chain is on: refused, and the message names the handle's
    for c in (0, 1):
        with pytest.raises(ValueError, match='have batch length 4 while a chain is switched on'):
            eng.set('conv_stats', 5.0, c)
        w = np.array([5.0])
        assert eng._lib.occ_set_state(eng._h, c, b'conv_stats', w.ctypes.data, 1) == -1
    # writes: only while the chain's switch is on; cnt and count whole numbers >= 0, every cnt equal
    with pytest.raises(ValueError, match='switched off for this chain'):
        eng.set('conv_count', 3.0, 0)
    with pytest.raises(ValueError, match='switched off for this chain'):
        eng.set('conv_sums', np.zeros(11 * n), 0)
    for bad in (0.5, -1.0, np.nan):
        with pytest.raises(ValueError, match='conv_count is a whole number >= 0'):
            eng.set('conv_count', bad, 1)
        w = np.zeros(11 * n)
        w[:n] = bad                                                    # (fractional, negative)
        with pytest.raises(ValueError, match='cnt slot of conv_sums holds one whole number >= 0 at every site'):
            eng.set('conv_sums', w, 1)
        assert eng._lib.occ_set_state(eng._h, 1, b'conv_sums', w.ctypes.data, w.size) == -1
    w = np.zeros(11 * n)
    w[:n] = 3.0
    w[n - 1] = 4.0                                                     # (unequal)
    with pytest.raises(ValueError, match='cnt slot of conv_sums holds one whole number >= 0 at every site'):
        eng.set('conv_sums', w, 1)
    with pytest.raises(ValueError, match='wrong length'):
        eng.set('conv_sums', np.zeros(11 * n - 1), 1)
    assert eng.conv_sums(1)['count'] == 0 and not eng.conv_sums(1)['sums'].any()       # (nothing of a refused write was kept)
    eng.run(3, 1)
    got = _sums(eng)
    assert got[0]['count'] == 0 and not got[0]['sums'].any()
    _whole(got[1:], 2, 4)
    # written sums are read back as written, and the next call goes on from them: cnt = 2 and L = 4, so the second of the
    # four iterations closes a batch
    w = np.arange(11 * n, dtype=np.float64) % 7 - 3.0
    w[:n] = 2.0
    eng.set('conv_sums', w, 1)
    eng.set('conv_count', 2.0, 1)
    assert np.array_equal(eng.get('conv_sums', 1), w) and eng.get('conv_count', 1)[0] == 2.0
    eng.run(4, 0)
    got = eng.conv_sums(1)
    assert got['count'] == 6 and np.all(got['sums'][CNT] == 6)
    assert np.array_equal(got['sums'][ETA + REF], w.reshape(11, n)[ETA + REF])         # (ref is taken at cnt = 0 alone)
    assert np.all(got['sums'][ETA + BSQ] >= w.reshape(11, n)[ETA + BSQ])
    assert np.all(got['sums'][ETA + S2] >= w.reshape(11, n)[ETA + S2])
    eng.close()


def test_a_change_of_batch_length_between_runs_equals_a_fresh_engine():
    """L = 5, a run, every chain off, L = 3, a run (the captured graphs of the first were dropped: L travels by value): the sums
    of the second are what an engine that ran the first without them holds."""
    prob, keys, starts = WORKLOADS['queen13x17'](2)
    eng = _engine(prob, keys, starts, L=5)
    eng.run(12, 2)
    eng.conv_stats(3)                                  # (Engine.conv_stats switches every chain off first)
    eng.run(9, 1)
    got = _sums(eng)
    eng.close()
    other = _engine(prob, keys, starts, L=0)
    other.run(12, 2)
    other.conv_stats(3)
    other.run(9, 1)
    _same(got, _sums(other))
    other.close()
    _whole(got, 8, 3)


def test_probit_handle_refuses():
    from .test_gpu_regions import _probit_problem
    from occuspytial_amd._engine import Engine
    prob, keys, starts = _probit_problem(2)
    eng = Engine(prob, keys)
    for nm in ('conv_stats', 'conv_count', 'conv_sums'):
        with pytest.raises(ValueError, match='per-site convergence diagnostics are not available for the probit model'):
            eng.get(nm)
        with pytest.raises(ValueError, match='per-site convergence diagnostics are not available for the probit model'):
            eng.set(nm, 5.0)
    v = np.full(1, 5.0)
    assert eng._lib.occ_set_state(eng._h, 0, b'conv_stats', v.ctypes.data, 1) == -5                        # OCC_E_STATE
    eng.close()


def test_checkpoint_and_restore_mid_run_equal_the_uninterrupted_run():
    prob, keys, starts = _workload_a(2)
    e1 = _engine(prob, keys, starts)
    e1.run(22, 5)                                        # (17 iterations: the checkpoint falls inside a batch)
    ck = e1.checkpoint()
    assert ck['conv_stats'].tolist() == [5.0, 5.0] and ck['conv_count'].tolist() == [17, 17]
    assert ck['conv_sums'].dtype == np.float64 and ck['conv_sums'].shape == (2, 11, prob.n)
    held = _sums(e1)
    e1.close()
    e2 = _engine(prob, keys, starts, L=0)                # a fresh engine that never heard of the sums
    assert not [k for k in e2.checkpoint() if k.startswith('conv_')]
    e2.restore(ck)
    assert e2._conv_batch == 5
    _same(held, _sums(e2))                               # bit-exact
    e2.run(15, 0)
    got = _sums(e2)
    e2.restore({k: v for k, v in ck.items() if not k.startswith('conv_')})      # (a checkpoint without them: the switch goes off)
    assert e2._conv_batch == 0 and e2.get('conv_stats', 0)[0] == 0.0
    e2.close()
    _same(got, _two_calls(prob, keys, starts, split=((22, 5), (15, 0))))


@pytest.mark.parametrize('cls_name, kw', [('LogitICARGibbs', {}), ('LogitRSRGibbs', dict(q=40))])
def test_sampler_returns_the_diagnostics_of_the_kept_draws(cls_name, kw):
    from occuspytial_amd.convergence import SiteDiagnostics
    s = _sampler(cls_name, **kw)
    chunked = s.sample(60, burnin=20, chains=3, progressbar=True, site_diagnostics=True)   # chunks of 16: one straddles the burn-in
    one = _sampler(cls_name, **kw).sample(60, burnin=20, chains=3, progressbar=False, site_diagnostics=True)
    plain = _sampler(cls_name, **kw).sample(60, burnin=20, chains=3, progressbar=False)
    assert plain.site_diagnostics is None and isinstance(one.site_diagnostics, SiteDiagnostics)
    assert sorted(one.data) == sorted(plain.data)                              # (post.summary and the chains are unchanged)
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(one[name], plain[name]) and np.array_equal(chunked[name], plain[name])
    sd = one.site_diagnostics
    assert sd.batch == 6 and sd.n_sites == 1200 and sd.n_draws.tolist() == [40, 40, 40] and sd.n_batches.tolist() == [6, 6, 6]
    assert np.array_equal(sd.per_chain_sums, chunked.site_diagnostics.per_chain_sums)
    for q in ('psi', 'eta'):
        assert np.all(sd.rhat(q) > 0.9) and np.all(sd.ess(q) > 0) and np.all(sd.mcse(q) > 0) and sd.worst(q, 7).shape == (7,)
    assert np.all((0 < sd.mean('psi')) & (sd.mean('psi') < 1)) and 'batch=6' in repr(sd)
    # resume: the sums go on from the checkpoint's with the checkpoint's L, and end as those of an uninterrupted run with it
    ck = s.checkpoint()
    assert ck['conv_stats'].tolist() == [6.0] * 3 and ck['conv_sums'].shape == (3, 11, 1200)
    more = s.resume(ck, 30, progressbar=False, site_diagnostics=True)
    longer = _sampler(cls_name, **kw).sample(90, burnin=20, chains=3, progressbar=False, site_diagnostics=6)
    assert more.site_diagnostics.n_draws.tolist() == [70] * 3 and more.site_diagnostics.batch == 6
    assert np.array_equal(more.site_diagnostics.per_chain_sums, longer.site_diagnostics.per_chain_sums)
    assert np.array_equal(more['alpha'], longer['alpha'][:, 40:])
    other = s.resume(ck, 30, progressbar=False, site_diagnostics=10)           # (another L: the checkpoint's is kept)
    assert other.site_diagnostics.batch == 6 and np.array_equal(other.site_diagnostics.per_chain_sums, more.site_diagnostics.per_chain_sums)
    again = s.resume(ck, 5, progressbar=False)                                 # (not asked for: the checkpoint's switch goes off)
    assert again.site_diagnostics is None and not s._engine._conv_batch
