"""Posterior predictive check of the detection histories, formed on the device (state names ``ppc_stats``, ``ppc_draws``).

Per kept draw the z update replicates every surveyed site's detections from the draw's (z, alpha) and adds four integer sums:
the Freeman-Tukey discrepancy of the observed and of the replicated detections in 2^-32 fixed point, the replicated detections
and the replicated sites with a detection.  Integer sums do not depend on the order of addition, so every comparison between
two ways of running the engine is equality; the comparison with numpy (``_columns``) is equality for the two counts and, for
the two discrepancies, within one quantum per surveyed site with z = 1.  Workloads: A, the 30x40 lattice; the wide-row graph
and the ragged queen fixtures; G, 17x19 with nine covariates of each kind (the generic kernels); the reduced-rank model on
both solve paths.  Every test runs under its own time limit (``_time_limit``).
"""

import numpy as np
import pytest
from scipy.special import expit

from ._outputs_gpu import engine_with, time_limit as _time_limit, two_calls  # noqa: F401 (autouse in this module)
from .test_gpu_parity import KEY, _problem_from_golden, _random_start
from .test_gpu_site_summaries import _rsr_problem, _workload_a, _workload_g

pytestmark = pytest.mark.gpu
STREAM_PPC = 13


# ------------------------------------------------------------------ helpers
def _engine(prob, keys, starts, on=True, **kw):
    return engine_with(prob, keys, starts, ppc=on, **kw)


def _rows(eng):
    return [eng.ppc_draws(c) for c in range(eng.n_chains)]


def _two_calls(prob, keys, starts, split=((33, 4), (10, 0)), **kw):
    """run(33, 4) then run(10, 0) -> per chain the 39 recorded rows, (39, 4)."""
    return two_calls(lambda: _engine(prob, keys, starts, **kw), _rows, split, per_call=True)


def _same(a, b):
    assert len(a) == len(b)
    for c, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.shape[1] == 4 and np.array_equal(u, v), (c, u.shape, v.shape)


def _columns(prob, alpha, z, u):
    """The four columns of one draw from their definitions, in numpy -> (T_obs quanta, T_rep quanta, detections, sites,
    surveyed sites with z = 1, the smallest |u_r - d_r|).  The quanta are Python integers."""
    S = prob.S
    row_site = np.repeat(np.arange(S), np.diff(prob.site_ptr))
    d = expit(prob.W @ np.asarray(alpha))
    zi = (np.asarray(z)[prob.site_id] != 0).astype(np.float64)
    y_i = np.bincount(row_site, weights=prob.y, minlength=S)
    E = zi * np.bincount(row_site, weights=d, minlength=S)        # (np.bincount adds in row order)
    y_rep = zi * np.bincount(row_site, weights=(u < d).astype(np.float64), minlength=S)
    assert not np.any(y_i[zi == 0])                                # (a site with z = 0 has had no detection)
    a = (np.sqrt(y_i) - np.sqrt(E)) ** 2
    b = (np.sqrt(y_rep) - np.sqrt(E)) ** 2
    fx = lambda x: int(np.rint(x * 2.0 ** 32).astype(np.uint64).sum(dtype=np.uint64))
    return fx(a), fx(b), int(y_rep.sum()), int(np.count_nonzero(y_rep)), int(zi.sum()), float(np.abs(u - d).min())


# ------------------------------------------------------------------ 1: restatement
WORKLOADS = {
    'lattice': lambda chains: _workload_a(chains),
    'wide_rows': lambda chains: (lambda pr: (pr[0], [KEY], [pr[1]]))(_problem_from_golden('ref_graph300_weighted')),
    'ragged': lambda chains: (lambda pr: (pr[0], [KEY], [pr[1]]))(_problem_from_golden('ref_queen150_ragged')),
    'generic': lambda chains: _workload_g(),
    'rsr40': lambda chains: _rsr_problem(40),
    'rsr160': lambda chains: _rsr_problem(160),
}
CASES = [('lattice', 1), ('lattice', 2), ('lattice', 4), ('wide_rows', 1), ('ragged', 1), ('generic', 1), ('rsr40', 2), ('rsr160', 2)]


@pytest.mark.parametrize('name, chains', CASES)
def test_rows_equal_their_restatement_in_numpy(name, chains):
    """Twelve iterations as twelve run(1, 0) calls.  After each: alpha, the new z and the iteration the z update used are read
    back, u is re-drawn with occ_draw(uniform, key, it, 13, R), and the four columns are formed in numpy.  Columns 2 and 3 are
    equal (no row has |u - d| < 1e-12, asserted, so none could flip); columns 0 and 1 agree within one quantum per surveyed
    site with z = 1.  The same twelve iterations as one run(12, 0) give equal rows."""
    from occuspytial_amd._engine import device_draw
    prob, keys, starts = WORKLOADS[name](chains)
    eng = _engine(prob, keys, starts)
    assert eng.get('ppc_stats')[0] == 1.0
    stepped = [[] for _ in keys]
    worst = 0
    for _ in range(12):
        eng.run(1, 0)
        for c, key in enumerate(keys):
            row = eng.ppc_draws(c)
            assert row.shape == (1, 4)
            it = int(eng.get('iter', c)) - 1
            u = device_draw('uniform', n=prob.R, key=key, it=it, stream=STREAM_PPC)
            t_obs, t_rep, det, sites, n_z1, margin = _columns(prob, eng.get('alpha', c), eng.get('z', c), u)
            assert margin >= 1e-12
            assert row[0, 2] == det and row[0, 3] == sites, (name, c, row[0], det, sites)
            got = [int(row[0, k] * 2.0 ** 32) for k in (0, 1)]
            assert all(row[0, k] * 2.0 ** 32 == got[k] for k in (0, 1))           # (whole quanta)
            diff = max(abs(got[0] - t_obs), abs(got[1] - t_rep))
            worst = max(worst, diff)
            assert diff <= n_z1, (name, c, got, t_obs, t_rep, n_z1)
            stepped[c].append(row[0])
    print(name, chains, 'largest difference from numpy, in quanta of 2^-32:', worst)
    eng.close()
    one = _engine(prob, keys, starts)
    one.run(12, 0)
    _same(_rows(one), [np.stack(r) for r in stepped])
    one.close()
    assert all(np.ptp(np.stack(r), axis=0).all() for r in stepped)        # (every column moves)


# ------------------------------------------------------------------ 2: bit-equal rows
SCHED_KEYS = ('OCC_EVENT_SYNC', 'OCC_STREAM_EVENTS', 'OCC_CU_SPLIT', 'OCC_NO_SIDE_STREAM', 'OCC_EAGER_ONLY', 'OCC_NO_PERSISTENT',
              'OCC_DEBUG_STREAMS_SERIALISED', 'OCC_NO_XCD_LOCAL')


def test_differently_split_calls_give_the_same_rows():
    prob, keys, starts = _workload_a(2)
    ref = _two_calls(prob, keys, starts)
    assert [r.shape for r in ref] == [(39, 4)] * 2
    _same(ref, _two_calls(prob, keys, starts, split=((5, 4), (28, 0), (3, 0), (7, 0))))
    _same(ref, _two_calls(prob, keys, starts, split=((5, 4), (1, 0), (37, 0))))     # (a call of one iteration)


@pytest.mark.parametrize('env', [{'OCC_EVENT_SYNC': '1'}, {'OCC_EVENT_SYNC': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_CU_SPLIT': '0'},
                                 {'OCC_DEBUG_STREAMS_SERIALISED': '1'},
                                 {'OCC_NO_SIDE_STREAM': '1'}, {'OCC_EAGER_ONLY': '1'}, {'OCC_NO_XCD_LOCAL': '1'},
                                 {'OCC_NO_XCD_LOCAL': '1', 'OCC_CU_SPLIT': '0'},
                                 {'OCC_NO_PERSISTENT': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_NO_PERSISTENT': '1', 'OCC_NO_SIDE_STREAM': '1'}])
def test_every_scheduling_mode_gives_the_same_rows(monkeypatch, env):
    """Graph replay against eager stepping (OCC_EAGER_ONLY) and every other way of scheduling an iteration."""
    prob, keys, starts = _workload_a(2)
    for k in SCHED_KEYS:
        monkeypatch.delenv(k, raising=False)
    ref = _two_calls(prob, keys, starts)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _same(ref, _two_calls(prob, keys, starts))


@pytest.mark.parametrize('name', ['generic', 'rsr40', 'rsr160', 'ragged'])
def test_graph_replay_equals_eager_stepping_on_the_other_kernels(monkeypatch, name):
    prob, keys, starts = WORKLOADS[name](2)
    monkeypatch.delenv('OCC_EAGER_ONLY', raising=False)
    ref = _two_calls(prob, keys, starts)
    monkeypatch.setenv('OCC_EAGER_ONLY', '1')
    _same(ref, _two_calls(prob, keys, starts))


def test_tile_looping_kernel_gives_the_rows_of_launch_per_step(monkeypatch):
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
        out[mode] = _rows(eng)
        assert eng.stats()['fused_fallbacks'] == 0
        eng.close()
    assert [r.shape for r in out['tiles']] == [(21, 4)] * 2
    _same(out['tiles'], out['launch_per_step'])


def test_batched_chains_have_the_rows_of_single_chain_runs():
    prob, _ = _problem_from_golden('ref_graph300_weighted')
    keys = [KEY, KEY ^ 0xABCDEF, 12345]
    rng = np.random.default_rng(3)
    starts = [dict(alpha=rng.standard_normal(prob.q), beta=rng.standard_normal(prob.p), tau=1.0 + c,
                   eta=(lambda e: e - e.mean())(rng.standard_normal(prob.n))) for c in range(3)]
    batch = _engine(prob, keys, starts)
    batch.run(20, 4)
    both = _rows(batch)
    batch.close()
    for c in range(3):
        solo = _engine(prob, [keys[c]], [starts[c]])
        solo.run(20, 4)
        _same([both[c]], _rows(solo))
        solo.close()
    assert [r.shape for r in both] == [(16, 4)] * 3


def test_engine_group_switches_everywhere_and_routes_by_chain():
    """Three chains over two engines (both on device 0 here): chain c lives on engine c % 2.  The checkpoint carries the
    switch, not the draws."""
    from occuspytial_amd._engine import Engine, EngineGroup
    prob, keys, starts = _workload_a(3)
    grp = EngineGroup(prob, keys, [0, 0], engine_factory=lambda pr, ks, dev: Engine(pr, ks, device=dev))
    for c in range(3):
        grp.set_start(c, **starts[c])
    grp.ppc_stats(True)
    assert grp._ppc_on
    grp.run(20, 5)
    first = [grp.ppc_draws(c) for c in range(3)]
    ck = grp.checkpoint()
    assert ck['ppc_stats'].tolist() == [1.0] * 3 and 'ppc_draws' not in ck
    grp.restore(ck)
    grp.run(10, 0)
    got = [np.concatenate([a, grp.ppc_draws(c)]) for c, a in enumerate(first)]
    grp.close()
    _same(_two_calls(prob, keys, starts, split=((20, 5), (10, 0))), got)


def _headline_rows(iters=10):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(100, 100, visits=5, p=2, q=2, random_state=0)
    prob = FlatProblem(Q, W, X, y)
    eng = _engine(prob, [KEY + 5 * c for c in range(4)], [_random_start(prob, 60 + c) for c in range(4)])
    eng.run(iters, 0)
    a = _rows(eng)
    eng.run(7, 2)
    out = [np.concatenate([u, v]) for u, v in zip(a, _rows(eng))], eng.stats()
    eng.close()
    return out


def _rsr_rows():
    prob, keys, starts = _rsr_problem(40)
    eng = _engine(prob, keys, starts)
    eng.run(8, 0)
    a = _rows(eng)
    eng.run(5, 1)
    out = [np.concatenate([u, v]) for u, v in zip(a, _rows(eng))], eng.stats()
    eng.close()
    return out


def test_a_call_rerun_after_a_barrier_timeout_counts_nothing_twice(monkeypatch):
    """The knobs of test_barrier_timeout_falls_back_to_launch_per_step_with_the_same_bits."""
    ref, _ = _headline_rows()
    monkeypatch.setenv('OCC_CU_SPLIT', '32')
    monkeypatch.setenv('OCC_DEBUG_SKIP_RESIDENCY_PROBE', '1')
    monkeypatch.setenv('OCC_QUIET', '1')
    alt, st = _headline_rows()
    assert st['fused_fallbacks'] == 1
    assert [r.shape for r in alt] == [(15, 4)] * 4
    _same(ref, alt)


def test_a_call_rerun_after_a_broken_handover_counts_nothing_twice(monkeypatch):
    """The knob of test_broken_stream_handover_falls_back_with_the_same_bits: fused ICAR path and reduced-rank model."""
    monkeypatch.setenv('OCC_QUIET', '1')
    ref, _ = _headline_rows()
    rsr_ref, _ = _rsr_rows()
    monkeypatch.setenv('OCC_DEBUG_BREAK_HANDOVER', '1')
    alt, st = _headline_rows()
    assert st['fused_fallbacks'] == 1
    _same(ref, alt)
    rsr_alt, rst = _rsr_rows()
    assert rst['fused_fallbacks'] == 1
    assert [r.shape for r in rsr_alt] == [(12, 4)] * 2
    _same(rsr_ref, rsr_alt)


def test_checkpoint_and_restore_carry_the_switch():
    prob, keys, starts = _workload_a(2)
    e1 = _engine(prob, keys, starts)
    e1.run(20, 5)
    ck = e1.checkpoint()
    assert ck['ppc_stats'].tolist() == [1.0, 1.0] and 'ppc_draws' not in ck
    e1.close()
    e2 = _engine(prob, keys, starts, on=False)           # a fresh engine that never heard of the check
    assert 'ppc_stats' not in e2.checkpoint()
    e2.restore(ck)
    assert e2.get('ppc_stats', 1)[0] == 1.0
    assert e2.ppc_draws(0).shape == (0, 4)               # the draws belong to a call and are not carried
    e2.run(15, 0)
    e3 = _engine(prob, keys, starts)
    e3.run(20, 5)
    e3.run(15, 0)
    _same(_rows(e2), _rows(e3))
    e2.close()
    e3.close()


def _sampler(cls_name='LogitICARGibbs', **kw):
    import occuspytial_amd
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(30, 40, visits=3, p=2, q=2, random_state=2)
    return getattr(occuspytial_amd, cls_name)(Q, W, X, y, random_state=7, **kw)


@pytest.mark.parametrize('cls_name, kw', [('LogitICARGibbs', {}), ('LogitRSRGibbs', dict(q=40))])
def test_sampler_returns_the_check_of_the_kept_draws(cls_name, kw):
    from occuspytial_amd.ppc import PredictiveCheck
    s = _sampler(cls_name, **kw)
    chunked = s.sample(60, burnin=20, chains=3, progressbar=True, ppc=True)   # chunks of 16: one straddles the burn-in
    one = _sampler(cls_name, **kw).sample(60, burnin=20, chains=3, progressbar=False, ppc=True)
    plain = _sampler(cls_name, **kw).sample(60, burnin=20, chains=3, progressbar=False)
    assert plain.ppc is None and isinstance(one.ppc, PredictiveCheck)
    assert sorted(one.data) == sorted(plain.data)                              # (post.summary and the chains are unchanged)
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(one[name], plain[name]) and np.array_equal(chunked[name], plain[name])
    for name in ('ft_obs', 'ft_rep', 'detections_rep', 'sites_detected_rep'):
        assert getattr(one.ppc, name).shape == (3, 40)
        assert np.array_equal(getattr(one.ppc, name), getattr(chunked.ppc, name)), name
    prob = s._problem
    assert one.ppc.detections == int(prob.y.sum()) and one.ppc.sites_detected == len(prob.obs) and one.ppc.n_draws == 120
    assert 0.0 <= one.ppc.p_value <= 1.0 and one.ppc.c_hat > 0.0 and 'p_value' in repr(one.ppc)
    # resume: the rows of the new draws are the tail of an uninterrupted run's
    ck = s.checkpoint()
    assert 'ppc_stats' in ck
    more = s.resume(ck, 30, progressbar=False, ppc=True)
    longer = _sampler(cls_name, **kw).sample(90, burnin=20, chains=3, progressbar=False, ppc=True)
    assert np.array_equal(more.ppc.ft_rep, longer.ppc.ft_rep[:, 40:]) and np.array_equal(more.ppc.ft_obs, longer.ppc.ft_obs[:, 40:])
    assert np.array_equal(more['alpha'], longer['alpha'][:, 40:])
    again = s.resume(ck, 5, progressbar=False)                                 # (not asked for: the checkpoint's switch goes off)
    assert again.ppc is None and not s._engine._ppc_on


@pytest.mark.parametrize('site, ll, regions', [(s, l, r) for s in (False, True) for l in (False, True) for r in (False, True)][1:])
def test_rows_are_the_same_beside_every_other_switch(site, ll, regions):
    prob, keys, starts = _workload_a(2)
    ids = (np.arange(prob.n) % 7).astype(np.int64) if regions else None
    _same(_two_calls(prob, keys, starts), _two_calls(prob, keys, starts, site=site, ll=ll, ids=ids))


# ------------------------------------------------------------------ 3: unchanged elsewhere
@pytest.mark.parametrize('name', ['lattice', 'ragged', 'generic', 'rsr40'])
def test_nothing_else_sees_the_switch(name):
    """alpha, beta, tau, eta, z, the site_* and ll_* sums and region_draws are the same bits with ppc_stats on and off."""
    prob, keys, starts = WORKLOADS[name](2)
    ids = (np.arange(prob.n) % 7).astype(np.int64)
    engines = {}
    for which in ('on', 'off'):
        eng = engines[which] = _engine(prob, keys, starts, on=which == 'on', site=True, ll=True, ids=ids)
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
        assert on.ppc_draws(c).shape == (10, 4)
    on.step()                                                   # occ_step never counts: the last call's rows stay
    assert on.ppc_draws(0).shape == (10, 4)
    for eng in engines.values():
        eng.close()


# ------------------------------------------------------------------ 4: a long run
def test_invariants_of_a_long_run():
    """450 iterations, 400 kept, four chains of which the last has its switch off: exactly `keep` rows, length 0 for the chain
    that does not count, 0 <= col3 <= col2 <= R, col3 <= the occupied surveyed sites (region_draws with the surveyed sites as
    one region), columns 0 and 1 not negative."""
    prob, keys, starts = _workload_a(4)
    ids = np.full(prob.n, -1, dtype=np.int64)
    ids[prob.site_id] = 0
    eng = _engine(prob, keys, starts, ids=ids)
    eng.set('ppc_stats', 0.0, 3)
    eng.run(450, 50)
    for c in range(3):
        rows = eng.ppc_draws(c)
        occupied = eng.region_draws(c)[:, 0]
        assert rows.shape == (400, 4) and occupied.shape == (400,)
        assert np.all(rows[:, 2:] == np.floor(rows[:, 2:]))
        assert np.all(0 <= rows[:, 3]) and np.all(rows[:, 3] <= rows[:, 2]) and np.all(rows[:, 2] <= prob.R)
        assert np.all(rows[:, 3] <= occupied)
        assert np.all(rows[:, :2] >= 0.0)
        assert np.all(np.ptp(rows, axis=0) > 0)
    assert eng.ppc_draws(3).shape == (0, 4) and eng.get('ppc_draws', 3).size == 0
    eng.close()


# ------------------------------------------------------------------ 5: refusals
@pytest.mark.parametrize('name', ['lattice', 'rsr40'])
def test_refusals(name):
    prob, keys, starts = WORKLOADS[name](2)
    eng = _engine(prob, keys, starts, on=False)
    for nm in ('ppc_stats', 'ppc_draws'):
        with pytest.raises(ValueError, match='set ppc_stats first'):
            eng.get(nm)
        v = np.zeros(8)
        n = __import__('ctypes').c_int64(0)
        assert eng._lib.occ_get_state(eng._h, 0, nm.encode(), v.ctypes.data, 8, __import__('ctypes').byref(n)) == -5     # OCC_E_STATE
    with pytest.raises(ValueError, match='set ppc_stats first'):
        eng.set('ppc_draws', np.zeros(4))
    for bad in (2.0, -1.0, 0.5, np.nan):
        with pytest.raises(ValueError, match='ppc_stats is 0 or 1'):
            eng.set('ppc_stats', bad)
        v = np.array([bad])
        assert eng._lib.occ_set_state(eng._h, 0, b'ppc_stats', v.ctypes.data, 1) == -1                                   # OCC_E_BADARG
    with pytest.raises(ValueError, match='wrong length'):
        eng.set('ppc_stats', np.ones(2))
    with pytest.raises(ValueError, match='set ppc_stats first'):      # (nothing of the refused values was kept)
        eng.get('ppc_stats')
    eng.set('ppc_stats', 1.0, 1)
    assert [eng.get('ppc_stats', c)[0] for c in (0, 1)] == [0.0, 1.0] and eng.get('ppc_draws', 1).size == 0
    with pytest.raises(ValueError, match='read-only'):
        eng.set('ppc_draws', np.zeros(4))
    eng.set_start(1, **starts[1])                                      # occ_set_start and occ_set_keys do not touch the switch
    eng.set_keys(keys)
    assert eng.get('ppc_stats', 1)[0] == 1.0
    eng.run(3, 1)
    assert eng.ppc_draws(0).shape == (0, 4) and eng.ppc_draws(1).shape == (2, 4)
    eng.set('ppc_stats', 0.0, 1)
    eng.run(3, 1)
    assert eng.ppc_draws(1).shape == (0, 4) and eng.get('ppc_stats', 1)[0] == 0.0      # (still answered: it has been on)
    eng.close()


def test_probit_handle_refuses():
    from .test_gpu_regions import _probit_problem
    from occuspytial_amd._engine import Engine
    prob, keys, starts = _probit_problem(2)
    eng = Engine(prob, keys)
    for nm in ('ppc_stats', 'ppc_draws'):
        with pytest.raises(ValueError, match='posterior predictive checks are not available for the probit model'):
            eng.get(nm)
    with pytest.raises(ValueError, match='posterior predictive checks are not available for the probit model'):
        eng.set('ppc_stats', 1.0)
    v = np.ones(1)
    assert eng._lib.occ_set_state(eng._h, 0, b'ppc_stats', v.ctypes.data, 1) == -5                                        # OCC_E_STATE
    eng.close()


# ------------------------------------------------------------------ 6: one decision that must come out right
DECISION = dict(n=400, visits=4, seed=11, coef=4.0, site_seed=303, noise_seed=101, y_seed=202, size=400, burnin=100, chains=2)
CPU_P_VALUE = dict(A=0.442, B=0.002)   # on the CPU restatement of the ABI (see the test's docstring)
CPU_C_HAT = dict(A=1.025, B=2.207)


def _decision_models():
    """The recipe of test_gpu_waic's ``_decision_models`` -- a 20x20-site problem of ``make_data``, every site surveyed four
    times, p = q = 2, detections drawn afresh as y_r ~ Bernoulli(z_i expit(-0.5 + coef w_i)) -- with a detection covariate
    that is CONSTANT within a site, w_i ~ U(-2, 2): per-visit noise averages out of a site's total, a site-level effect
    overdisperses the totals.  Model A is given the covariate; model B gets independent per-visit noise of the same law in
    its place.  Fixed seeds.  -> (Q, W_A, W_B, X, y)."""
    from occuspytial_amd.utils import make_data
    d = DECISION
    Q, W, X, _, _, _, _, z = make_data(n=d['n'], min_v=d['visits'], max_v=d['visits'], ns=d['n'], p=2, q=2, random_state=d['seed'])
    rng_y, rng_b, rng_s = np.random.default_rng(d['y_seed']), np.random.default_rng(d['noise_seed']), np.random.default_rng(d['site_seed'])
    WA, WB, y = {}, {}, {}
    for site in sorted(W):
        Wi = np.asarray(W[site], dtype=float).copy()
        Wi[:, 1] = rng_s.uniform(-2, 2)
        y[site] = rng_y.binomial(1, z[site] * expit(-0.5 + d['coef'] * Wi[:, 1]))
        WA[site] = Wi
        Wb = Wi.copy()
        Wb[:, 1] = rng_b.uniform(-2, 2, size=Wi.shape[0])
        WB[site] = Wb
    return Q, WA, WB, X, y


def test_the_check_accepts_the_model_that_has_the_site_covariate_and_rejects_the_other():
    """A's p_value inside (0.1, 0.9), B's below 0.05, c_hat(B) > c_hat(A).  Seed, coefficient and length were chosen on the CPU:
    both models stepped with the CPU restatement of the ABI (2 chains, 400 iterations, 100 of them burn-in, the sampler's own
    start values and keys), the four columns formed in numpy from alpha and z of every kept iteration with numpy uniforms.
    There A has p_value 0.442 (required: inside (0.25, 0.75)) and c_hat 1.025, B has p_value 0.002 (required: below 0.005, a
    factor of ten inside the threshold) and c_hat 2.207; 424 detections at 137 of the 400 sites.  (With coefficient 1.5 B's
    p-value was 0.117 and with 2.5 it was 0.010: the z of a site without a detection absorbs part of the overdispersion.)"""
    from occuspytial_amd import LogitICARGibbs
    d = DECISION
    Q, WA, WB, X, y = _decision_models()
    out = {}
    for name, W in (('A', WA), ('B', WB)):
        post = LogitICARGibbs(Q, W, X, y, random_state=5).sample(d['size'], burnin=d['burnin'], chains=d['chains'], progressbar=False, ppc=True)
        out[name] = post.ppc
        print('model', name, post.ppc, 'on the CPU: p_value', CPU_P_VALUE[name], 'c_hat', CPU_C_HAT[name])
        assert post.ppc.n_draws == (d['size'] - d['burnin']) * d['chains']
    assert 0.1 < out['A'].p_value < 0.9
    assert out['B'].p_value < 0.05
    assert out['B'].c_hat > out['A'].c_hat
