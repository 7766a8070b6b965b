"""Occupied sites per region and draw, counted on the device (state names ``region_id``, ``region_stats``, ``region_draws``).

Counts are integers, so every comparison in this file is equality: against ``np.bincount`` of the z read back, between every
way the engine can schedule an iteration, through both run-time fallbacks and checkpoint / restore, and against the per-site
sums of z that were merged before (``site_z``).  Workloads: A, the 30x40 lattice; the wide-row graph fixture; G, 17x19 with
nine covariates of each kind (the generic kernels); the reduced-rank model on both solve paths (40 and 160 basis columns);
``ProbitRSRGibbs``.  Every test runs under its own time limit (``_time_limit``), and the engine's own host waits have theirs.
"""

import numpy as np
import pytest

from ._outputs_gpu import engine_with, time_limit as _time_limit, two_calls  # noqa: F401 (autouse in this module)
from .test_gpu_parity import KEY, _problem_from_golden, _random_start
from .test_gpu_site_summaries import _rsr_problem, _workload_a, _workload_g

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers
def _ids(n, G, seed=1):
    """A map with exactly G regions: G = 1 the whole lattice; G = 7 with about an eighth of the sites in none; G = 256."""
    rng = np.random.default_rng(seed)
    if G == 1:
        return np.zeros(n, dtype=np.int64)
    ids = rng.integers(-1 if G == 7 else 0, G, size=n)
    ids[rng.permutation(n)[:G]] = np.arange(G)          # every region has a site
    if G == 7:
        ids[rng.permutation(n)[G:G + 5]] = -1
        assert np.count_nonzero(ids < 0) >= 5
    assert ids.max() == G - 1
    return ids


def _bincount(ids, z, G):
    return np.bincount(ids[(ids >= 0) & (np.asarray(z) != 0)], minlength=G)


def _detected(prob):
    seen = np.zeros(prob.n, dtype=bool)
    seen[np.asarray(prob.obs, dtype=int)] = True
    return seen


def _engine(prob, keys, starts, ids=None, on=True, **kw):
    return engine_with(prob, keys, starts, ids=ids, region_on=on, **kw)


def _probit_problem(chains=2, q=12):
    from occuspytial_amd import ProbitRSRGibbs
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(20, 23, visits=3, p=3, q=2, random_state=6)
    s = ProbitRSRGibbs(Q, W, X, y, random_state=10, q=q)
    prob = s._problem
    rng = np.random.default_rng(12)
    m = prob.probit['dim']
    starts = [dict(alpha=rng.standard_normal(prob.q), beta=rng.standard_normal(prob.p), tau=1.0 + c, eta=rng.standard_normal(m),
                   eps=rng.standard_normal(prob.n)) for c in range(chains)]
    return prob, [KEY + 3 * c for c in range(chains)], starts


def _rows(eng):
    return [eng.region_draws(c) for c in range(eng.n_chains)]


def _two_calls(prob, keys, starts, ids, **kw):
    """run(33, 4) then run(10, 0) -> per chain the 39 recorded rows, (39, G)."""
    return two_calls(lambda: _engine(prob, keys, starts, ids, **kw), _rows, per_call=True)


def _same(a, b):
    assert len(a) == len(b)
    for c, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and np.array_equal(u, v), (c, u.shape, v.shape)


# ------------------------------------------------------------------ 1: exactness
WORKLOADS = {
    'lattice': lambda chains: _workload_a(chains),
    'wide_rows': lambda chains: (lambda pr: (pr[0], [KEY], [pr[1]]))(_problem_from_golden('ref_graph300_weighted')),
    'generic': lambda chains: _workload_g(),
    'rsr40': lambda chains: _rsr_problem(40),
    'rsr160': lambda chains: _rsr_problem(160),
    'probit': lambda chains: _probit_problem(chains),
}
CASES = [('lattice', c, G) for c in (1, 2, 4) for G in (1, 7, 256)] + [
    ('wide_rows', 1, 7), ('wide_rows', 1, 256), ('generic', 1, 1), ('generic', 1, 256), ('rsr40', 2, 7), ('rsr160', 2, 1),
    ('probit', 1, 256), ('probit', 2, 7), ('probit', 4, 1)]


@pytest.mark.parametrize('name, chains, G', CASES)
def test_counts_equal_the_bincount_of_z_read_back(name, chains, G):
    """Twelve iterations as twelve run(1, 0) calls: after each, region_draws is np.bincount of the chain's z by region; the
    same twelve as one run(12, 0) give the same rows."""
    prob, keys, starts = WORKLOADS[name](chains)
    ids = _ids(prob.n, G)
    eng = _engine(prob, keys, starts, ids)
    assert np.array_equal(eng.get('region_id'), ids) and eng.get('region_stats')[0] == 1.0
    stepped = [[] for _ in keys]
    for _ in range(12):
        eng.run(1, 0)
        for c in range(len(keys)):
            row = eng.region_draws(c)
            assert row.shape == (1, G)
            assert np.array_equal(row[0], _bincount(ids, eng.get('z', c), G)), (name, c)
            stepped[c].append(row[0])
    final_z = [eng.get('z', c) for c in range(len(keys))]
    eng.close()
    one = _engine(prob, keys, starts, ids)
    one.run(12, 0)
    _same(_rows(one), [np.stack(r) for r in stepped])
    for c in range(len(keys)):
        assert np.array_equal(one.get('z', c), final_z[c])
    one.close()
    assert any(np.ptp(np.stack(r), axis=0).any() for r in stepped)        # (the counts move: z is being drawn)


# ------------------------------------------------------------------ 2: determinism
SCHED_KEYS = ('OCC_EVENT_SYNC', 'OCC_STREAM_EVENTS', 'OCC_CU_SPLIT', 'OCC_NO_SIDE_STREAM', 'OCC_EAGER_ONLY', 'OCC_NO_PERSISTENT',
              'OCC_DEBUG_STREAMS_SERIALISED', 'OCC_NO_XCD_LOCAL')


@pytest.mark.parametrize('env', [{'OCC_EVENT_SYNC': '1'}, {'OCC_EVENT_SYNC': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_CU_SPLIT': '0'},
                                 {'OCC_DEBUG_STREAMS_SERIALISED': '1'},
                                 {'OCC_NO_SIDE_STREAM': '1'}, {'OCC_EAGER_ONLY': '1'}, {'OCC_NO_XCD_LOCAL': '1'},
                                 {'OCC_NO_XCD_LOCAL': '1', 'OCC_CU_SPLIT': '0'},
                                 {'OCC_NO_PERSISTENT': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_NO_PERSISTENT': '1', 'OCC_NO_SIDE_STREAM': '1'}])
def test_every_scheduling_mode_gives_the_same_rows(monkeypatch, env):
    """Graph replay against eager stepping (OCC_EAGER_ONLY) and every other way of scheduling an iteration."""
    prob, keys, starts = _workload_a(2)
    ids = _ids(prob.n, 7)
    for k in SCHED_KEYS:
        monkeypatch.delenv(k, raising=False)
    ref = _two_calls(prob, keys, starts, ids)
    assert [r.shape for r in ref] == [(39, 7)] * 2
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _same(ref, _two_calls(prob, keys, starts, ids))


@pytest.mark.parametrize('name', ['generic', 'rsr40', 'rsr160', 'probit'])
def test_graph_replay_equals_eager_stepping_on_the_other_kernels(monkeypatch, name):
    prob, keys, starts = WORKLOADS[name](2)
    ids = _ids(prob.n, 7)
    monkeypatch.delenv('OCC_EAGER_ONLY', raising=False)
    ref = _two_calls(prob, keys, starts, ids)
    if name == 'probit':     # (its occ_run has one path; a call split in two replays fewer whole graphs and steps the rest)
        eng = _engine(prob, keys, starts, ids)
        parts = []
        for n_iter, burnin in ((5, 4), (28, 0), (3, 0), (7, 0)):
            eng.run(n_iter, burnin)
            parts.append(_rows(eng))
        eng.close()
        _same(ref, [np.concatenate([p[c] for p in parts]) for c in range(len(keys))])
        return
    monkeypatch.setenv('OCC_EAGER_ONLY', '1')
    _same(ref, _two_calls(prob, keys, starts, ids))


def test_tile_looping_kernel_gives_the_rows_of_launch_per_step(monkeypatch):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(61, 67, visits=3, p=2, q=2, random_state=5)
    prob = FlatProblem(Q, W, X, y)
    keys = [KEY + 7 * c for c in range(2)]
    starts = [_random_start(prob, 11 + c) for c in range(2)]
    ids = _ids(prob.n, 256)
    monkeypatch.setenv('OCC_FORCE_TILES', '1')
    out = {}
    for mode in ('tiles', 'launch_per_step'):
        monkeypatch.delenv('OCC_NO_PERSISTENT', raising=False)
        if mode == 'launch_per_step':
            monkeypatch.setenv('OCC_NO_PERSISTENT', '1')
        eng = _engine(prob, keys, starts, ids)
        assert eng.stats()['persistent_solve'] == (3 if mode == 'tiles' else 0)
        eng.run(24, 3)
        out[mode] = _rows(eng)
        assert eng.stats()['fused_fallbacks'] == 0
        eng.close()
    assert [r.shape for r in out['tiles']] == [(21, 256)] * 2
    _same(out['tiles'], out['launch_per_step'])


def test_batched_chains_have_the_rows_of_single_chain_runs():
    prob, _ = _problem_from_golden('ref_graph300_weighted')
    keys = [KEY, KEY ^ 0xABCDEF, 12345]
    rng = np.random.default_rng(3)
    starts = [dict(alpha=rng.standard_normal(prob.q), beta=rng.standard_normal(prob.p), tau=1.0 + c,
                   eta=(lambda e: e - e.mean())(rng.standard_normal(prob.n))) for c in range(3)]
    ids = _ids(prob.n, 7)
    batch = _engine(prob, keys, starts, ids)
    batch.run(20, 4)
    both = _rows(batch)
    batch.close()
    for c in range(3):
        solo = _engine(prob, [keys[c]], [starts[c]], ids)
        solo.run(20, 4)
        _same([both[c]], _rows(solo))
        solo.close()
    assert [r.shape for r in both] == [(16, 7)] * 3
    pprob, pkeys, pstarts = _probit_problem(3)
    pids = _ids(pprob.n, 7)
    batch = _engine(pprob, pkeys, pstarts, pids)
    batch.run(20, 4)
    both = _rows(batch)
    batch.close()
    solo = _engine(pprob, [pkeys[2]], [pstarts[2]], pids)
    solo.run(20, 4)
    _same([both[2]], _rows(solo))
    solo.close()


def test_engine_group_sets_the_map_everywhere_and_routes_by_chain():
    """Three chains over two engines (both on device 0 here): chain c lives on engine c % 2."""
    from occuspytial_amd._engine import Engine, EngineGroup
    prob, keys, starts = _workload_a(3)
    ids = _ids(prob.n, 7)
    grp = EngineGroup(prob, keys, [0, 0], engine_factory=lambda pr, ks, dev: Engine(pr, ks, device=dev))
    for c in range(3):
        grp.set_start(c, **starts[c])
    grp.regions(ids)
    grp.region_stats(True)
    grp.run(20, 5)
    first = [grp.region_draws(c) for c in range(3)]
    ck = grp.checkpoint()
    assert ck['region_id'].shape == (3, prob.n) and np.array_equal(ck['region_id'][2], ids) and ck['region_stats'].tolist() == [1.0] * 3
    assert 'region_draws' not in ck
    grp.restore(ck)
    grp.run(10, 0)
    got = [np.concatenate([a, grp.region_draws(c)]) for c, a in enumerate(first)]
    grp.close()
    one = _engine(prob, keys, starts, ids)
    one.run(20, 5)
    a = _rows(one)
    one.run(10, 0)
    _same([np.concatenate([u, v]) for u, v in zip(a, _rows(one))], got)
    one.close()


def test_rows_sums_and_draws_do_not_see_each_other():
    """The rows are the same with any combination of site_stats / ll_stats beside them; the site_* and ll_* sums are the same
    bits with and without region_stats; alpha, beta, tau, eta and z are the same bits with the switch on and off; and one
    chain with the switch off beside one with it on returns length 0."""
    prob, keys, starts = _workload_a(2)
    ids = _ids(prob.n, 7)
    ref = _two_calls(prob, keys, starts, ids)
    for site, ll in ((True, False), (False, True), (True, True)):
        _same(ref, _two_calls(prob, keys, starts, ids, site=site, ll=ll))
    engines = {}
    for name, kw in (('on', dict(ids=ids)), ('off', dict(ids=ids, on=False)), ('never', dict())):
        eng = engines[name] = _engine(prob, keys, starts, site=True, ll=True, **kw)
        eng.rec = eng.run(33, 4) + eng.run(10, 0)
    on, off, never = engines['on'], engines['off'], engines['never']
    assert [r.shape for r in _rows(on)] == [(10, 7)] * 2 and [r.shape for r in _rows(off)] == [(0, 7)] * 2
    for other in (off, never):
        for u, v in zip(on.rec, other.rec):
            assert np.array_equal(u, v)
        for c in range(2):
            for nm in ('alpha', 'beta', 'eta', 'z'):
                assert np.array_equal(on.get(nm, c), other.get(nm, c)), nm
            assert on.get('tau', c) == other.get('tau', c)
            a, b = on.site_sums(c), other.site_sums(c)
            assert a['count'] == b['count'] == 39 and all(np.array_equal(a[k], b[k]) for k in ('psi', 'occ', 'z', 'eta', 'eta2'))
            a, b = on.loglik_sums(c), other.loglik_sums(c)
            assert a['count'] == b['count'] == 39 and all(np.array_equal(a[k], b[k]) for k in ('lik', 'log', 'log2'))
    # one chain on, one off, in one handle; then the map can be changed only with every switch off
    off.set('region_stats', 1.0, 1)
    assert [off.get('region_stats', c)[0] for c in (0, 1)] == [0.0, 1.0]
    more = off.run(6, 1)
    on.run(6, 1)
    assert off.region_draws(0).shape == (0, 7) and np.array_equal(off.region_draws(1), on.region_draws(1))
    assert np.array_equal(more[0], never.run(6, 1)[0])
    for eng in engines.values():
        eng.close()


def test_probit_draws_do_not_depend_on_the_switch():
    prob, keys, starts = _probit_problem(2)
    ids = _ids(prob.n, 7)
    on, off = _engine(prob, keys, starts, ids), _engine(prob, keys, starts)
    r_on, r_off = on.run(33, 4) + on.run(10, 0), off.run(33, 4) + off.run(10, 0)
    for u, v in zip(r_on, r_off):
        assert np.array_equal(u, v)
    for c in range(2):
        for nm in ('alpha', 'beta', 'eta', 'eps', 'z', 'c'):
            assert np.array_equal(on.get(nm, c), off.get(nm, c)), nm
        assert np.array_equal(on.region_draws(c)[-1], _bincount(ids, on.get('z', c), 7))
    on.step()                                                   # occ_step never counts: the last call's rows stay
    assert on.region_draws(0).shape == (10, 7)
    on.close()
    off.close()


def _headline_rows(G=7, iters=10):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(100, 100, visits=5, p=2, q=2, random_state=0)
    prob = FlatProblem(Q, W, X, y)
    eng = _engine(prob, [KEY + 5 * c for c in range(4)], [_random_start(prob, 60 + c) for c in range(4)], _ids(prob.n, G), site=True)
    eng.run(iters, 0)
    a = _rows(eng)
    eng.run(7, 2)
    out = [np.concatenate([u, v]) for u, v in zip(a, _rows(eng))], [eng.site_sums(c) for c in range(4)], eng.stats()
    eng.close()
    return out


def _rsr_rows():
    prob, keys, starts = _rsr_problem(40)
    eng = _engine(prob, keys, starts, _ids(prob.n, 7))
    eng.run(8, 0)
    a = _rows(eng)
    eng.run(5, 1)
    out = [np.concatenate([u, v]) for u, v in zip(a, _rows(eng))], eng.stats()
    eng.close()
    return out


def test_a_call_rerun_after_a_barrier_timeout_counts_nothing_twice(monkeypatch):
    """The knobs of test_barrier_timeout_falls_back_to_launch_per_step_with_the_same_bits."""
    ref, ref_site, _ = _headline_rows()
    monkeypatch.setenv('OCC_CU_SPLIT', '32')
    monkeypatch.setenv('OCC_DEBUG_SKIP_RESIDENCY_PROBE', '1')
    monkeypatch.setenv('OCC_QUIET', '1')
    alt, alt_site, st = _headline_rows()
    assert st['fused_fallbacks'] == 1
    assert [r.shape for r in alt] == [(15, 7)] * 4
    _same(ref, alt)
    for a, b in zip(ref_site, alt_site):
        assert a['count'] == b['count'] == 15 and np.array_equal(a['z'], b['z'])


def test_a_call_rerun_after_a_broken_handover_counts_nothing_twice(monkeypatch):
    """The knob of test_broken_stream_handover_falls_back_with_the_same_bits: fused ICAR path and reduced-rank model."""
    monkeypatch.setenv('OCC_QUIET', '1')
    ref, _, _ = _headline_rows(G=256)
    rsr_ref, _ = _rsr_rows()
    monkeypatch.setenv('OCC_DEBUG_BREAK_HANDOVER', '1')
    alt, _, st = _headline_rows(G=256)
    assert st['fused_fallbacks'] == 1
    _same(ref, alt)
    rsr_alt, rst = _rsr_rows()
    assert rst['fused_fallbacks'] == 1
    assert [r.shape for r in rsr_alt] == [(12, 7)] * 2
    _same(rsr_ref, rsr_alt)


@pytest.mark.parametrize('name', ['lattice', 'probit'])
def test_checkpoint_and_restore_carry_map_and_switch(name):
    prob, keys, starts = WORKLOADS[name](2)
    ids = _ids(prob.n, 7)
    e1 = _engine(prob, keys, starts, ids)
    e1.run(20, 5)
    ck = e1.checkpoint()
    assert np.array_equal(ck['region_id'][0], ids) and ck['region_stats'].tolist() == [1.0, 1.0] and 'region_draws' not in ck
    e1.close()
    e2 = _engine(prob, keys, starts)           # a fresh engine that never heard of regions
    e2.restore(ck)
    assert np.array_equal(e2.get('region_id'), ids) and e2.get('region_stats', 1)[0] == 1.0
    assert e2.region_draws(0).shape == (0, 7)  # the draws belong to a call and are not carried
    e2.run(15, 0)
    e3 = _engine(prob, keys, starts, ids)
    e3.run(20, 5)
    e3.run(15, 0)
    _same(_rows(e2), _rows(e3))
    e2.close()
    e3.close()


def _sampler(cls_name='LogitICARGibbs', **kw):
    import occuspytial_amd
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(30, 40, visits=3, p=2, q=2, random_state=2)
    return getattr(occuspytial_amd, cls_name)(Q, W, X, y, random_state=7, **kw), X.shape[0]


@pytest.mark.parametrize('cls_name, kw', [('LogitICARGibbs', {}), ('LogitRSRGibbs', dict(q=40)), ('ProbitRSRGibbs', dict(q=20))])
def test_sampler_returns_the_occupied_sites_of_the_kept_draws(cls_name, kw):
    s, n = _sampler(cls_name, **kw)
    ids = _ids(n, 7)
    chunked = s.sample(60, burnin=20, chains=3, progressbar=True, regions=ids)   # chunks of 16: one straddles the burn-in
    s_one = _sampler(cls_name, **kw)[0]
    one = s_one.sample(60, burnin=20, chains=3, progressbar=False, regions=ids)
    plain = _sampler(cls_name, **kw)[0].sample(60, burnin=20, chains=3, progressbar=False)
    assert plain.regions is None and 'occupied' not in plain.data
    assert one['occupied'].shape == (3, 40, 7) and one['occupied'].dtype == np.float64
    assert np.array_equal(chunked['occupied'], one['occupied'])
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(one[name], plain[name]) and np.array_equal(chunked[name], plain[name])
    r = one.regions
    assert np.array_equal(r.sizes, np.bincount(ids[ids >= 0], minlength=7))
    assert np.array_equal(r.detected, _bincount(ids, _detected(s._problem), 7))
    assert np.all(one['occupied'] >= r.detected) and np.all(one['occupied'] <= r.sizes)
    assert np.array_equal(r.pao, one['occupied'] / r.sizes)
    assert np.array_equal(one['occupied'][0, -1], _bincount(ids, s_one.state.z, 7))      # (state.z: chain 0 after its last draw)
    summ = one.summary
    assert 'occupied[3]' in (list(summ.index) if hasattr(summ, 'index') else list(summ))
    whole = _sampler(cls_name, **kw)[0].sample(60, burnin=20, chains=3, progressbar=False, regions=True)
    assert whole['occupied'].shape == (3, 40, 1)
    all_in = _sampler(cls_name, **kw)[0].sample(60, burnin=20, chains=3, progressbar=False, regions=np.where(ids < 0, 0, ids))
    assert np.array_equal(whole['occupied'][:, :, 0], all_in['occupied'].sum(axis=2))
    # resume: the rows of the new draws are the tail of an uninterrupted run's
    ck = s.checkpoint()
    assert 'region_id' in ck
    more = s.resume(ck, 30, progressbar=False, regions=ids)
    longer = _sampler(cls_name, **kw)[0].sample(90, burnin=20, chains=3, progressbar=False, regions=ids)
    assert np.array_equal(more['occupied'], longer['occupied'][:, 40:]) and np.array_equal(more['alpha'], longer['alpha'][:, 40:])
    assert np.array_equal(more.regions.pao, more['occupied'] / r.sizes)


# ------------------------------------------------------------------ 3: against the code already merged
@pytest.mark.parametrize('name, G', [('lattice', 7), ('lattice', 256), ('generic', 7), ('rsr40', 1), ('rsr160', 7)])
def test_rows_add_up_to_the_per_site_sums_of_z(name, G):
    """site_stats on over the same kept iterations: for every region, sum_t occupied[t, g] == sum_{i in g} site_z[i], exactly
    (both are integers far below 2^53)."""
    prob, keys, starts = WORKLOADS[name](2)
    ids = _ids(prob.n, G)
    eng = _engine(prob, keys, starts, ids, site=True)
    eng.run(40, 7)
    for c in range(len(keys)):
        sums = eng.site_sums(c)
        assert sums['count'] == 33
        rows = eng.region_draws(c)
        assert rows.shape == (33, G)
        want = np.bincount(ids[ids >= 0], weights=sums['z'][ids >= 0], minlength=G)
        assert np.array_equal(rows.sum(axis=0), want), (name, c)
    eng.close()


# ------------------------------------------------------------------ 4: invariants
def test_invariants_of_a_long_run():
    """450 iterations, 400 kept, four chains of which the last has its switch off: exactly `keep` rows, every count between
    the region's sites with a detection and its size, and length 0 for the chain that does not count."""
    prob, keys, starts = _workload_a(4)
    ids = _ids(prob.n, 7)
    eng = _engine(prob, keys, starts, ids)
    eng.set('region_stats', 0.0, 3)
    eng.run(450, 50)
    sizes = np.bincount(ids[ids >= 0], minlength=7)
    det = _bincount(ids, _detected(prob), 7)
    assert det.sum() > 0 and np.all(det < sizes)
    for c in range(3):
        rows = eng.region_draws(c)
        assert rows.shape == (400, 7)
        assert np.all(rows == np.floor(rows)) and np.all(rows >= det) and np.all(rows <= sizes)
        assert np.array_equal(rows[-1], _bincount(ids, eng.get('z', c), 7))
        assert np.all(np.ptp(rows, axis=0) > 0)
    assert eng.region_draws(3).shape == (0, 7) and eng.get('region_draws', 3).size == 0
    eng.close()


# ------------------------------------------------------------------ 5: refusals
@pytest.mark.parametrize('name', ['lattice', 'rsr40', 'probit'])
def test_refusals(name):
    prob, keys, starts = WORKLOADS[name](2)
    eng = _engine(prob, keys, starts)
    for nm in ('region_id', 'region_stats', 'region_draws'):
        with pytest.raises(ValueError, match='set region_id first'):
            eng.get(nm)
    with pytest.raises(ValueError, match='set region_id first'):
        eng.set('region_stats', 1.0)
    with pytest.raises(ValueError, match='set region_id first'):
        eng.set('region_draws', np.zeros(3))
    ids = _ids(prob.n, 7).astype(float)
    for bad in (np.where(np.arange(prob.n) == 5, 0.5, ids), np.where(np.arange(prob.n) == 5, 256.0, ids),
                np.where(np.arange(prob.n) == 5, -2.0, ids), np.where(np.arange(prob.n) == 5, np.nan, ids)):
        with pytest.raises(ValueError, match='whole numbers from -1'):
            eng.set('region_id', bad)
        assert eng._lib.occ_set_state(eng._h, 0, b'region_id', bad.ctypes.data, bad.size) == -1        # OCC_E_BADARG
    with pytest.raises(ValueError, match='wrong length'):
        eng.set('region_id', ids[:-1])
    with pytest.raises(ValueError, match='set region_id first'):      # (nothing of the refused maps was kept)
        eng.get('region_id')
    eng.set('region_id', ids, 1)                                       # any valid chain index sets the handle's map ...
    assert np.array_equal(eng.get('region_id', 0), ids)                # ... and reads it
    assert eng.get('region_draws').size == 0 and eng.get('region_stats')[0] == 0.0
    eng.set('region_stats', 1.0, 1)
    with pytest.raises(ValueError, match='while a chain has region_stats on'):
        eng.set('region_id', ids)
    assert eng._lib.occ_set_state(eng._h, 0, b'region_id', ids.ctypes.data, ids.size) == -5            # OCC_E_STATE
    with pytest.raises(ValueError, match='0 or 1'):
        eng.set('region_stats', 2.0)
    with pytest.raises(ValueError, match='read-only'):
        eng.set('region_draws', np.zeros(7))
    # occ_set_start and occ_set_keys touch neither map nor switch
    st = dict(starts[1])
    eps = st.pop('eps', None)
    eng.set_start(1, **st)
    if eps is not None:
        eng.set('eps', eps, 1)
    eng.set_keys(keys)
    assert eng.get('region_stats', 1)[0] == 1.0 and np.array_equal(eng.get('region_id'), ids)
    eng.set('region_stats', 0.0, 1)
    eng.set('region_id', np.zeros(prob.n))                              # all switches off: the map may change, G with it
    eng.region_stats(True)
    eng._regions = np.zeros(prob.n, dtype=np.int64)
    eng.run(3, 1)
    assert eng.region_draws(0).shape == (2, 1)
    if name == 'probit':      # the existing refusals of the probit handle are what they were
        for nm in ('site_stats', 'site_z', 'll_stats', 'll_lik'):
            with pytest.raises(ValueError, match='not available for the probit model'):
                eng.get(nm)
        with pytest.raises(ValueError, match='not available for the probit model'):
            eng.set('site_stats', 1.0)
        with pytest.raises(ValueError, match='not available for the probit model'):
            eng.set('ll_stats', 1.0)
    eng.close()
