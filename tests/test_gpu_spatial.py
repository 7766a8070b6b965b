"""Spatial residual check, formed on the device (state names ``moran_stats``, ``moran_draws``; csrc/occ_spatial.hpp).

Per kept draw two kernels behind the z update add eight signed integer sums in 2^-32 fixed point: A, B, C, D of Moran's I of
the occupancy residuals r = z - psi, and the same of one replicate r* = z* - psi.  Integer sums do not depend on the order of
addition, so every comparison between two ways of running the engine is equality; the comparison with numpy (``_columns``)
is within one quantum per site.  Workloads: 13x17 and 30x40 queen lattices, the weighted 300-node graph of the golden
fixtures, the 700-site `hub` graph of tests/_layout_graphs.py (true SELL-64 bases, one row of 46 off-diagonals), 17x19 with nine covariates of each kind (the generic kernels), the reduced-rank model at 40 columns.  Every test
runs under its own time limit (``_time_limit``).
"""

import numpy as np
import pytest
from scipy import sparse
from scipy.special import expit

from ._outputs_gpu import engine_with, time_limit as _time_limit, two_calls  # noqa: F401 (autouse in this module)
from .test_gpu_parity import KEY, _problem_from_golden, _random_start
from .test_gpu_ppc import SCHED_KEYS
from .test_gpu_site_summaries import _rsr_problem, _workload_a, _workload_g

pytestmark = pytest.mark.gpu
STREAM_SPATIAL = 14
Q32 = 2.0 ** 32


# ------------------------------------------------------------------ helpers
def _engine(prob, keys, starts, on=True, **kw):
    return engine_with(prob, keys, starts, moran=on, **kw)


def _rows(eng):
    return [eng.moran_draws(c) for c in range(eng.n_chains)]


def _two_calls(prob, keys, starts, split=((33, 4), (10, 0)), **kw):
    """run(33, 4) then run(10, 0) -> per chain the 39 recorded rows, (39, 8)."""
    return two_calls(lambda: _engine(prob, keys, starts, **kw), _rows, split, per_call=True)


def _same(a, b):
    assert len(a) == len(b)
    for c, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.shape[1] == 8 and np.array_equal(u, v), (c, u.shape, v.shape)


def _weights(prob):
    """-> (W = -offdiag(Q) as CSR, d = its row sums, S0)."""
    Q = sparse.csr_matrix(prob.Q)
    W = -(Q - sparse.diags(Q.diagonal()))
    W = sparse.csr_matrix(W)
    W.eliminate_zeros()
    d = np.asarray(W.sum(axis=1)).ravel()
    return W, d, float(d.sum())


def _moran(cols, n, S0):
    A, B, C, D = cols
    rbar = C / n
    return (n / S0) * (A - 2 * rbar * B + rbar * rbar * S0) / (D - n * rbar * rbar)


def _columns(prob, W, d, beta, eta, z, u):
    """The eight columns of one draw from their definitions, in numpy -> (quanta as Python integers, the real-valued sums,
    the smallest |u - psi|)."""
    psi = expit(prob.X @ np.asarray(beta) + np.asarray(eta))
    out, real = [], []
    for zz in ((np.asarray(z) != 0).astype(np.float64), (u < psi).astype(np.float64)):
        r = zz - psi
        terms = (r * (W @ r), d * r, r, r * r)
        out += [int(np.rint(t * Q32).astype(np.int64).sum()) for t in terms]
        real += [float(t.sum()) for t in terms]
    return out, real, float(np.abs(u - psi).min())


def _lattice(rows, cols, chains, seed):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(rows, cols, visits=3, p=2, q=2, random_state=seed)
    prob = FlatProblem(Q, W, X, y)
    return prob, [KEY + 13 * c for c in range(chains)], [_random_start(prob, 40 + c) for c in range(chains)]


def _hub(chains):
    from . import _layout_graphs as G
    prob = G.survey(G.graph('hub'), G.SEEDS['hub'])
    return prob, [KEY + 13 * c for c in range(chains)], [_random_start(prob, 40 + c) for c in range(chains)]


# ------------------------------------------------------------------ 1: restatement
WORKLOADS = {
    'queen13x17': lambda chains: _lattice(13, 17, chains, 6),
    'queen30x40': lambda chains: _workload_a(chains),
    'weighted300': lambda chains: (lambda pr: (pr[0], [KEY], [pr[1]]))(_problem_from_golden('ref_graph300_weighted')),
    'generic': lambda chains: _workload_g(),
    'rsr40': lambda chains: _rsr_problem(40),
    'hub': lambda chains: _hub(chains),   # true SELL bases (ell_w = 0): the sums rebuild a CSR from sell_ptr as it comes back
}
CASES = [('queen13x17', 1), ('queen30x40', 1), ('queen30x40', 2), ('queen30x40', 4), ('weighted300', 1), ('generic', 1), ('rsr40', 2),
         ('hub', 2)]


@pytest.mark.parametrize('name, chains', CASES)
def test_rows_equal_their_restatement_in_numpy(name, chains):
    """Twelve iterations as twelve run(1, 0) calls.  After each: beta, eta, the new z and the iteration are read back, u is
    re-drawn with occ_draw(uniform, key, it, 14, n), and the eight columns are formed in numpy from Q.  No site has
    |u - psi| < 1e-12 (asserted), so z* is equal; the real-valued terms agree to about 1e-14, so a site's quantised term differs by
    at most one unit and a column by at most n.  Moran's I from the device's row and from numpy agree within 1e-9.  The same
    twelve iterations as one run(12, 0) give equal rows."""
    from occuspytial_amd._engine import device_draw
    prob, keys, starts = WORKLOADS[name](chains)
    W, d, S0 = _weights(prob)
    n = prob.n
    eng = _engine(prob, keys, starts)
    assert eng.get('moran_stats')[0] == 1.0
    stepped = [[] for _ in keys]
    worst = worst_i = 0
    for _ in range(12):
        eng.run(1, 0)
        for c, key in enumerate(keys):
            row = eng.moran_draws(c)
            assert row.shape == (1, 8)
            it = int(eng.get('iter', c)) - 1
            u = device_draw('uniform', n=n, key=key, it=it, stream=STREAM_SPATIAL)
            want, real, margin = _columns(prob, W, d, eng.get('beta', c), eng.get('eta', c), eng.get('z', c), u)
            assert margin >= 1e-12
            got = [int(v * Q32) for v in row[0]]
            assert all(row[0, k] * Q32 == got[k] for k in range(8))                 # (whole quanta)
            diff = max(abs(g - w) for g, w in zip(got, want))
            worst = max(worst, diff)
            assert diff <= n, (name, c, got, want)
            assert row[0, 3] > 0 and row[0, 7] > 0
            for half in (0, 4):
                i_dev, i_np = _moran(row[0, half:half + 4], n, S0), _moran(real[half:half + 4], n, S0)
                worst_i = max(worst_i, abs(i_dev - i_np))
                assert abs(i_dev - i_np) < 1e-9 and abs(i_dev) < 2.0, (name, c, half, i_dev, i_np)
            stepped[c].append(row[0])
    print(name, chains, 'largest difference from numpy: %d quanta of 2^-32, %.2e in I' % (worst, worst_i))
    eng.close()
    one = _engine(prob, keys, starts)
    one.run(12, 0)
    _same(_rows(one), [np.stack(r) for r in stepped])
    one.close()
    assert all(np.ptp(np.stack(r), axis=0).all() for r in stepped)        # (every column moves)


# ------------------------------------------------------------------ 2: call splitting
def test_differently_split_calls_give_the_same_rows():
    prob, keys, starts = _workload_a(2)
    ref = _two_calls(prob, keys, starts)
    assert [r.shape for r in ref] == [(39, 8)] * 2
    _same(ref, _two_calls(prob, keys, starts, split=((5, 4), (28, 0), (3, 0), (7, 0))))
    _same(ref, _two_calls(prob, keys, starts, split=((5, 4), (1, 0), (37, 0))))     # (a call of one iteration)


# ------------------------------------------------------------------ 3: scheduling paths
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


@pytest.mark.parametrize('name', ['generic', 'rsr40', 'weighted300'])
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
    assert [r.shape for r in out['tiles']] == [(21, 8)] * 2
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
    assert [r.shape for r in both] == [(16, 8)] * 3


# ------------------------------------------------------------------ 4: nothing else sees the switch
@pytest.mark.parametrize('name', ['queen30x40', 'generic', 'rsr40'])
def test_nothing_else_sees_the_switch(name):
    """alpha, beta, tau, eta, z, the site_* and ll_* sums, region_draws and ppc_draws are the same bits with moran_stats on and
    off; occ_step leaves the record alone."""
    prob, keys, starts = WORKLOADS[name](2)
    ids = (np.arange(prob.n) % 7).astype(np.int64)
    engines = {}
    for which in ('on', 'off'):
        eng = engines[which] = _engine(prob, keys, starts, on=which == 'on', site=True, ll=True, ids=ids, ppc=True)
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
        assert on.moran_draws(c).shape == (10, 8)
    before = on.moran_draws(0).copy()
    on.step()                                                   # occ_step never counts: the last call's rows stay
    assert np.array_equal(on.moran_draws(0), before)
    for eng in engines.values():
        eng.close()


@pytest.mark.parametrize('site, ll, regions, ppc', [(s, l, r, p) for s in (False, True) for l in (False, True) for r in (False, True)
                                                    for p in (False, True)][1:])
def test_rows_are_the_same_beside_every_other_switch(site, ll, regions, ppc):
    prob, keys, starts = _workload_a(2)
    ids = (np.arange(prob.n) % 7).astype(np.int64) if regions else None
    split = ((12, 3), (5, 0))
    _same(_two_calls(prob, keys, starts, split=split), _two_calls(prob, keys, starts, split=split, site=site, ll=ll, ids=ids, ppc=ppc))


# ------------------------------------------------------------------ 5: windows
def test_windows_and_a_chain_that_does_not_count():
    """120 iterations, 100 kept, four chains of which the last has its switch off: exactly `keep` rows, length 0 for the chain
    that does not count, D and D* positive, |I| < 2 on the lattice for the residuals and their replicate."""
    prob, keys, starts = _workload_a(4)
    _, _, S0 = _weights(prob)
    eng = _engine(prob, keys, starts)
    eng.set('moran_stats', 0.0, 3)
    eng.run(120, 20)
    for c in range(3):
        rows = eng.moran_draws(c)
        assert rows.shape == (100, 8)
        assert np.all(rows[:, 3] > 0) and np.all(rows[:, 7] > 0)
        for half in (0, 4):
            assert np.all(np.abs(_moran(rows[:, half:half + 4].T, prob.n, S0)) < 2.0)
        assert np.all(np.ptp(rows, axis=0) > 0)
    assert eng.moran_draws(3).shape == (0, 8) and eng.get('moran_draws', 3).size == 0
    eng.close()


# ------------------------------------------------------------------ 6: refusals
@pytest.mark.parametrize('name', ['queen30x40', 'rsr40'])
def test_refusals(name):
    import ctypes
    prob, keys, starts = WORKLOADS[name](2)
    eng = _engine(prob, keys, starts, on=False)
    for nm in ('moran_stats', 'moran_draws'):
        with pytest.raises(ValueError, match='set moran_stats first'):
            eng.get(nm)
        v = np.zeros(8)
        n = ctypes.c_int64(0)
        assert eng._lib.occ_get_state(eng._h, 0, nm.encode(), v.ctypes.data, 8, ctypes.byref(n)) == -5     # OCC_E_STATE
    with pytest.raises(ValueError, match='set moran_stats first'):
        eng.set('moran_draws', np.zeros(8))
    for bad in (2.0, -1.0, 0.5, np.nan):
        with pytest.raises(ValueError, match='moran_stats is 0 or 1'):
            eng.set('moran_stats', bad)
        v = np.array([bad])
        assert eng._lib.occ_set_state(eng._h, 0, b'moran_stats', v.ctypes.data, 1) == -1                  # OCC_E_BADARG
    with pytest.raises(ValueError, match='wrong length'):
        eng.set('moran_stats', np.ones(2))
    eng.set('moran_stats', 0.0)                                         # (off before it was ever on: accepted, nothing allocated)
    with pytest.raises(ValueError, match='set moran_stats first'):      # (nothing of the refused values was kept)
        eng.get('moran_stats')
    eng.set('moran_stats', 1.0, 1)
    assert [eng.get('moran_stats', c)[0] for c in (0, 1)] == [0.0, 1.0] and eng.get('moran_draws', 1).size == 0
    with pytest.raises(ValueError, match='read-only'):
        eng.set('moran_draws', np.zeros(8))
    eng.set_start(1, **starts[1])                                      # occ_set_start and occ_set_keys do not touch the switch
    eng.set_keys(keys)
    assert eng.get('moran_stats', 1)[0] == 1.0
    eng.run(3, 1)
    assert eng.moran_draws(0).shape == (0, 8) and eng.moran_draws(1).shape == (2, 8)
    eng.set('moran_stats', 0.0, 1)
    eng.run(3, 1)
    assert eng.moran_draws(1).shape == (0, 8) and eng.get('moran_stats', 1)[0] == 0.0      # (still answered: it has been on)
    eng.close()


def test_probit_handle_refuses():
    from .test_gpu_regions import _probit_problem
    from occuspytial_amd._engine import Engine
    prob, keys, starts = _probit_problem(2)
    eng = Engine(prob, keys)
    for nm in ('moran_stats', 'moran_draws'):
        with pytest.raises(ValueError, match='the spatial residual check is not available for the probit model'):
            eng.get(nm)
    with pytest.raises(ValueError, match='the spatial residual check is not available for the probit model'):
        eng.set('moran_stats', 1.0)
    v = np.ones(1)
    assert eng._lib.occ_set_state(eng._h, 0, b'moran_stats', v.ctypes.data, 1) == -5                       # OCC_E_STATE
    eng.close()


def test_a_precision_with_a_positive_off_diagonal_is_refused():
    """The dense prior form admits any singular positive semi-definite Q; Q^2 of a lattice has positive off-diagonals (the
    two-step neighbours).  The switch answers OCC_E_BADARG and stays unset; the handle samples as before."""
    from occuspytial_amd._engine import Engine
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(6, 7, visits=3, p=2, q=2, random_state=3)
    Q2 = sparse.csr_matrix(Q @ Q)
    assert (Q2 - sparse.diags(Q2.diagonal())).max() > 0
    prob = FlatProblem(Q2, W, X, y, prior_draw='dense')
    eng = Engine(prob, [KEY])
    eng.set_start(0, **_random_start(prob, 5))
    with pytest.raises(ValueError, match='every off-diagonal of Q'):
        eng.set('moran_stats', 1.0)
    v = np.ones(1)
    assert eng._lib.occ_set_state(eng._h, 0, b'moran_stats', v.ctypes.data, 1) == -1                       # OCC_E_BADARG
    with pytest.raises(ValueError, match='set moran_stats first'):
        eng.get('moran_stats')
    a, b, t = eng.run(4, 1)
    assert a.shape == (1, 3, 2) and np.all(np.isfinite(t))
    eng.close()


# ------------------------------------------------------------------ 7: checkpoint and sampler
def test_checkpoint_and_restore_carry_the_switch():
    prob, keys, starts = _workload_a(2)
    e1 = _engine(prob, keys, starts)
    e1.run(20, 5)
    ck = e1.checkpoint()
    assert ck['moran_stats'].tolist() == [1.0, 1.0] and 'moran_draws' not in ck
    e1.close()
    e2 = _engine(prob, keys, starts, on=False)           # a fresh engine that never heard of the check
    assert 'moran_stats' not in e2.checkpoint()
    e2.restore(ck)
    assert e2.get('moran_stats', 1)[0] == 1.0
    assert e2.moran_draws(0).shape == (0, 8)             # the draws belong to a call and are not carried
    e2.run(15, 0)
    e3 = _engine(prob, keys, starts)
    e3.run(20, 5)
    e3.run(15, 0)
    _same(_rows(e2), _rows(e3))
    e2.close()
    e3.close()


def test_engine_group_switches_everywhere_and_routes_by_chain():
    from occuspytial_amd._engine import Engine, EngineGroup
    prob, keys, starts = _workload_a(3)
    grp = EngineGroup(prob, keys, [0, 0], engine_factory=lambda pr, ks, dev: Engine(pr, ks, device=dev))
    for c in range(3):
        grp.set_start(c, **starts[c])
    grp.moran_stats(True)
    assert grp._moran_on
    grp.run(20, 5)
    first = [grp.moran_draws(c) for c in range(3)]
    ck = grp.checkpoint()
    assert ck['moran_stats'].tolist() == [1.0] * 3 and 'moran_draws' not in ck
    grp.restore(ck)
    grp.run(10, 0)
    got = [np.concatenate([a, grp.moran_draws(c)]) for c, a in enumerate(first)]
    grp.close()
    _same(_two_calls(prob, keys, starts, split=((20, 5), (10, 0))), got)


def _sampler(cls_name='LogitICARGibbs', **kw):
    import occuspytial_amd
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(30, 40, visits=3, p=2, q=2, random_state=2)
    return getattr(occuspytial_amd, cls_name)(Q, W, X, y, random_state=7, **kw)


@pytest.mark.parametrize('cls_name, kw', [('LogitICARGibbs', {}), ('LogitRSRGibbs', dict(q=40))])
def test_sampler_returns_the_check_of_the_kept_draws(cls_name, kw):
    from occuspytial_amd.spatial import SpatialCheck
    s = _sampler(cls_name, **kw)
    chunked = s.sample(60, burnin=20, chains=3, progressbar=True, spatial_check=True)   # chunks of 16: one straddles the burn-in
    one = _sampler(cls_name, **kw).sample(60, burnin=20, chains=3, progressbar=False, spatial_check=True)
    plain = _sampler(cls_name, **kw).sample(60, burnin=20, chains=3, progressbar=False)
    assert plain.spatial_check is None and isinstance(one.spatial_check, SpatialCheck)
    assert sorted(one.data) == sorted(plain.data)                              # (post.summary and the chains are unchanged)
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(one[name], plain[name]) and np.array_equal(chunked[name], plain[name])
    for name in ('moran_obs', 'moran_rep'):
        assert getattr(one.spatial_check, name).shape == (3, 40)
        assert np.array_equal(getattr(one.spatial_check, name), getattr(chunked.spatial_check, name)), name
    sc = one.spatial_check
    assert sc.n == 1200 and sc.n_draws == 120 and sc.expected == -1.0 / 1199
    assert 0.0 <= sc.p_value <= 1.0 and abs(sc.excess) < 2.0 and 'p_value' in repr(sc)
    # resume: the rows of the new draws are the tail of an uninterrupted run's
    ck = s.checkpoint()
    assert 'moran_stats' in ck
    more = s.resume(ck, 30, progressbar=False, spatial_check=True)
    longer = _sampler(cls_name, **kw).sample(90, burnin=20, chains=3, progressbar=False, spatial_check=True)
    assert np.array_equal(more.spatial_check.moran_obs, longer.spatial_check.moran_obs[:, 40:])
    assert np.array_equal(more.spatial_check.moran_rep, longer.spatial_check.moran_rep[:, 40:])
    assert np.array_equal(more['alpha'], longer['alpha'][:, 40:])
    again = s.resume(ck, 5, progressbar=False)                                 # (not asked for: the checkpoint's switch goes off)
    assert again.spatial_check is None and not s._engine._moran_on


# ------------------------------------------------------------------ 8: one decision that must come out right
CPU_P_VALUE = dict(A=(0.333, 0.312, 0.300), B=(0.000, 0.000, 0.000))   # oracle keys 1 to 3 (see the test's docstring)
CPU_MEAN_I = dict(A=0.011, B=0.115)


def _decision_data():
    """20x20 queen lattice, sites row-major; a mid-frequency occupancy pattern f of amplitude 2.5 as the third covariate."""
    from occuspytial_amd.utils import get_generator, rand_precision_mat
    n = 400
    Q = rand_precision_mat(20, 20)
    rng = get_generator(2)
    row, col = np.divmod(np.arange(n), 20)
    f = np.sin(2 * np.pi * 3 * row / 20) * np.sin(2 * np.pi * 3 * col / 20)
    X = np.column_stack([np.ones(n), rng.uniform(-2, 2, n), f])
    beta, alpha = np.array([0.0, 0.7, 2.5]), np.array([0.3, 0.5])
    z = rng.binomial(1, expit(X @ beta))
    W, y = {}, {}
    for i in range(n):
        w = rng.uniform(-2, 2, (4, 2))
        w[:, 0] = 1
        W[i] = w
        y[i] = rng.binomial(1, z[i] * expit(w @ alpha))
    return Q, W, X, y


def test_the_check_accepts_the_model_with_the_pattern_and_rejects_the_one_without():
    """Both models are LogitRSRGibbs(q=2); A gets all three columns of X, B the first two, so B's residuals keep the pattern.
    600 iterations, 200 discarded, three chains, start alpha = beta = theta = 0 and tau = 1.  Conditions: A's p_value inside
    (0.1, 0.9), B's below 0.05, excess(B) > excess(A).
    On the CPU (the oracle's chains, keys 1 to 3, numpy's replicate uniforms): A p_value 0.333, 0.312, 0.300, mean I_obs 0.011;
    B p_value 0.000, 0.000, 0.000, mean I_obs 0.115.
    On the device (one MI355X, three chains): A p_value 0.355, 0.323, 0.263 (pooled 0.313), mean I_obs 0.0108, excess 0.0125;
    B p_value 0.000, 0.000, 0.000, mean I_obs 0.1154, excess 0.1174."""
    from occuspytial_amd import LogitRSRGibbs
    Q, W, X, y = _decision_data()
    out = {}
    for name, cols in (('A', 3), ('B', 2)):
        start = dict(alpha=np.zeros(2), beta=np.zeros(cols), tau=1.0, eta=np.zeros(2))
        post = LogitRSRGibbs(Q, W, X[:, :cols], y, random_state=5, q=2).sample(600, burnin=200, chains=3, start=start, progressbar=False,
                                                                               spatial_check=True)
        sc = out[name] = post.spatial_check
        print('model', name, sc, 'mean I_obs %.4f, mean I_rep %.4f' % (sc.moran_obs.mean(), sc.moran_rep.mean()),
              'per chain p:', [round(float(np.mean(sc.moran_rep[c] > sc.moran_obs[c])), 3) for c in range(3)],
              '| on the CPU: p_value', CPU_P_VALUE[name], 'mean I_obs', CPU_MEAN_I[name])
        assert sc.n_draws == 1200
    assert 0.1 < out['A'].p_value < 0.9
    assert out['B'].p_value < 0.05
    assert out['B'].excess > out['A'].excess
