"""Held-out predictive scoring, accumulated on the device (state names ``holdout_data``, ``holdout_stats``, ``holdout_count``,
``holdout_sums``; csrc/occ_holdout.hpp).

Per iteration past a call's burn-in one kernel behind the z update adds, per held-out entry of a chain whose switch is on, five
float64 slots: the count, the marginal likelihood L of the entry's withheld detection history under the iteration's alpha, beta
and eta, l = log L, l^2 and pd, the predictive probability of at least one detection.  A column belongs to one thread and
additions run in iteration order, so every comparison between two ways of running the engine is equality of bits.  The
comparison with numpy has the bounds of tests/test_gpu_waic.py (docstring of ``test_sums_equal_their_restatement_in_numpy``).  The held-out sites are NOT
surveyed in the engine's problem: every workload here takes sites out of a generated problem (or uses the sites a fixture
leaves unsurveyed) and gives them withheld visits of ragged lengths.  Every test runs under its own time limit.
"""
import ctypes

import numpy as np
import pytest
from scipy import sparse
from scipy.special import expit

from . import _z_theory as zt
from ._outputs_gpu import engine_with, time_limit as _time_limit, two_calls  # noqa: F401 (autouse in this module)
from .conftest import load_golden
from .test_gpu_parity import KEY, _random_start
from .test_gpu_ppc import SCHED_KEYS

pytestmark = pytest.mark.gpu
CNT, LIK, LOG, LOG2, PD = range(5)


# ------------------------------------------------------------------ workloads
def _visits(rng, sites, q, lengths=None, p_detect=0.3):
    """Withheld visits for ``sites``: W rows with a leading 1 and uniform(-2, 2) covariates, y ~ Bernoulli(p_detect) per row;
    ``lengths[k]`` rows for the k-th site (default: 1 to 6, ragged)."""
    W, y = {}, {}
    for k, s in enumerate(sites):
        v = int(lengths[k]) if lengths is not None and k < len(lengths) and lengths[k] else int(rng.integers(1, 7))
        w = rng.uniform(-2, 2, size=(v, q))
        w[:, 0] = 1.0
        W[int(s)], y[int(s)] = w, rng.binomial(1, p_detect, size=v)
    return W, y


def _lattice(rows, cols, held, chains, seed, visits=3, p=2, q=2, lengths=None, rsr=0):
    """A lattice problem of make_lattice_problem with the sites ``held`` taken out of W and y, and withheld visits for them."""
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(rows, cols, visits=visits, p=p, q=q, random_state=seed)
    for s in held:
        del W[int(s)], y[int(s)]
    prob = FlatProblem(Q, W, X, y)
    assert sorted(prob.not_surveyed) == sorted(int(s) for s in held)
    rng = np.random.default_rng(1000 + seed)
    Wt, yt = _visits(rng, held, q, lengths)
    if rsr:
        m = prob.enable_rsr(q=rsr)['dim']
        starts = [dict(alpha=rng.standard_normal(q), beta=rng.standard_normal(p), tau=1.0 + c, eta=rng.standard_normal(m)) for c in range(chains)]
    else:
        starts = [_random_start(prob, 40 + c) for c in range(chains)]
        if p > 2:   # (the generic kernels: moderate predictors, as tests/test_gpu_site_summaries.py starts them)
            for st in starts:
                st['alpha'], st['beta'] = 0.3 * st['alpha'], 0.3 * st['beta']
    return prob, [KEY + 13 * c for c in range(chains)], starts, Wt, yt


def _queen13x17(chains, held=None):
    n = 13 * 17
    held = sorted(set([0, n - 1] + list(range(2, n - 1, 3)))) if held is None else held     # the first and the last site; 75 entries
    return _lattice(13, 17, held, chains, 6, lengths=[1, 40])                                # one row, forty rows, then 1 to 6


def _weighted300(chains):
    """The weighted 300-node graph fixture (tests/test_gpu_parity.py's ``_problem_from_golden``) with every third site taken out
    of its W and y and held out."""
    from occuspytial_amd._problem import FlatProblem
    g = load_golden('ref_graph300_weighted')
    n = g['X'].shape[0]
    Q = sparse.csr_matrix((g['Q_data'], g['Q_indices'], g['Q_indptr']), shape=(n, n))
    W, y, cur = {}, {}, 0
    for s, v in zip(g['sites'], g['visits']):
        W[int(s)], y[int(s)] = g['W_flat'][cur:cur + v], g['y_flat'][cur:cur + v]
        cur += v
    held = sorted(W)[::3]
    for s in held:
        del W[s], y[s]
    hp = {k[3:]: g[k] for k in g if k.startswith('hp_')} or None
    prob = FlatProblem(Q, W, g['X'], y, hp)
    start = dict(alpha=g['start_alpha'], beta=g['start_beta'], tau=float(g['start_tau']), eta=g['start_eta'])
    Wt, yt = _visits(np.random.default_rng(77), held, prob.q)
    return prob, [KEY], [start], Wt, yt


WORKLOADS = {
    'queen13x17': _queen13x17,                                                               # 75 entries: one partial workgroup
    'single': lambda chains: _queen13x17(chains, held=[57]),                                 # H = 1
    'queen30x40': lambda chains: _lattice(30, 40, list(range(1, 1200, 4)), chains, 2, lengths=[3, 1, 37]),   # 300 entries: two workgroups
    'weighted300': _weighted300,
    'generic': lambda chains: _lattice(17, 19, list(range(0, 323, 5)), 1, 18, visits=6, p=9, q=9),          # p = q = 9
    'rsr40': lambda chains: _lattice(24, 30, list(range(3, 720, 4)), 2, 4, rsr=40),
}


def _workload_a(chains=2):
    return WORKLOADS['queen30x40'](chains)


# ------------------------------------------------------------------ helpers
def _engine(prob, keys, starts, Wt, yt, on=True, **kw):
    return engine_with(prob, keys, starts, holdout=(Wt, yt) if on else None, **kw)


def _sums(eng):
    return [eng.holdout_sums(c) for c in range(eng.n_chains)]


def _two_calls(work, split=((33, 4), (10, 0)), **kw):
    """run(33, 4) then run(10, 0) -> per chain the sums of the 39 iterations past the calls' burn-in."""
    return two_calls(lambda: _engine(*work, **kw), _sums, split)


def _same(a, b):
    assert len(a) == len(b)
    for c, (u, v) in enumerate(zip(a, b)):
        assert u['count'] == v['count'], (c, u['count'], v['count'])
        assert u['sums'].dtype == np.float64 and u['sums'].shape == v['sums'].shape and u['sums'].shape[0] == 5
        assert np.array_equal(u['sums'], v['sums']), (c, np.count_nonzero(u['sums'] != v['sums']))


def _whole(sums, count):
    """Every chain counted `count` iterations, so did every entry; L and pd are probabilities, l a log-probability."""
    for s in sums:
        g = s['sums']
        assert s['count'] == count and np.all(g[CNT] == count) and np.all(np.isfinite(g))
        assert np.all(g[LIK] >= 0) and np.all(g[LIK] <= count * (1 + 1e-12)) and np.all(g[LOG] <= 0)
        assert np.all(g[PD] >= 0) and np.all(g[PD] <= count * (1 + 1e-12))


def lsig(a):
    """log expit(a), stable on both sides."""
    return np.minimum(a, 0.0) - np.log1p(np.exp(-np.abs(a)))


def holdout_terms(X, data, alpha, beta, eta):
    """l, L and pd of every held-out entry from the table of the header (include/occ_gibbs.h), in numpy, and beside them the
    sizes ``b`` and ``bp`` that the rounding bounds of l and of pd are proportional to (docstring of ``test_sums_equal_their_restatement_in_numpy``).
    ``data``: (site, ptr, y, W) as occuspytial_amd.holdout.unpack returns them."""
    site, ptr, y, W = data
    H = site.size
    a0 = X[site] @ beta + eta[site]
    a0_abs = np.abs(X[site] * beta).sum(axis=1) + np.abs(eta[site])
    wa = W @ alpha
    wa_abs = np.abs(W * alpha).sum(axis=1)
    ll, lik, pd, b, bp = (np.zeros(H) for _ in range(5))
    ref = zt.problem_terms(X, eta, beta, W, alpha, ptr, site)           # as if no entry had a detection
    for h in range(H):
        rows = slice(ptr[h], ptr[h + 1])
        psi = expit(a0[h])
        P = np.prod(expit(-wa[rows]))
        pd[h] = psi * (1.0 - P)
        bp[h] = (a0_abs[h] + 1.0) + np.sum(wa_abs[rows] + 1.0)
        if y[rows].any():
            t0 = lsig(a0[h])
            terms = lsig(np.where(y[rows] != 0, wa[rows], -wa[rows]))
            acc = t0
            for t in terms:                                           # rows in row order
                acc = acc + t
            ll[h], lik[h] = acc, np.exp(acc)
            b[h] = (a0_abs[h] + abs(t0) + 1.0) + np.sum(wa_abs[rows] + np.abs(terms) + 1.0)
        else:
            ll[h], lik[h] = ref['l'][h], ref['D'][h]                   # log space: nothing is subtracted (tests/_z_theory.py)
            b[h] = ref['b'][h] + abs(ll[h])                            # (sum |products_0| + 1) + sum_r (sum |products_r| + 1) + |l|
    return ll, lik, pd, b, bp


def host_sums(eng, prob, data, steps, advance):
    """``steps`` x advance(eng, t); after each, alpha, beta and eta of every chain are read and the terms accumulated on the host,
    with the bounds' sizes beside them.  Works on any engine (the device's or the CPU restatement of the ABI)."""
    C, H = eng.n_chains, data[0].size
    acc = [{k: np.zeros(H) for k in ('lik', 'log', 'log2', 'pd', 'b', 'bp', 'maxabs')} for _ in range(C)]
    for t in range(steps):
        advance(eng, t)
        for c in range(C):
            alpha, beta, eta = (eng.get(name, c) for name in ('alpha', 'beta', 'eta'))
            ll, lik, pd, b, bp = holdout_terms(prob.X, data, alpha, beta, eta)
            a = acc[c]
            a['lik'] += lik
            a['log'] += ll
            a['log2'] += ll * ll
            a['pd'] += pd
            a['b'] += b
            a['bp'] += bp
            a['maxabs'] = np.maximum(a['maxabs'], np.abs(ll))
            yield t, c, a


# ------------------------------------------------------------------ 1: restatement
CASES = [('queen13x17', 1), ('queen13x17', 2), ('queen13x17', 4), ('single', 2), ('queen30x40', 2), ('weighted300', 1), ('generic', 1),
         ('rsr40', 2)]
CAP = 1e-6


@pytest.mark.parametrize('name, chains', CASES)
def test_sums_equal_their_restatement_in_numpy(name, chains):
    """Thirteen iterations, alternately as run(1, 0) and as occ_step.  After each, alpha, beta and eta of every chain are read
    back, l, L and pd are restated in numpy (``holdout_terms``) and all five slots are compared.  u = 2^-53.  ``cnt`` and
    ``count`` are exact.  The bounds are those of tests/test_gpu_waic.py's ``_restatement``, taken over the withheld rows:

    A detection in the withheld history.  l = lsig(a_0) + sum_r lsig(a_r), a_0 = x_i beta + eta_i, a_r = +- w_r alpha.  Host and
      device form each dot product in their own order: they differ by at most 2 (q + 1) u sum |products| (2.2e-15 sum |products|
      for q <= 9).  lsig has slope <= 1, so the term inherits that; its own evaluation adds at most 4 u (|term| + 1).  Adding the
      <= 41 terms and then 13 iterations rounds at most (41 + 13) u sum |terms| = 6e-15 sum |terms|.  Held to
      B_l = 1e-12 sum_t sum_terms (sum |products| + |term| + 1), a margin of more than a hundred.
    No detection.  l = log D, D = (1 - psi) + psi prod_r expit(-w_r alpha), on the host in log space (tests/_z_theory.py): both
      terms of D are positive and each has the relative error of its logarithm, |d a_0| and |d a_0| + sum_r (|d a_r| + 4 u); the
      device takes 1 - psi without cancellation, so no 1 / (1 - psi) enters.  Held to
      B_l = 1e-12 sum_t ((sum |products_0| + 1) + sum_r (sum |products_r| + 1) + |l|), as tests/test_gpu_waic.py.
    sum L: L <= 1 and d L = L d l or D d l: the same absolute bound B_l.
    sum l^2: 2 max_t |l_t| B_l + 1e-12 sum l^2 (the fused multiply-adds round 13 times at u sum l^2).
    sum pd: pd = psi (1 - P), P = prod_r expit(-w_r alpha) <= 1.  |d psi| <= |d a_0| / 4 + 4 u, |d P| <= P sum_r (|d a_r| + 4 u),
      the product and the difference round at 2 u: |d pd| <= (p + 1) u sum |products_0| + 10 u + sum_r (2 (q + 1) u
      sum |products_r| + 4 u); held to B_pd = 1e-12 sum_t ((sum |products_0| + 1) + sum_r (sum |products_r| + 1)).
    ``CAP``: B_l must stay below 1e-6, as when it grew as 1 / (1 - psi), at every entry, so that it cannot grow until it hides a
    failure: an error in a sign, a row or a term moves l by more than 1e-3.
    The same thirteen iterations as one run(13, 0) give equal bits."""
    from occuspytial_amd.holdout import holdout_arg, unpack
    work = WORKLOADS[name](chains)
    prob, keys = work[0], work[1]
    data = unpack(holdout_arg(work[3:], prob), prob.q)
    H, C = data[0].size, len(keys)
    lengths = np.diff(data[1])
    seen = np.add.reduceat(data[2], data[1][:-1]) > 0
    if name in ('queen13x17', 'queen30x40'):
        assert lengths.min() == 1 and lengths.max() >= 37 and seen[:64].any() and not seen[:64].all()   # ragged, both kinds in a wave
    if name == 'queen13x17':
        assert data[0][0] == 0 and data[0][-1] == prob.n - 1 and H % 64 != 0
    if name == 'queen30x40':
        assert H > 256 and H % 256 != 0
    if name == 'single':
        assert H == 1
    eng = _engine(*work)
    assert [eng.get('holdout_stats', c)[0] for c in range(C)] == [1.0] * C
    assert np.array_equal(eng.get('holdout_data', C - 1), holdout_arg(work[3:], prob))
    worst = dict(log=0.0, lik=0.0, log2=0.0, pd=0.0, bound=0.0)
    for t, c, a in host_sums(eng, prob, data, 13, lambda e, t: e.run(1, 0) if t % 2 == 0 else e.step()):
        N = t + 1
        got = eng.holdout_sums(c)
        g = got['sums']
        assert got['count'] == N and g.shape == (5, H) and np.all(g[CNT] == N)
        B = 1e-12 * a['b']
        B2 = 2.0 * a['maxabs'] * B + 1e-12 * a['log2']
        Bp = 1e-12 * a['bp']
        fig = dict(log=np.max(np.abs(g[LOG] - a['log']) / B), lik=np.max(np.abs(g[LIK] - a['lik']) / B),
                   log2=np.max(np.abs(g[LOG2] - a['log2']) / B2), pd=np.max(np.abs(g[PD] - a['pd']) / Bp), bound=B.max())
        for k, v in fig.items():
            worst[k] = max(worst[k], float(v))
        assert B.max() < CAP, (name, c, t, fig)
        assert fig['log'] <= 1.0 and fig['lik'] <= 1.0 and fig['log2'] <= 1.0 and fig['pd'] <= 1.0, (name, c, t, fig)
    print(name, chains, 'largest found / bound:', worst)
    stepped = _sums(eng)
    eng.close()
    _whole(stepped, 13)
    for s in stepped:
        assert np.all(s['sums'][LIK] > 0) and np.all(s['sums'][LOG] < 0) and np.all(s['sums'][PD] > 0)
    one = _engine(*work)
    one.run(13, 0)
    _same(_sums(one), stepped)
    one.close()


# ------------------------------------------------------------------ 2: extremes
def test_a_likelihood_that_underflows_stays_finite_in_its_logarithm():
    """A large alpha set through occ_set_state -- the next alpha is drawn afresh from Polya-Gamma variates of it and falls back
    within a few iterations (the CPU restatement of the ABI: |alpha| of 10, 3, 1.4, 0.6 after the first four), so the withheld
    rows' second covariate is also 2000 times the usual: |w_r alpha| stays in the hundreds and thousands.  Four iterations.  At
    detection entries whose l lies below -745.2 in every one of them -- judged by the restatement from the states read back --
    sum L is exactly 0 while sum l is finite; there is at least one such entry (on the CPU: 33 and 14 of the 44 detection entries).  At every entry: nothing is NaN, 0 <= sum L <= N, sum l <= 0, 0 <= sum pd <= N, Jensen
    (log(sum L / N) >= sum l / N) and Cauchy-Schwarz ((sum l)^2 <= N sum l^2), each up to the rounding of sums of N terms, held to
    1e-12 as in tests/test_gpu_waic.py."""
    from occuspytial_amd.holdout import holdout_arg, unpack
    prob, keys, starts, Wt, yt = _queen13x17(2)
    for s in Wt:
        Wt[s] = Wt[s].copy()
        Wt[s][:, 1] *= 2000.0
    data = unpack(holdout_arg((Wt, yt), prob), prob.q)
    seen = np.add.reduceat(data[2], data[1][:-1]) > 0
    eng = _engine(prob, keys, starts, Wt, yt)
    for c in range(2):
        eng.set('alpha', np.array([30.0, -40.0]), c)
    N = 4
    under = np.ones((2, data[0].size), dtype=bool)
    for t, c, a in host_sums(eng, prob, data, N, lambda e, t: e.step()):
        alpha, beta, eta = (eng.get(name, c) for name in ('alpha', 'beta', 'eta'))
        under[c] &= holdout_terms(prob.X, data, alpha, beta, eta)[0] < -745.2
    got = _sums(eng)
    eng.close()
    print('entries whose likelihood underflows in every iteration:', under.sum(axis=1), 'of', data[0].size)
    assert (under & seen).any()
    for c, s in enumerate(got):
        g = s['sums']
        assert s['count'] == N and np.all(g[CNT] == N) and not np.isnan(g).any() and np.all(np.isfinite(g[LOG])) and np.all(np.isfinite(g[LOG2]))
        assert np.all(g[LIK][under[c] & seen] == 0.0)
        assert np.all(g[LIK] >= 0) and np.all(g[LIK] <= N * (1 + 1e-12)) and np.all(g[LOG] <= 0)
        assert np.all(g[PD] >= 0) and np.all(g[PD] <= N * (1 + 1e-12))
        with np.errstate(divide='ignore'):
            gap = np.log(g[LIK] / N) - g[LOG] / N
        pos = g[LIK] > 0
        assert np.all(gap[pos] >= -1e-12 * (1.0 + np.abs(g[LOG][pos]) / N))
        assert np.all(N * g[LOG2] >= g[LOG] ** 2 * (1 - 1e-12))


# ------------------------------------------------------------------ 3: bit-equal sums whatever the path
@pytest.fixture(scope='module')
def ref_a():
    """Workload A (30x40, 300 entries), two chains, run(33, 4) then run(10, 0), on the default path: computed once, never changed."""
    ref = _two_calls(_workload_a(2))
    _whole(ref, 39)
    for s in ref:
        s['sums'].setflags(write=False)
    return ref


def test_differently_split_calls_give_the_same_sums(ref_a):
    _same(ref_a, _two_calls(_workload_a(2), split=((5, 4), (28, 0), (3, 0), (7, 0))))
    _same(ref_a, _two_calls(_workload_a(2), split=((5, 4), (1, 0), (37, 0))))            # (a call of one iteration)


def test_occ_step_counts():
    """occ_step's window has burn-in 0: eager steps count like the iterations of a replayed graph, also between two runs."""
    eng = _engine(*_workload_a(2))
    eng.run(4, 4 - 1)                 # (the three iterations of burn-in are not counted, the fourth is)
    for _ in range(9):
        eng.step()
    eng.run(29, 0)
    got = _sums(eng)
    eng.close()
    _whole(got, 39)
    _same(got, _two_calls(_workload_a(2), split=((4, 3), (38, 0))))


@pytest.mark.parametrize('env', [{'OCC_EVENT_SYNC': '1'}, {'OCC_EVENT_SYNC': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_CU_SPLIT': '0'},
                                 {'OCC_DEBUG_STREAMS_SERIALISED': '1'},
                                 {'OCC_NO_SIDE_STREAM': '1'}, {'OCC_EAGER_ONLY': '1'}, {'OCC_NO_XCD_LOCAL': '1'},
                                 {'OCC_NO_XCD_LOCAL': '1', 'OCC_CU_SPLIT': '0'},
                                 {'OCC_NO_PERSISTENT': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_NO_PERSISTENT': '1', 'OCC_NO_SIDE_STREAM': '1'}])
def test_every_scheduling_mode_gives_the_same_sums(monkeypatch, env):
    """Graph replay against eager stepping (OCC_EAGER_ONLY) and every other way of scheduling an iteration: the scheduling
    environments of tests/test_gpu_convergence.py."""
    for k in SCHED_KEYS:
        monkeypatch.delenv(k, raising=False)
    ref = _two_calls(_workload_a(2))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _same(ref, _two_calls(_workload_a(2)))


@pytest.mark.parametrize('name', ['generic', 'rsr40', 'weighted300'])
def test_graph_replay_equals_eager_stepping_on_the_other_kernels(monkeypatch, name):
    monkeypatch.delenv('OCC_EAGER_ONLY', raising=False)
    ref = _two_calls(WORKLOADS[name](2))
    _whole(ref, 39)
    monkeypatch.setenv('OCC_EAGER_ONLY', '1')
    _same(ref, _two_calls(WORKLOADS[name](2)))


def test_tile_looping_kernel_gives_the_sums_of_launch_per_step(monkeypatch):
    work = _lattice(61, 67, list(range(0, 61 * 67, 5)), 2, 5)
    monkeypatch.setenv('OCC_FORCE_TILES', '1')
    out = {}
    for mode in ('tiles', 'launch_per_step'):
        monkeypatch.delenv('OCC_NO_PERSISTENT', raising=False)
        if mode == 'launch_per_step':
            monkeypatch.setenv('OCC_NO_PERSISTENT', '1')
        eng = _engine(*work)
        assert eng.stats()['persistent_solve'] == (3 if mode == 'tiles' else 0)
        eng.run(24, 3)
        out[mode] = _sums(eng)
        assert eng.stats()['fused_fallbacks'] == 0
        eng.close()
    _whole(out['tiles'], 21)
    _same(out['tiles'], out['launch_per_step'])


def test_batched_chains_have_the_sums_of_single_chain_runs():
    prob, _, _, Wt, yt = _weighted300(1)
    keys = [KEY, KEY ^ 0xABCDEF, 12345]
    rng = np.random.default_rng(3)
    starts = [dict(alpha=rng.standard_normal(prob.q), beta=rng.standard_normal(prob.p), tau=1.0 + c,
                   eta=(lambda e: e - e.mean())(rng.standard_normal(prob.n))) for c in range(3)]
    batch = _engine(prob, keys, starts, Wt, yt)
    batch.run(20, 4)
    both = _sums(batch)
    batch.close()
    _whole(both, 16)
    for c in range(3):
        solo = _engine(prob, [keys[c]], [starts[c]], Wt, yt)
        solo.run(20, 4)
        _same([both[c]], _sums(solo))
        solo.close()


def test_engine_group_switches_everywhere_and_routes_by_chain():
    from occuspytial_amd._engine import Engine, EngineGroup
    prob, keys, starts, Wt, yt = _workload_a(3)
    grp = EngineGroup(prob, keys, [0, 0], engine_factory=lambda pr, ks, dev: Engine(pr, ks, device=dev))
    for c in range(3):
        grp.set_start(c, **starts[c])
    assert grp._holdout is None and not grp._holdout_on
    grp.holdout_data(Wt, yt)
    grp.holdout_stats(True)
    assert grp._holdout_on and grp._holdout.size == grp.get('holdout_data', 2).size
    grp.run(20, 5)
    ck = grp.checkpoint()
    assert ck['holdout_stats'].tolist() == [1.0] * 3 and ck['holdout_count'].tolist() == [15] * 3
    assert ck['holdout_sums'].shape == (3, 5, 300) and ck['holdout_sums'].dtype == np.float64 and ck['holdout_data'].shape[0] == 3
    grp.restore(ck)
    grp.run(10, 0)
    got = [grp.holdout_sums(c) for c in range(3)]
    grp.close()
    _same(_two_calls((prob, keys, starts, Wt, yt), split=((20, 5), (10, 0))), got)


# ------------------------------------------------------------------ 4: a re-run call counts nothing twice
def _headline_sums(iters=10):
    work = _lattice(100, 100, list(range(2, 10000, 5)), 4, 0, visits=5)
    eng = _engine(*work)
    eng.run(iters, 0)
    eng.run(7, 2)
    out = _sums(eng), eng.stats()
    eng.close()
    return out


def test_a_call_rerun_after_a_broken_handover_counts_no_iteration_twice(monkeypatch):
    """The knob of tests/test_gpu_convergence.py's test of the same name, with the held-out sums on: a bounded wait gives up,
    the call is re-run from the snapshot, which holds the sums."""
    monkeypatch.setenv('OCC_QUIET', '1')
    ref, st = _headline_sums()
    assert st['fused_fallbacks'] == 0
    _whole(ref, 15)
    monkeypatch.setenv('OCC_DEBUG_BREAK_HANDOVER', '1')
    alt, st = _headline_sums()
    assert st['fused_fallbacks'] == 1
    _whole(alt, 15)
    _same(ref, alt)


def _everything_on_rsr():
    """The reduced-rank workload with every accumulator behind the z update and both kinds of per-site sums on, run (8, 0) then
    (5, 1): per chain the histograms, the batch-means sums, the held-out sums and the site sums, each with its count."""
    eng = _engine(*WORKLOADS['rsr40'](2), site=True, ll=True, bins=64, conv=4)
    eng.run(8, 0)
    eng.run(5, 1)
    out = [dict(hist=eng.hist_counts(c), conv=eng.conv_sums(c), holdout=eng.holdout_sums(c), site=eng.site_sums(c), ll=eng.loglik_sums(c))
           for c in range(eng.n_chains)], eng.stats()
    eng.close()
    return out


def test_a_rerun_call_restores_every_accumulator_from_one_snapshot_loop(monkeypatch):
    """All three accumulators and both kinds of per-site sums are on while a call is re-run after a broken hand-over: the
    snapshot holds uint32 histograms beside float64 sums, each in a buffer of its own, and every array comes back as the
    undisturbed run has it, bit for bit.  An element size or an address taken from the wrong kind would show here."""
    monkeypatch.setenv('OCC_QUIET', '1')
    ref, st = _everything_on_rsr()
    assert st['fused_fallbacks'] == 0
    monkeypatch.setenv('OCC_DEBUG_BREAK_HANDOVER', '1')
    alt, st = _everything_on_rsr()
    assert st['fused_fallbacks'] == 1
    assert len(ref) == len(alt) == 2
    for c, (u, v) in enumerate(zip(ref, alt)):
        assert u['hist']['counts'].dtype == np.uint32 and u['hist']['counts'].shape == (64, 720) and u['conv']['sums'].shape == (11, 720)
        assert u['holdout']['sums'].shape == (5, 180)
        for kind, data in (('hist', 'counts'), ('conv', 'sums'), ('holdout', 'sums')):
            assert u[kind]['count'] == v[kind]['count'] == 12, (c, kind)
            assert np.array_equal(u[kind][data], v[kind][data]), (c, kind, np.count_nonzero(u[kind][data] != v[kind][data]))
        assert np.all(u['hist']['counts'].sum(axis=0) == 12) and np.all(u['conv']['sums'][0] == 12) and np.all(u['holdout']['sums'][CNT] == 12)
        for kind in ('site', 'll'):
            assert u[kind]['count'] == v[kind]['count'] == 12 and sorted(u[kind]) == sorted(v[kind]), (c, kind)
            for name in u[kind]:
                assert np.array_equal(u[kind][name], v[kind][name]), (c, kind, name)


# ------------------------------------------------------------------ 5: nothing else sees the switch
@pytest.mark.parametrize('name', ['queen30x40', 'generic', 'rsr40'])
def test_nothing_else_sees_the_switch(name):
    """alpha, beta, tau, eta, z, the site_* and ll_* sums, region_draws, ppc_draws, moran_draws, hist_counts and conv_sums are the
    same bits with holdout_stats on and off, and holdout_count == conv_count."""
    work = WORKLOADS[name](2)
    prob, keys = work[0], work[1]
    ids = (np.arange(prob.n) % 7).astype(np.int64)
    engines = {}
    for which in ('on', 'off'):
        eng = engines[which] = _engine(*work, on=which == 'on', bins=64, conv=5, site=True, ll=True, ids=ids, ppc=True, moran=True)
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
        a, b = on.conv_sums(c), off.conv_sums(c)
        assert a['count'] == b['count'] == 39 and np.array_equal(a['sums'], b['sums'])
        assert on.holdout_sums(c)['count'] == a['count']
    _whole(_sums(on), 39)
    _same(_sums(on), _two_calls(work))                                    # (and the sums are those of an engine with nothing else on)
    with pytest.raises(ValueError, match='set holdout_data first'):       # (the other handle never heard of them)
        off.get('holdout_count')
    for eng in engines.values():
        eng.close()


def test_windows_and_a_chain_that_does_not_count():
    """120 iterations, 100 past the burn-in, four chains of which the last has its switch off; switching a chain on again
    zeroes its part alone; off keeps everything readable; replacing the data zeroes every chain's sums."""
    work = _workload_a(4)
    eng = _engine(*work)
    eng.set('holdout_stats', 0.0, 3)
    eng.run(120, 20)
    got = _sums(eng)
    _whole(got[:3], 100)
    assert got[3]['count'] == 0 and not got[3]['sums'].any()
    assert [eng.get('holdout_stats', c)[0] for c in range(4)] == [1.0, 1.0, 1.0, 0.0]
    eng.set('holdout_stats', 1.0, 1)                  # on again: zeroes chain 1 alone
    after = _sums(eng)
    assert after[1]['count'] == 0 and not after[1]['sums'].any()
    _same([got[0], got[2]], [after[0], after[2]])
    eng.set('holdout_stats', 0.0, 0)                  # off: stays readable, stops counting
    eng.set_start(1, **work[2][1])                    # occ_set_start and occ_set_keys do not touch the switch
    eng.set_keys(work[1])
    eng.run(6, 1)
    last = _sums(eng)
    _same([got[0]], [last[0]])
    _whole(last[1:2], 5)
    _whole(last[2:3], 105)
    with pytest.raises(ValueError, match='cannot be set while a chain has holdout_stats on'):
        eng.set('holdout_data', eng.get('holdout_data'))
    eng.holdout_data(work[3], work[4])                # (Engine.holdout_data switches every chain off first) the same data again:
    for s in _sums(eng):                              # every chain's sums and count are zero
        assert s['count'] == 0 and not s['sums'].any()
    few = sorted(work[3])[:7]                         # other data, of another size: the sums have its shape
    eng.holdout_data({s: work[3][s] for s in few}, {s: work[4][s] for s in few})
    eng.holdout_stats(True)
    eng.run(3, 0)
    got = _sums(eng)
    assert all(s['sums'].shape == (5, 7) for s in got)
    _whole(got, 3)
    eng.close()


# ------------------------------------------------------------------ 6: the interface
def _packed(work):
    from occuspytial_amd.holdout import holdout_arg
    return holdout_arg(work[3:], work[0])


@pytest.mark.parametrize('name', ['queen13x17', 'rsr40'])
def test_refusals(name):
    work = WORKLOADS[name](2)
    prob = work[0]
    good = _packed(work)
    H, R, q = int(good[0]), int(good[1]), prob.q
    eng = _engine(*work, on=False)
    v, ln = np.zeros(8), ctypes.c_int64(0)
    for nm in ('holdout_data', 'holdout_stats', 'holdout_count', 'holdout_sums'):        # before the first holdout_data
        with pytest.raises(ValueError, match='set holdout_data first'):
            eng.get(nm)
        assert eng._lib.occ_get_state(eng._h, 0, nm.encode(), v.ctypes.data, 8, ctypes.byref(ln)) == -5      # OCC_E_STATE
    for nm in ('holdout_stats', 'holdout_count', 'holdout_sums'):
        with pytest.raises(ValueError, match='set holdout_data first'):
            eng.set(nm, np.zeros(1))
        assert eng._lib.occ_set_state(eng._h, 0, nm.encode(), v.ctypes.data, 1) == -5

    def bad(change, match):
        w = good.copy()
        w = change(w)
        with pytest.raises(ValueError, match=match):
            eng.set('holdout_data', w, 1)
        assert eng._lib.occ_set_state(eng._h, 0, b'holdout_data', w.ctypes.data, w.size) == -1               # OCC_E_BADARG

    def put(i, x):
        def change(w):
            w[i] = x
            return w
        return change
    s0, p0, y0, w0 = 2, 2 + H, 3 + 2 * H, 3 + 2 * H + R
    bad(put(0, 0.0), '1 to n entries')                                       # H = 0
    bad(put(0, H + 0.5), 'whole numbers H and R')
    bad(put(0, np.nan), 'whole numbers H and R')
    bad(put(1, -1.0), 'whole numbers H and R')
    bad(lambda w: w[:1], 'whole numbers H and R')                             # too short to hold H and R
    bad(lambda w: w[:-1], 'has length')
    bad(lambda w: np.append(w, 0.0), 'has length')
    bad(put(0, H + 1.0), 'has length')
    bad(put(s0, 1.5), 'a site is a whole number')
    bad(put(s0, -1.0), 'a site is a whole number')
    bad(put(s0, float(prob.n)), 'a site is a whole number')
    bad(put(s0, float(prob.site_id[0])), 'is surveyed in this handle')         # a surveyed site
    bad(put(s0 + 1, good[s0]), 'appears twice')
    bad(put(p0, 1.0), 'ptr rises from 0 to R')
    bad(put(p0 + 1, 0.0), 'ptr rises from 0 to R')                            # an entry without a row
    bad(put(p0 + 1, 0.5), 'ptr rises from 0 to R')
    bad(put(p0 + H, R - 1.0), 'ptr rises from 0 to R')
    bad(put(y0 + 2, 2.0), 'y is 0 or 1')
    bad(put(y0, 0.5), 'y is 0 or 1')
    bad(put(w0 + 3, np.inf), 'W is finite')
    bad(put(w0 + R * q - 1, np.nan), 'W is finite')
    with pytest.raises(ValueError, match='set holdout_data first'):             # (all or nothing: nothing of the refused data was kept)
        eng.get('holdout_data')
    eng.set('holdout_data', good, 1)                                            # through any valid chain index
    assert np.array_equal(eng.get('holdout_data', 0), good)
    assert [eng.get('holdout_stats', c)[0] for c in (0, 1)] == [0.0, 0.0] and eng.get('holdout_sums', 0).shape == (5 * H,)
    bad(put(y0, 0.5), 'y is 0 or 1')                                            # (a refused replacement leaves the data as they are)
    assert np.array_equal(eng.get('holdout_data', 1), good)
    for x in (0.5, -1.0, 2.0, np.nan):
        with pytest.raises(ValueError, match='holdout_stats is 0 or 1'):
            eng.set('holdout_stats', x)
        w = np.array([x])
        assert eng._lib.occ_set_state(eng._h, 0, b'holdout_stats', w.ctypes.data, 1) == -1
    with pytest.raises(ValueError, match='wrong length'):
        eng.set('holdout_stats', np.ones(2))
    eng.set('holdout_stats', 1.0, 1)
    with pytest.raises(ValueError, match='cannot be set while a chain has holdout_stats on'):
        eng.set('holdout_data', good, 0)
    assert eng._lib.occ_set_state(eng._h, 0, b'holdout_data', good.ctypes.data, good.size) == -5
    # writes: only while the chain's switch is on; cnt and count whole numbers >= 0, every cnt equal
    with pytest.raises(ValueError, match='switched off for this chain'):
        eng.set('holdout_count', 3.0, 0)
    with pytest.raises(ValueError, match='switched off for this chain'):
        eng.set('holdout_sums', np.zeros(5 * H), 0)
    for x in (0.5, -1.0, np.nan):
        with pytest.raises(ValueError, match='holdout_count is a whole number >= 0'):
            eng.set('holdout_count', x, 1)
        w = np.zeros(5 * H)
        w[:H] = x
        with pytest.raises(ValueError, match='cnt slot of holdout_sums holds one whole number >= 0 at every entry'):
            eng.set('holdout_sums', w, 1)
        assert eng._lib.occ_set_state(eng._h, 1, b'holdout_sums', w.ctypes.data, w.size) == -1
    w = np.zeros(5 * H)
    w[:H] = 3.0
    w[H - 1] = 4.0                                                              # (unequal)
    with pytest.raises(ValueError, match='cnt slot of holdout_sums holds one whole number >= 0 at every entry'):
        eng.set('holdout_sums', w, 1)
    with pytest.raises(ValueError, match='wrong length'):
        eng.set('holdout_sums', np.zeros(5 * H - 1), 1)
    assert eng.holdout_sums(1)['count'] == 0 and not eng.holdout_sums(1)['sums'].any()   # (nothing of a refused write was kept)
    eng.run(3, 1)
    got = _sums(eng)
    assert got[0]['count'] == 0 and not got[0]['sums'].any()
    _whole(got[1:], 2)
    # written sums are read back as written, and the next call goes on from them
    w = -(np.arange(5 * H, dtype=np.float64) % 7)
    w[:H] = 2.0
    eng.set('holdout_sums', w, 1)
    eng.set('holdout_count', 2.0, 1)
    assert np.array_equal(eng.get('holdout_sums', 1), w) and eng.get('holdout_count', 1)[0] == 2.0
    eng.run(4, 0)
    got = eng.holdout_sums(1)
    assert got['count'] == 6 and np.all(got['sums'][CNT] == 6)
    assert np.all(got['sums'][LIK] > w.reshape(5, H)[LIK]) and np.all(got['sums'][LOG] < w.reshape(5, H)[LOG])
    eng.close()


def test_probit_handle_refuses():
    from .test_gpu_regions import _probit_problem
    from occuspytial_amd._engine import Engine
    prob, keys, starts = _probit_problem(2)
    eng = Engine(prob, keys)
    for nm in ('holdout_data', 'holdout_stats', 'holdout_count', 'holdout_sums'):
        with pytest.raises(ValueError, match='held-out scoring is not available for the probit model'):
            eng.get(nm)
        with pytest.raises(ValueError, match='held-out scoring is not available for the probit model'):
            eng.set(nm, 1.0)
    v = np.full(1, 1.0)
    assert eng._lib.occ_set_state(eng._h, 0, b'holdout_stats', v.ctypes.data, 1) == -5                      # OCC_E_STATE
    eng.close()


def test_checkpoint_and_restore_mid_run_equal_the_uninterrupted_run():
    work = _workload_a(2)
    e1 = _engine(*work)
    e1.run(22, 5)
    ck = e1.checkpoint()
    assert ck['holdout_stats'].tolist() == [1.0, 1.0] and ck['holdout_count'].tolist() == [17, 17]
    assert ck['holdout_sums'].dtype == np.float64 and ck['holdout_sums'].shape == (2, 5, 300)
    assert np.array_equal(ck['holdout_data'][1], _packed(work))
    held = _sums(e1)
    e1.close()
    e2 = _engine(*work, on=False)                        # a fresh engine that never heard of the sums
    assert not [k for k in e2.checkpoint() if k.startswith('holdout_')]
    e2.restore(ck)
    assert e2._holdout_on and np.array_equal(e2._holdout, _packed(work))
    _same(held, _sums(e2))                               # bit-exact
    e2.run(15, 0)
    got = _sums(e2)
    e2.restore({k: v for k, v in ck.items() if not k.startswith('holdout_')})      # (a checkpoint without them: the switch goes off)
    assert not e2._holdout_on and e2.get('holdout_stats', 0)[0] == 0.0
    e2.close()
    _same(got, _two_calls(work, split=((22, 5), (15, 0))))


def _sampler(cls_name='LogitICARGibbs', **kw):
    """The 30x40 lattice of the other modules' ``_sampler`` with every fourth site withheld -> (sampler, (W_test, y_test))."""
    import occuspytial_amd
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(30, 40, visits=3, p=2, q=2, random_state=2)
    held = list(range(1, 1200, 4))
    Wt, yt = {s: W.pop(s) for s in held}, {s: y.pop(s) for s in held}
    return getattr(occuspytial_amd, cls_name)(Q, W, X, y, random_state=7, **kw), (Wt, yt)


@pytest.mark.parametrize('cls_name, kw', [('LogitICARGibbs', {}), ('LogitRSRGibbs', dict(q=40))])
def test_sampler_returns_the_score_of_the_kept_draws(cls_name, kw):
    from occuspytial_amd.holdout import HoldoutScore, compare
    s, held = _sampler(cls_name, **kw)
    chunked = s.sample(60, burnin=20, chains=3, progressbar=True, holdout=held)   # chunks of 16: one straddles the burn-in
    s1, _ = _sampler(cls_name, **kw)
    one = s1.sample(60, burnin=20, chains=3, progressbar=False, holdout=held)
    plain = _sampler(cls_name, **kw)[0].sample(60, burnin=20, chains=3, progressbar=False)
    assert plain.holdout is None and isinstance(one.holdout, HoldoutScore)
    assert sorted(one.data) == sorted(plain.data)                              # (post.summary and the chains are unchanged)
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(one[name], plain[name]) and np.array_equal(chunked[name], plain[name])
    hs = one.holdout
    assert hs.n_sites == 300 and hs.n_draws.tolist() == [40, 40, 40] and hs.sites.tolist() == sorted(held[0])
    assert hs.detected.tolist() == [bool(np.any(held[1][k])) for k in sorted(held[0])]
    assert np.array_equal(hs.sums, chunked.holdout.sums) and np.all(hs.sums[CNT] == 120)
    assert np.isfinite(hs.elpd) and hs.elpd < 0 and hs.se > 0 and 0 < hs.brier < 1 and 0 <= hs.auc <= 1
    assert np.all((0 < hs.p_detect) & (hs.p_detect < 1)) and np.all(hs.elpd_i >= hs.mean_loglik_i - 1e-12) and 'sites=300' in repr(hs)
    assert compare(hs, chunked.holdout) == {'elpd_diff': 0.0, 'se_diff': 0.0}
    # resume: the sums go on from the checkpoint's, and end as those of an uninterrupted run
    ck = s.checkpoint()
    assert ck['holdout_stats'].tolist() == [1.0] * 3 and ck['holdout_sums'].shape == (3, 5, 300)
    more = s.resume(ck, 30, progressbar=False, holdout=held)
    longer = _sampler(cls_name, **kw)[0].sample(90, burnin=20, chains=3, progressbar=False, holdout=held)
    assert more.holdout.n_draws.tolist() == [70] * 3
    assert np.array_equal(more.holdout.sums, longer.holdout.sums)
    assert np.array_equal(more['alpha'], longer['alpha'][:, 40:])
    few = ({k: held[0][k] for k in sorted(held[0])[:9]}, {k: held[1][k] for k in sorted(held[0])[:9]})
    other = s.resume(ck, 30, progressbar=False, holdout=few)                   # (other data: from zero)
    assert other.holdout.n_sites == 9 and other.holdout.n_draws.tolist() == [30] * 3
    again = s.resume(ck, 5, progressbar=False)                                 # (not asked for: the checkpoint's switch goes off)
    assert again.holdout is None and not s._engine._holdout_on


# ------------------------------------------------------------------ 7: one decision that must come out right
CPU_RATIO = 5.35   # elpd_diff / se_diff of the decision below on the CPU restatement of the ABI (see the test's docstring)
DECISION = dict(size=400, burnin=100, chains=2, every=5)


def decision_models():
    """The 400-site ``make_data`` problem of tests/test_gpu_waic.py's decision (coefficient 2 on one detection covariate; model A is
    given it, model B independent noise in its place) with every fifth surveyed site withheld.
    -> (Q, X, {model: (W_train, y_train, W_test, y_test)})."""
    from .test_gpu_waic import _decision_models
    Q, WA, WB, X, y = _decision_models()
    held = sorted(WA)[::DECISION['every']]
    out = {}
    for name, W in (('A', WA), ('B', WB)):
        out[name] = ({s: W[s] for s in W if s not in held}, {s: y[s] for s in y if s not in held},
                     {s: W[s] for s in held}, {s: y[s] for s in held})
    return Q, X, out


def test_held_out_score_prefers_the_model_that_has_the_detection_covariate():
    """compare(A, B).elpd_diff / se_diff >= 2, the conventional two-standard-error rule.  Iterations and hold-out size were fixed on
    the CPU: both models stepped with the CPU restatement of the ABI (2 chains, 400 iterations, 100 of them burn-in, the sampler's
    own start values and keys), the states read and the score formed in numpy from ``holdout_terms``; the ratio there is
    ``CPU_RATIO`` (elpd_diff = 48.93, se_diff = 9.146; elpd -98.1 for A and -147.0 for B over the 80 withheld sites), more than twice
    the threshold, as required."""
    from occuspytial_amd import LogitICARGibbs
    from occuspytial_amd.holdout import compare
    d = DECISION
    Q, X, models = decision_models()
    out = {}
    for name, (W, y, Wt, yt) in models.items():
        post = LogitICARGibbs(Q, W, X, y, random_state=5).sample(d['size'], burnin=d['burnin'], chains=d['chains'], progressbar=False, holdout=(Wt, yt))
        out[name] = post.holdout
        print('model', name, post.holdout)
        assert post.holdout.n_sites == 80 and post.holdout.n_draws.tolist() == [d['size'] - d['burnin']] * d['chains']
    cmp = compare(out['A'], out['B'])
    print('A against B:', cmp, 'ratio', cmp['elpd_diff'] / cmp['se_diff'], 'on the CPU:', CPU_RATIO)
    assert cmp['elpd_diff'] / cmp['se_diff'] >= 2.0
