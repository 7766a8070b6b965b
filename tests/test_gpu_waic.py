"""Streaming WAIC: the per-site log-likelihood sums accumulated on the device (state names ``ll_*``) against an independent
numpy restatement, bitwise across every way the engine can schedule an iteration, their invariants, and one model
comparison that must come out right.

The workloads are those of test_gpu_site_summaries.py (A: the 30x40 lattice; G: 17x19 with nine covariates of each kind, the
generic kernels; the reduced-rank problem).  The bounds of the restatement test are derived in its docstring, none is
measured."""
import numpy as np
import pytest
from scipy.special import expit

from . import _z_theory as zt
from ._outputs_gpu import engine_with, two_calls
from .test_gpu_parity import KEY, _problem_from_golden, _random_start
from .test_gpu_site_summaries import SUMS as SITE_SUMS
from .test_gpu_site_summaries import _read_all as _read_all_site
from .test_gpu_site_summaries import _rsr_problem, _same as _same_site, _workload_a, _workload_g

pytestmark = pytest.mark.gpu

SUMS = ('ll_lik', 'll_log', 'll_log2')


def _read(eng, chain=0):
    """-> (count, {name: sum}) of one chain."""
    return int(eng.get('ll_count', chain)[0]), {name: eng.get(name, chain) for name in SUMS}


def _read_all(eng):
    return [_read(eng, c) for c in range(eng.n_chains)]


def _same(a, b):
    """Counts equal, every sum bit-equal, chain by chain."""
    assert len(a) == len(b)
    for (ca, sa), (cb, sb) in zip(a, b):
        assert ca == cb, (ca, cb)
        for name in SUMS:
            assert np.array_equal(sa[name], sb[name]), (name, np.abs(sa[name] - sb[name]).max())


def _engine(prob, keys, starts, ll=True, site=False):
    return engine_with(prob, keys, starts, site=site, ll=ll)


def _masks(prob):
    """-> (surveyed, detection seen) as boolean arrays over the n sites."""
    surveyed = np.zeros(prob.n, dtype=bool)
    surveyed[prob.site_id] = True
    seen = np.zeros(prob.n, dtype=bool)
    seen[prob.site_id[prob.obs_site.astype(bool)]] = True
    return surveyed, seen


# ------------------------------------------------------------------ 1: against an independent restatement
def lsig(a):
    """log expit(a), stable on both sides."""
    return np.minimum(a, 0.0) - np.log1p(np.exp(-np.abs(a)))


def _ll_terms(prob, alpha, beta, eta):
    """The marginal log-likelihood l and likelihood L of every surveyed site (z integrated out), in numpy, from the
    definitions -- and, beside them, the size ``b`` that the rounding bound of l is proportional to (docstring of
    ``_restatement``).  -> (l, L, b), each of length n and 0 at the sites that were not surveyed."""
    n = prob.n
    a0 = prob.X @ beta + eta
    a0_abs = np.abs(prob.X * beta).sum(axis=1) + np.abs(eta)          # sum |products| of x_i beta + eta_i
    wa = prob.W @ alpha
    wa_abs = np.abs(prob.W * alpha).sum(axis=1)
    y = np.asarray(prob.y).ravel() != 0
    ll, lik, b = np.zeros(n), np.zeros(n), np.zeros(n)
    ref = zt.problem_terms(prob.X, eta, beta, prob.W, alpha, prob.site_ptr, prob.site_id)   # as if no site had a detection
    for s in range(prob.S):
        i = prob.site_id[s]
        rows = slice(prob.site_ptr[s], prob.site_ptr[s + 1])
        if prob.obs_site[s]:
            t0 = lsig(a0[i])
            terms = lsig(np.where(y[rows], wa[rows], -wa[rows]))
            acc = t0
            for t in terms:                                           # rows in row order
                acc = acc + t
            ll[i], lik[i] = acc, np.exp(acc)
            b[i] = (a0_abs[i] + abs(t0) + 1.0) + np.sum(wa_abs[rows] + np.abs(terms) + 1.0)
        else:
            ll[i], lik[i] = ref['l'][s], ref['D'][s]                   # log space: nothing is subtracted (tests/_z_theory.py)
            b[i] = ref['b'][s] + abs(ll[i])                            # (sum |products_0| + 1) + sum_r (sum |products_r| + 1) + |l|
    return ll, lik, b


def _host_sums(eng, prob, steps=12):
    """``steps`` x occ_step; after each, alpha, beta and eta of every chain are read and the three terms accumulated on the
    host, with the bound's size beside them.  Works on any engine (the device's or the CPU restatement of the ABI)."""
    C, n = eng.n_chains, prob.n
    acc = [{k: np.zeros(n) for k in ('lik', 'log', 'log2', 'b', 'maxabs')} for _ in range(C)]
    for _ in range(steps):
        eng.step()
        for c in range(C):
            alpha, beta, eta = (eng.get(name, c) for name in ('alpha', 'beta', 'eta'))
            ll, lik, b = _ll_terms(prob, alpha, beta, eta)
            a = acc[c]
            a['lik'] += lik
            a['log'] += ll
            a['log2'] += ll * ll
            a['b'] += b
            a['maxabs'] = np.maximum(a['maxabs'], np.abs(ll))
    return acc


def _restatement(prob, keys, starts, cap, steps=12):
    """Switch on, ``steps`` x occ_step; after each step alpha, beta, eta are read and l, L formed on the host from the table of
    the header (include/occ_gibbs.h).  u = 2^-53.  ``ll_count`` is exact; the unsurveyed sites' sums are exactly 0.  Bounds:

    A detection at the site.  l = lsig(a_0) + sum_r lsig(a_r), a_0 = x_i beta + eta_i, a_r = +- w_r alpha.  Host and device
      form each dot product in their own order: both are within (q + 1) u sum |products| of the exact value (p + 1 for a_0),
      so they differ by at most 2 (q + 1) u sum |products| = 2.2e-15 sum |products| for q <= 9.  lsig has slope
      1 - expit(a) <= 1, so the term inherits exactly that; its own evaluation -- exp and log1p to a few ulp of a value
      <= log 2, one subtraction rounded at u |term| -- adds at most 4 u (|term| + 1).  Adding the <= 7 terms and then 12
      iterations rounds at most (7 + 12) u sum |terms|.  Together: below 2.2e-15 sum |products| + 2.6e-15 (|term| + 1) per
      term, held to   B_l = 1e-12 sum_t sum_terms (sum |products| + |term| + 1),   a margin of four hundred.
    No detection.  l = log D, D = (1 - psi) + psi prod_r expit(-w_r alpha), on the host in log space (tests/_z_theory.py:
      l = logaddexp(lsig(-a_0), lsig(a_0) + sum_r lsig(-w_r alpha)), nothing subtracted).  Both terms of D are positive and
      each has the relative error of its logarithm: |d a_0| for 1 - psi and for psi (slope of lsig <= 1), |d a_r| + 4 u per
      factor -- the device takes 1 - psi from exp(-|a_0|) without cancellation, so no 1 / (1 - psi) enters:
        |d l| <= 2 (p + 1) u sum |products_0| + 10 u + sum_r (2 (q + 1) u sum |products_r| + 4 u) + 4 u |l|,
      held to   B_l = 1e-12 sum_t ((sum |products_0| + 1) + sum_r (sum |products_r| + 1) + |l|).
    ll_lik: L <= 1 and d L = L d l (a detection: L = exp(l), plus one ulp of L) or D d l (none): the same absolute bound B_l.
    ll_log2: d(l^2) = 2 |l| d l, summed: 2 max_t |l_t| B_l; the fused multiply-adds round 12 times at u sum l^2, held to
      1e-12 sum l^2.
    ``cap``: B_l must stay below it at every site, as when it grew as 1 / (1 - psi), so that it cannot grow until it hides a
    failure (an error in a sign, a row or a term moves l by far more than 1e-6).  The CPU restatement of the ABI, stepped
    through ``_host_sums`` on these four workloads, keeps B_l below 5.1e-9 (A), 3.0e-9 (wide rows), 5.8e-9 (generic) and
    5.3e-10 (reduced rank) -- the largest values belong to sites whose psi comes within 1e-3 of 1: the caps are 1e-8 (A, wide
    rows), 2e-8 (generic) and 1e-9 (reduced rank), a hundred times below what a wrong term would do."""
    eng = _engine(prob, keys, starts)
    acc = _host_sums(eng, prob, steps)
    surveyed, _ = _masks(prob)
    for c in range(len(keys)):
        count, dev = _read(eng, c)
        a = acc[c]
        B = 1e-12 * a['b']
        B2 = 2.0 * a['maxabs'] * B + 1e-12 * a['log2']
        sv = surveyed
        fig = dict(chain=c, bound_max=B.max(),
                   log_over_bound=np.max(np.abs(dev['ll_log'] - a['log'])[sv] / B[sv]),
                   lik_over_bound=np.max(np.abs(dev['ll_lik'] - a['lik'])[sv] / B[sv]),
                   log2_over_bound=np.max(np.abs(dev['ll_log2'] - a['log2'])[sv] / B2[sv]))
        print('log-likelihood sums against the restatement:', fig)
        assert count == steps
        for name in SUMS:
            assert not dev[name][~sv].any(), name
        assert np.all(dev['ll_lik'][sv] > 0) and np.all(dev['ll_log'][sv] < 0)
        assert B.max() < cap, fig
        assert fig['log_over_bound'] <= 1.0, fig
        assert fig['lik_over_bound'] <= 1.0, fig
        assert fig['log2_over_bound'] <= 1.0, fig
    eng.close()


def test_sums_equal_an_independent_restatement_workload_a():
    prob, keys, starts = _workload_a(2)
    _restatement(prob, keys, starts, cap=1e-8)


def test_sums_equal_an_independent_restatement_wide_rows():
    """A third of this fixture's sites is not surveyed: their sums stay exactly 0."""
    prob, start = _problem_from_golden('ref_graph300_weighted')
    _restatement(prob, [KEY], [start], cap=1e-8)


def test_sums_equal_an_independent_restatement_generic_kernels():
    prob, keys, starts = _workload_g()
    _restatement(prob, keys, starts, cap=2e-8)


def test_reduced_rank_sums_equal_an_independent_restatement():
    """eta is K theta, read as ``eta`` (the reference's ``spatial``)."""
    prob, keys, starts = _rsr_problem(40)
    _restatement(prob, keys, starts, cap=1e-9)


# ------------------------------------------------------------------ 2: bit-equal however the iterations are scheduled
def _replay_against_stepping(prob, keys, starts):
    e1 = _engine(prob, keys, starts)
    rec1 = e1.run(33, 4) + e1.run(10, 0)
    e2 = _engine(prob, keys, starts, ll=False)
    for _ in range(4):
        e2.step()
    e2.loglik_stats(True)
    for _ in range(39):
        e2.step()
    s1, s2 = _read_all(e1), _read_all(e2)
    assert [c for c, _ in s1] == [39] * len(keys)
    _same(s1, s2)
    e3 = _engine(prob, keys, starts, ll=False)     # the switch never touched: the feature only reads
    rec3 = e3.run(33, 4) + e3.run(10, 0)
    for u, v in zip(rec1, rec3):
        assert np.array_equal(u, v)
    for c in range(len(keys)):
        for name in ('alpha', 'beta', 'eta', 'z'):
            assert np.array_equal(e1.get(name, c), e3.get(name, c)), name
        assert e1.get('tau', c) == e3.get('tau', c)
    with pytest.raises(ValueError, match='not been switched on'):
        e3.get('ll_lik')
    for e in (e1, e2, e3):
        e.close()


def test_graph_replay_equals_eager_stepping_bitwise():
    _replay_against_stepping(*_workload_a(2))


def test_generic_kernels_graph_replay_equals_eager_stepping_bitwise():
    _replay_against_stepping(*_workload_g())


def test_reduced_rank_graph_replay_equals_eager_stepping_bitwise():
    _replay_against_stepping(*_rsr_problem(40))


def _two_calls(prob, keys, starts, site=False):
    return two_calls(lambda: _engine(prob, keys, starts, site=site), lambda eng: (_read_all(eng), _read_all_site(eng) if site else None))


SCHED_KEYS = ('OCC_EVENT_SYNC', 'OCC_STREAM_EVENTS', 'OCC_CU_SPLIT', 'OCC_NO_SIDE_STREAM', 'OCC_EAGER_ONLY', 'OCC_NO_PERSISTENT',
              'OCC_DEBUG_STREAMS_SERIALISED', 'OCC_NO_XCD_LOCAL')


@pytest.mark.parametrize('env', [{'OCC_EVENT_SYNC': '1'}, {'OCC_EVENT_SYNC': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_CU_SPLIT': '0'},
                                 {'OCC_DEBUG_STREAMS_SERIALISED': '1'},
                                 {'OCC_NO_SIDE_STREAM': '1'}, {'OCC_EAGER_ONLY': '1'}, {'OCC_NO_XCD_LOCAL': '1'},
                                 {'OCC_NO_XCD_LOCAL': '1', 'OCC_CU_SPLIT': '0'},
                                 {'OCC_NO_PERSISTENT': '1', 'OCC_STREAM_EVENTS': '1'}, {'OCC_NO_PERSISTENT': '1', 'OCC_NO_SIDE_STREAM': '1'}])
def test_every_scheduling_mode_gives_the_same_sums(monkeypatch, env):
    prob, keys, starts = _workload_a(2)
    for k in SCHED_KEYS:
        monkeypatch.delenv(k, raising=False)
    ref, _ = _two_calls(prob, keys, starts)
    assert [c for c, _ in ref] == [39, 39]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _same(ref, _two_calls(prob, keys, starts)[0])


def test_the_two_kinds_of_sums_do_not_see_each_other():
    """ll_* with the site sums beside them == ll_* alone; site_* with the log-likelihood sums beside them == site_* alone;
    and the switches are independent: one chain of each combination in one handle."""
    prob, keys, starts = _workload_a(2)
    ll_alone, _ = _two_calls(prob, keys, starts)
    ll_both, site_both = _two_calls(prob, keys, starts, site=True)
    _same(ll_alone, ll_both)
    only = _engine(prob, keys, starts, ll=False, site=True)
    only.run(33, 4)
    only.run(10, 0)
    _same_site(_read_all_site(only), site_both)
    only.close()
    mixed = _engine(prob, keys, starts, ll=False)       # chain 0: the log-likelihood sums only; chain 1: the site sums only
    mixed.set('ll_stats', 1.0, 0)
    mixed.set('site_stats', 1.0, 1)
    assert [mixed.get('ll_stats', c)[0] for c in (0, 1)] == [1.0, 0.0]
    assert [mixed.get('site_stats', c)[0] for c in (0, 1)] == [0.0, 1.0]
    mixed.run(33, 4)
    mixed.run(10, 0)
    _same([ll_alone[0]], [_read(mixed, 0)])
    c1, s1 = _read(mixed, 1)
    assert c1 == 0 and all(not s1[name].any() for name in SUMS)
    got = _read_all_site(mixed)
    _same_site([site_both[1]], [got[1]])
    assert got[0][0] == 0 and all(not got[0][1][name].any() for name in SITE_SUMS)
    mixed.set('ll_stats', 0.0, 0)                       # back to the twin that keeps the site sums only
    assert mixed.get('site_stats', 1)[0] == 1.0
    mixed.run(5, 0)
    _same([ll_alone[0]], [_read(mixed, 0)])
    assert _read_all_site(mixed)[1][0] == 44
    mixed.close()


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
        eng.run(24, 0)
        eng.step()
        out[mode] = _read_all(eng)
        assert eng.stats()['fused_fallbacks'] == 0
        eng.close()
    assert [c for c, _ in out['tiles']] == [25, 25]
    _same(out['tiles'], out['launch_per_step'])


def test_batched_chains_have_the_sums_of_single_chain_runs():
    prob, _ = _problem_from_golden('ref_graph300_weighted')
    keys = [KEY, KEY ^ 0xABCDEF, 12345]
    rng = np.random.default_rng(3)
    starts = [dict(alpha=rng.standard_normal(prob.q), beta=rng.standard_normal(prob.p), tau=1.0 + c,
                   eta=(lambda e: e - e.mean())(rng.standard_normal(prob.n))) for c in range(3)]
    batch = _engine(prob, keys, starts)
    batch.run(20, 4)
    both = _read_all(batch)
    batch.close()
    for c in range(3):
        solo = _engine(prob, [keys[c]], [starts[c]])
        solo.run(20, 4)
        _same([both[c]], _read_all(solo))
        solo.close()
    assert [c for c, _ in both] == [16, 16, 16]


def test_engine_group_routes_switch_sums_and_checkpoints_by_chain():
    """Three chains over two engines (both on device 0 here): chain c lives on engine c % 2."""
    from occuspytial_amd._engine import Engine, EngineGroup
    prob, keys, starts = _workload_a(3)
    grp = EngineGroup(prob, keys, [0, 0], engine_factory=lambda pr, ks, dev: Engine(pr, ks, device=dev))
    for c in range(3):
        grp.set_start(c, **starts[c])
    grp.loglik_stats(True)
    grp.run(20, 5)
    ck = grp.checkpoint()
    assert ck['ll_count'].ravel().tolist() == [15, 15, 15] and ck['ll_log'].shape == (3, prob.n) and 'site_psi' not in ck
    grp.restore(ck)
    grp.run(10, 0)
    got = [(grp.loglik_sums(c)['count'], {'ll_' + k: v for k, v in grp.loglik_sums(c).items() if k != 'count'}) for c in range(3)]
    grp.close()
    one = _engine(prob, keys, starts)
    one.run(20, 5)
    one.run(10, 0)
    _same(_read_all(one), got)
    one.close()


def _headline_sums(iters=10):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(100, 100, visits=5, p=2, q=2, random_state=0)
    prob = FlatProblem(Q, W, X, y)
    eng = _engine(prob, [KEY + 5 * c for c in range(4)], [_random_start(prob, 60 + c) for c in range(4)], site=True)
    eng.run(iters, 0)
    eng.run(7, 2)
    out = (_read_all(eng), _read_all_site(eng)), eng.stats()
    eng.close()
    return out


def _rsr_sums():
    prob, keys, starts = _rsr_problem(40)
    eng = _engine(prob, keys, starts)
    eng.run(8, 0)
    eng.run(5, 1)
    out = _read_all(eng), eng.stats()
    eng.close()
    return out


def test_a_call_rerun_after_a_barrier_timeout_counts_no_iteration_twice(monkeypatch):
    """The knobs of test_barrier_timeout_falls_back_to_launch_per_step_with_the_same_bits, with both switches on."""
    (ref, ref_site), _ = _headline_sums()
    monkeypatch.setenv('OCC_CU_SPLIT', '32')
    monkeypatch.setenv('OCC_DEBUG_SKIP_RESIDENCY_PROBE', '1')
    monkeypatch.setenv('OCC_QUIET', '1')
    (alt, alt_site), st = _headline_sums()
    assert st['fused_fallbacks'] == 1
    assert [c for c, _ in alt] == [15] * 4
    _same(ref, alt)
    _same_site(ref_site, alt_site)


def test_a_call_rerun_after_a_broken_handover_counts_no_iteration_twice(monkeypatch):
    """The knob of test_broken_stream_handover_falls_back_with_the_same_bits: fused ICAR path and reduced-rank model."""
    monkeypatch.setenv('OCC_QUIET', '1')
    (ref, ref_site), _ = _headline_sums()
    rsr_ref, _ = _rsr_sums()
    monkeypatch.setenv('OCC_DEBUG_BREAK_HANDOVER', '1')
    (alt, alt_site), st = _headline_sums()
    assert st['fused_fallbacks'] == 1
    assert [c for c, _ in alt] == [15] * 4
    _same(ref, alt)
    _same_site(ref_site, alt_site)
    rsr_alt, rst = _rsr_sums()
    assert rst['fused_fallbacks'] == 1
    assert [c for c, _ in rsr_alt] == [12, 12]
    _same(rsr_ref, rsr_alt)


def test_checkpoint_and_restore_keep_the_sums():
    prob, keys, starts = _workload_a(2)
    e1 = _engine(prob, keys, starts, site=True)
    r1 = e1.run(20, 5)
    ck = e1.checkpoint()
    assert np.array_equal(ck['ll_count'].ravel(), [15, 15]) and ck['ll_lik'].shape == (2, prob.n) and 'site_psi' in ck
    e1.restore(ck)
    r1 = r1 + e1.run(15, 0)
    e2 = _engine(prob, keys, starts, site=True)
    r2 = e2.run(20, 5) + e2.run(15, 0)
    s1 = _read_all(e1)
    assert [c for c, _ in s1] == [30, 30]
    _same(s1, _read_all(e2))
    _same_site(_read_all_site(e1), _read_all_site(e2))
    for u, v in zip(r1, r2):
        assert np.array_equal(u, v)
    # switched off, the sums stay readable and no longer move; they may be written only while the switch is on
    e2.loglik_stats(False)
    e2.run(3, 0)
    _same(s1, _read_all(e2))
    assert e2.get('ll_stats')[0] == 0.0 and e2.get('site_stats')[0] == 1.0 and _read_all_site(e2)[0][0] == 33
    with pytest.raises(ValueError, match='switched off'):
        e2.set('ll_count', 3.0)
    with pytest.raises(ValueError, match='switched off'):
        e2.set('ll_log', np.zeros(prob.n))
    e2.loglik_stats(True)
    c0, s0 = _read(e2)
    assert c0 == 0 and all(not s0[name].any() for name in SUMS)
    with pytest.raises(ValueError, match='whole number'):
        e2.set('ll_count', 2.5)
    e1.close()
    e2.close()


def _sampler():
    from occuspytial_amd import LogitICARGibbs
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(30, 40, visits=3, p=2, q=2, random_state=2)
    return LogitICARGibbs(Q, W, X, y, random_state=7), X.shape[0]


def _waic_equal(a, b):
    assert a.n_draws.tolist() == b.n_draws.tolist() and np.array_equal(a.site_id, b.site_id)
    for name in ('lppd_i', 'p_waic_i', 'elpd_i'):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for name in ('lppd', 'p_waic', 'elpd', 'waic', 'se', 'n_high_var'):
        assert getattr(a, name) == getattr(b, name), name


def test_sampler_returns_the_waic_of_the_kept_draws():
    s, n = _sampler()
    chunked = s.sample(60, burnin=20, chains=3, progressbar=True, waic=True)   # chunks of 16: one straddles the burn-in
    one = _sampler()[0].sample(60, burnin=20, chains=3, progressbar=False, waic=True)
    plain = _sampler()[0].sample(60, burnin=20, chains=3, progressbar=False)
    with_sites = _sampler()[0].sample(60, burnin=20, chains=3, progressbar=False, waic=True, site_summaries=True)
    assert plain.waic is None and one.sites is None and with_sites.sites is not None
    _waic_equal(chunked.waic, one.waic)
    _waic_equal(with_sites.waic, one.waic)
    assert one.waic.n_draws.tolist() == [40, 40, 40] and one.waic.n_sites == n
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(one[name], plain[name]) and np.array_equal(chunked[name], plain[name])
    w = one.waic
    assert np.all(np.isfinite(w.elpd_i)) and np.all(w.lppd_i < 0) and np.all(w.p_waic_i >= 0) and w.waic == -2.0 * w.elpd
    # resume goes on from the checkpoint's sums
    ck = s.checkpoint()
    assert 'll_log' in ck and 'site_psi' not in ck
    more = s.resume(ck, 30, progressbar=False, waic=True)
    whole = _sampler()[0].sample(90, burnin=20, chains=3, progressbar=False, waic=True)
    assert more.waic.n_draws.tolist() == [70, 70, 70]
    _waic_equal(more.waic, whole.waic)
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(more[name], whole[name][:, 40:])


def test_reduced_rank_sampler_returns_waic():
    from occuspytial_amd import LogitRSRGibbs
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(24, 30, visits=3, p=2, q=2, random_state=4)
    out = LogitRSRGibbs(Q, W, X, y, random_state=5, q=40).sample(30, burnin=10, chains=2, progressbar=False, waic=True)
    assert out.waic.n_draws.tolist() == [20, 20] and out.waic.elpd_i.shape == (X.shape[0],)
    assert np.isfinite(out.waic.waic) and np.isfinite(out.waic.se) and 0 < out.waic.p_waic


def test_probit_engine_refuses_the_state_names():
    from occuspytial_amd import ProbitRSRGibbs
    from occuspytial_amd._engine import Engine
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(12, 12, visits=3, p=2, q=2, random_state=1)
    s = ProbitRSRGibbs(Q, W, X, y, random_state=1, q=10)
    eng = Engine(s._problem, [KEY])
    for name in ('ll_stats', 'll_count') + SUMS:
        with pytest.raises(ValueError, match='not available for the probit model'):
            eng.get(name)
    with pytest.raises(ValueError, match='not available for the probit model'):
        eng.set('ll_stats', 1.0)
    eng.close()


# ------------------------------------------------------------------ 3: invariants
def test_invariants_of_a_long_run():
    """450 iterations, 400 kept, four chains; N = 400, u = 2^-53.  At every surveyed site, each up to the rounding of sums of
    N terms (a relative N u = 4.4e-14 per sum, held to 1e-12):
      0 < sum L <= count (L is a probability) and sum l <= 0;
      log(sum L / N) >= sum l / N (Jensen: the logarithm of the mean of exp(l) is at least the mean of l) -- up to
        1e-12 (1 + |sum l| / N), the absolute rounding of either side;
      (sum l)^2 <= N sum l^2 (Cauchy-Schwarz) -- up to a relative 1e-12."""
    prob, keys, starts = _workload_a(4)
    eng = _engine(prob, keys, starts)
    eng.run(450, 50)
    N = 400
    surveyed, seen = _masks(prob)
    assert seen.any() and (surveyed & ~seen).any()
    for c in range(4):
        count, s = _read(eng, c)
        lik, log, log2 = (s[name][surveyed] for name in SUMS)
        assert count == N
        assert np.all(lik > 0) and np.all(lik <= N * (1 + 1e-12)) and np.all(log <= 0)
        gap = np.log(lik / N) - log / N
        print('Jensen gap: min', gap.min(), 'max', gap.max(), ' Cauchy-Schwarz: min', (N * log2 - log ** 2).min())
        assert np.all(gap >= -1e-12 * (1.0 + np.abs(log) / N))
        assert np.all(N * log2 >= log ** 2 * (1 - 1e-12))
    eng.close()
    # (every site of that lattice is surveyed) a fixture where a third of the sites is not: their sums stay exactly 0
    prob, start = _problem_from_golden('ref_queen150_ragged')
    surveyed, _ = _masks(prob)
    assert (~surveyed).sum() == 50
    eng = _engine(prob, [KEY], [start])
    eng.run(60, 10)
    count, s = _read(eng)
    assert count == 50
    for name in SUMS:
        assert not s[name][~surveyed].any() and np.all(s[name][surveyed] != 0)
    eng.close()


# ------------------------------------------------------------------ 4: one decision that must come out right
CPU_RATIO = 13.3   # elpd_diff / se_diff of the decision below on the CPU restatement of the ABI: 294.7 / 22.08
DECISION = dict(n=400, visits=4, seed=11, coef=2.0, noise_seed=101, y_seed=202, size=400, burnin=100, chains=2)


def _decision_models():
    """A 20x20-site problem of ``make_data`` (every site surveyed four times, p = q = 2) whose detections are drawn afresh
    with ONE strong detection covariate: y_r ~ Bernoulli(z_i expit(-0.5 + coef w_r)).  Model A is given W; model B gets that
    column replaced by independent noise of the same law, uniform on (-2, 2).  Fixed seeds.  -> (Q, W_A, W_B, X, y)."""
    from occuspytial_amd.utils import make_data
    d = DECISION
    Q, W, X, _, _, _, _, z = make_data(n=d['n'], min_v=d['visits'], max_v=d['visits'], ns=d['n'], p=2, q=2, random_state=d['seed'])
    rng_y, rng_b = np.random.default_rng(d['y_seed']), np.random.default_rng(d['noise_seed'])
    WA, WB, y = {}, {}, {}
    for site in sorted(W):
        Wi = np.asarray(W[site], dtype=float)
        y[site] = rng_y.binomial(1, z[site] * expit(-0.5 + d['coef'] * Wi[:, 1]))
        WA[site] = Wi
        Wb = Wi.copy()
        Wb[:, 1] = rng_b.uniform(-2, 2, size=Wi.shape[0])
        WB[site] = Wb
    return Q, WA, WB, X, y


def test_waic_prefers_the_model_that_has_the_detection_covariate():
    """compare(A, B).elpd_diff > 4 se_diff, and 0 < p_waic < S for both.  Seed, size and coefficient were chosen on the CPU:
    both models stepped with the CPU restatement of the ABI (2 chains, 400 iterations, 100 of them burn-in, the sampler's own
    start values and keys) and WAIC formed in numpy from ``_ll_terms``.  There elpd_diff = 294.7 and se_diff = 22.08, a ratio of
    13.3 (``CPU_RATIO``): more than twice the threshold of 4, as required.  (410 detections at 209 of the 400 sites; WAIC
    1067.4 for A with p_waic = 21.6, 1656.8 for B with p_waic = 26.0.)"""
    from occuspytial_amd import LogitICARGibbs
    from occuspytial_amd.waic import compare
    d = DECISION
    Q, WA, WB, X, y = _decision_models()
    out = {}
    for name, W in (('A', WA), ('B', WB)):
        post = LogitICARGibbs(Q, W, X, y, random_state=5).sample(d['size'], burnin=d['burnin'], chains=d['chains'], progressbar=False, waic=True)
        out[name] = post.waic
        print('model', name, post.waic)
        assert post.waic.n_sites == d['n'] and post.waic.n_draws.tolist() == [d['size'] - d['burnin']] * d['chains']
        assert 0 < post.waic.p_waic < post.waic.n_sites
    cmp = compare(out['A'], out['B'])
    print('A against B:', cmp, 'ratio', cmp['elpd_diff'] / cmp['se_diff'], 'on the CPU:', CPU_RATIO)
    assert cmp['elpd_diff'] > 4.0 * cmp['se_diff']
