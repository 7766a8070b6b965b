"""Per-site posterior sums accumulated on the device (state names ``site_*``): against an independent numpy restatement,
against the oracle, and bitwise across every way the engine can schedule an iteration.

Workload A: the 30x40 lattice of ``test_every_scheduling_mode_gives_the_same_chains``; workload G: 17x19 with nine covariates of
each kind (the generic kernels).  The bounds of the restatement test are derived in its docstring, none is measured."""
import numpy as np
import pytest
from scipy.special import expit

from . import _z_theory as zt
from ._outputs_gpu import engine_with, two_calls
from .test_gpu_parity import KEY, _problem_from_golden, _random_start

pytestmark = pytest.mark.gpu

SUMS = ('site_psi', 'site_occ', 'site_z', 'site_eta', 'site_eta2')


def _read(eng, chain=0):
    """-> (count, {name: sum}) of one chain."""
    return int(eng.get('site_count', chain)[0]), {name: eng.get(name, chain) for name in SUMS}


def _read_all(eng):
    return [_read(eng, c) for c in range(eng.n_chains)]


def _same(a, b):
    """Counts equal, every sum bit-equal, chain by chain."""
    assert len(a) == len(b)
    for (ca, sa), (cb, sb) in zip(a, b):
        assert ca == cb, (ca, cb)
        for name in SUMS:
            assert np.array_equal(sa[name], sb[name]), (name, np.abs(sa[name] - sb[name]).max())


def _workload_a(chains=2):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(30, 40, visits=3, p=2, q=2, random_state=2)
    prob = FlatProblem(Q, W, X, y)
    rng = np.random.default_rng(3)
    starts = []
    for _ in range(chains):
        eta = rng.standard_normal(prob.n)
        starts.append(dict(eta=eta - eta.mean(), alpha=rng.standard_normal(2), beta=rng.standard_normal(2), tau=1.0))
    return prob, [KEY + 11 * c for c in range(chains)], starts


def _workload_g():
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(17, 19, visits=6, p=9, q=9, random_state=18)
    prob = FlatProblem(Q, W, X, y)
    rng = np.random.default_rng(9)
    start = dict(alpha=0.3 * rng.standard_normal(9), beta=0.3 * rng.standard_normal(9), tau=1.1,
                 eta=(lambda e: e - e.mean())(rng.standard_normal(prob.n)))
    return prob, [KEY + 1], [start]


def _rsr_problem(q):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(24, 30, visits=3, p=2, q=2, random_state=4)
    prob = FlatProblem(Q, W, X, y)
    m = prob.enable_rsr(q=q)['dim']
    rng = np.random.default_rng(8)
    starts = [dict(alpha=rng.standard_normal(2), beta=rng.standard_normal(2), tau=1.0 + c, eta=rng.standard_normal(m)) for c in range(2)]
    return prob, [KEY, KEY + 1], starts


def _engine(prob, keys, starts, on=True):
    return engine_with(prob, keys, starts, site=on)


# ------------------------------------------------------------------ 1 / 7: against an independent restatement
def _terms(prob, alpha, beta, eta):
    """psi and P(z = 1 | alpha, beta, eta, y) of every site from the reference's formulas (logit.py:234-252), in numpy; the
    probability of a surveyed site without a detection from the log-space reference of tests/_z_theory.py, which subtracts
    nothing."""
    psi = expit(prob.X @ beta + eta)
    pr = psi.copy()                                   # unsurveyed sites
    ref = zt.problem_terms(prob.X, eta, beta, prob.W, alpha, prob.site_ptr, prob.site_id)
    pr[prob.site_id] = np.where(np.asarray(prob.obs_site) != 0, 1.0, ref['pr'])
    return psi, pr


def _restatement(prob, keys, starts, cap, steps=12):
    """Switch on, ``steps`` x occ_step; after each step alpha, beta, eta, z are read and the five terms accumulated on the
    host.  ``pr`` of iteration t uses alpha of iteration t and is formed before z is updated.  Bounds:
      site_count, site_z: exact;
      site_eta, site_eta2: 1e-12 relative to sum |term| (12 additions of 2^-53 each, hundred-fold margin);
      site_psi / N: 1e-12 absolute (host and device form x beta + eta in different orders, |d| <= (p + 1) 2^-53 sum |terms|
        <= 1.5e-13 for p <= 12 even if the terms sum to 100; psi' <= 1/4; two expit implementations differ by a few ulp of 1);
      site_occ / N at site i: 1e-12 absolute, against the log-space reference of tests/_z_theory.py (pr has the slope
        pr (1 - pr) <= 1/4 in its logit a_0 + sum_r lsig(t_r), which host and device form within 2 (p + 1) u sum |products| of
        each other; the device takes 1 - psi without cancellation, so no 1 / (1 - psi) enters) -- and the bound stays capped
        (``cap``) as it was when it grew with 1 / (1 - psi)."""
    eng = _engine(prob, keys, starts)
    C, n = len(keys), prob.n
    acc = [{k: np.zeros(n) for k in ('psi', 'occ', 'z', 'eta', 'eta2', 'abs_eta')} for _ in range(C)]
    for _ in range(steps):
        eng.step()
        for c in range(C):
            alpha, beta, eta, z = (eng.get(name, c) for name in ('alpha', 'beta', 'eta', 'z'))
            psi, pr = _terms(prob, alpha, beta, eta)
            a = acc[c]
            a['psi'] += psi
            a['occ'] += pr
            a['z'] += z
            a['eta'] += eta
            a['eta2'] += eta * eta
            a['abs_eta'] += np.abs(eta)
    N = float(steps)
    for c in range(C):
        count, dev = _read(eng, c)
        a = acc[c]
        bound = np.full(n, 1e-12)
        fig = dict(chain=c, eta=np.max(np.abs(dev['site_eta'] - a['eta']) / a['abs_eta']),
                   eta2=np.max(np.abs(dev['site_eta2'] - a['eta2']) / a['eta2']),
                   psi=np.max(np.abs(dev['site_psi'] - a['psi'])) / N,
                   occ_over_bound=np.max(np.abs(dev['site_occ'] - a['occ']) / N / bound), bound_max=bound.max())
        print('site sums against the restatement:', fig)
        assert count == steps
        assert np.array_equal(dev['site_z'], a['z'])
        assert fig['eta'] <= 1e-12 and fig['eta2'] <= 1e-12, fig
        assert fig['psi'] <= 1e-12, fig
        assert bound.max() < cap, fig
        assert fig['occ_over_bound'] <= 1.0, fig
    eng.close()


def test_sums_equal_an_independent_restatement_workload_a():
    prob, keys, starts = _workload_a(2)
    _restatement(prob, keys, starts, cap=1e-11)


def test_sums_equal_an_independent_restatement_wide_rows():
    prob, start = _problem_from_golden('ref_graph300_weighted')
    _restatement(prob, [KEY], [start], cap=1e-11)


def test_sums_equal_an_independent_restatement_generic_kernels():
    prob, keys, starts = _workload_g()
    _restatement(prob, keys, starts, cap=1e-9)


def test_reduced_rank_sums_equal_an_independent_restatement():
    """eta is K theta, read as ``eta`` (the reference's ``spatial``)."""
    prob, keys, starts = _rsr_problem(40)
    _restatement(prob, keys, starts, cap=1e-11)


# ------------------------------------------------------------------ 2: against the oracle, exact
@pytest.mark.parametrize('case', ['ref_queen150_ragged', 'ref_queen150_hparams', 'ref_rook400_v3', 'ref_queen400_v3', 'ref_graph300_weighted'])
def test_z_sums_equal_the_oracles_in_the_reseated_lock_step(oracle, case):
    """The lock step of test_lockstep_iterations_match_oracle: writing alpha, beta, tau, eta, z, xz between the steps does not
    disturb the sums."""
    prob, start = _problem_from_golden(case)
    eng = _engine(prob, [KEY], [start])
    orc = oracle.OracleSampler(prob, KEY)
    orc.set_start(**start)
    zsum = np.zeros(prob.n)
    for _ in range(6):
        eng.step()
        orc.step()
        assert np.array_equal(eng.get('z'), orc.get('z'))
        zsum += orc.get('z')
        for name in ('alpha', 'beta', 'tau', 'eta', 'z', 'xz'):
            eng.set(name, orc.get(name))
    count, dev = _read(eng)
    assert count == 6 and np.array_equal(dev['site_z'], zsum)
    eng.close()


# ------------------------------------------------------------------ 3 / 7: graph replay == eager stepping
def _replay_against_stepping(prob, keys, starts):
    e1 = _engine(prob, keys, starts)
    rec1 = e1.run(33, 4) + e1.run(10, 0)
    e2 = _engine(prob, keys, starts, on=False)
    for _ in range(4):
        e2.step()
    e2.site_stats(True)
    for _ in range(39):
        e2.step()
    s1, s2 = _read_all(e1), _read_all(e2)
    assert [c for c, _ in s1] == [39] * len(keys)
    _same(s1, s2)
    e3 = _engine(prob, keys, starts, on=False)     # the switch never touched: the feature only reads
    rec3 = e3.run(33, 4) + e3.run(10, 0)
    for u, v in zip(rec1, rec3):
        assert np.array_equal(u, v)
    for c in range(len(keys)):
        assert np.array_equal(e1.get('eta', c), e3.get('eta', c)) and np.array_equal(e1.get('z', c), e3.get('z', c))
    with pytest.raises(ValueError, match='not been switched on'):
        e3.get('site_psi')
    for e in (e1, e2, e3):
        e.close()


def test_graph_replay_equals_eager_stepping_bitwise():
    _replay_against_stepping(*_workload_a(2))


def test_reduced_rank_large_basis_graph_replay_equals_eager_stepping_bitwise():
    """A basis above 128 columns: the blocked one-stream path."""
    _replay_against_stepping(*_rsr_problem(160))


# ------------------------------------------------------------------ 4: every scheduling mode
def _two_calls(prob, keys, starts):
    return two_calls(lambda: _engine(prob, keys, starts), _read_all)


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
    ref = _two_calls(prob, keys, starts)
    assert [c for c, _ in ref] == [39, 39]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
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
        eng.run(24, 0)
        eng.step()
        out[mode] = _read_all(eng)
        assert eng.stats()['fused_fallbacks'] == 0
        eng.close()
    assert [c for c, _ in out['tiles']] == [25, 25]
    _same(out['tiles'], out['launch_per_step'])


def test_a_solve_carried_into_a_second_replay_is_counted_once(monkeypatch):
    """The Krylov cap forced low: k_z_ob runs its skip pass for the carried solve; that pass adds nothing."""
    prob, start = _problem_from_golden('ref_queen150_ragged')
    keys = [KEY, KEY + 1]
    ref = _engine(prob, keys, [start, start])
    ref.run(12, 0)
    want = _read_all(ref)
    ref.close()
    monkeypatch.setenv('OCC_FORCE_KRYLOV_CAP', '4')
    monkeypatch.setenv('OCC_NO_PERSISTENT', '1')
    low = _engine(prob, keys, [start, start])
    low.run(12, 0)
    assert low.stats()['stalls'] > 0
    got = _read_all(low)
    low.close()
    assert [c for c, _ in got] == [12, 12]
    _same(want, got)


# ------------------------------------------------------------------ 5: batched == solo
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
    grp.site_stats(True)
    grp.run(20, 5)
    ck = grp.checkpoint()
    assert ck['site_count'].ravel().tolist() == [15, 15, 15] and ck['site_eta'].shape == (3, prob.n)
    grp.restore(ck)
    grp.run(10, 0)
    got = [(grp.site_sums(c)['count'], {'site_' + k: v for k, v in grp.site_sums(c).items() if k != 'count'}) for c in range(3)]
    grp.close()
    one = _engine(prob, keys, starts)
    one.run(20, 5)
    one.run(10, 0)
    _same(_read_all(one), got)
    one.close()


# ------------------------------------------------------------------ 6: no double counting after a fallback
def _headline_sums(iters=10):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(100, 100, visits=5, p=2, q=2, random_state=0)
    prob = FlatProblem(Q, W, X, y)
    eng = _engine(prob, [KEY + 5 * c for c in range(4)], [_random_start(prob, 60 + c) for c in range(4)])
    eng.run(iters, 0)
    eng.run(7, 2)
    out = _read_all(eng), eng.stats()
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
    """The knobs of test_barrier_timeout_falls_back_to_launch_per_step_with_the_same_bits, with the switch on."""
    ref, _ = _headline_sums()
    monkeypatch.setenv('OCC_CU_SPLIT', '32')
    monkeypatch.setenv('OCC_DEBUG_SKIP_RESIDENCY_PROBE', '1')
    monkeypatch.setenv('OCC_QUIET', '1')
    alt, st = _headline_sums()
    assert st['fused_fallbacks'] == 1
    assert [c for c, _ in alt] == [15] * 4
    _same(ref, alt)


def test_a_call_rerun_after_a_broken_handover_counts_no_iteration_twice(monkeypatch):
    """The knob of test_broken_stream_handover_falls_back_with_the_same_bits: fused ICAR path and reduced-rank model."""
    monkeypatch.setenv('OCC_QUIET', '1')
    ref, _ = _headline_sums()
    rsr_ref, _ = _rsr_sums()
    monkeypatch.setenv('OCC_DEBUG_BREAK_HANDOVER', '1')
    alt, st = _headline_sums()
    assert st['fused_fallbacks'] == 1
    assert [c for c, _ in alt] == [15] * 4
    _same(ref, alt)
    rsr_alt, rst = _rsr_sums()
    assert rst['fused_fallbacks'] == 1
    assert [c for c, _ in rsr_alt] == [12, 12]
    _same(rsr_ref, rsr_alt)


# ------------------------------------------------------------------ 8: invariants
def test_invariants_of_a_long_run():
    """Sites with a detection: site_occ == site_z == count exactly.  Unsurveyed sites: site_occ == site_psi bit for bit
    (pr = psi there).  0 < mean psi < 1.  And |site_z - site_occ| / N <= 7 / sqrt(N) at every site and chain -- Azuma: given
    the rest, z_t is Bernoulli(pr_t) from its own uniform, so sum (z_t - pr_t) is a martingale with increments in [-1, 1]
    and P(|sum| >= 7 sqrt(N)) <= 2 exp(-24.5) ~ 5e-11 per site."""
    prob, keys, starts = _workload_a(4)
    eng = _engine(prob, keys, starts)
    eng.run(450, 50)
    N = 400
    seen = np.zeros(prob.n, dtype=bool)
    seen[prob.site_id[prob.obs_site.astype(bool)]] = True
    unsurveyed = np.ones(prob.n, dtype=bool)
    unsurveyed[prob.site_id] = False
    assert seen.any()
    for c in range(4):
        count, s = _read(eng, c)
        assert count == N
        assert np.all(s['site_occ'][seen] == N) and np.all(s['site_z'][seen] == N)
        assert np.array_equal(s['site_occ'][unsurveyed], s['site_psi'][unsurveyed])
        assert np.all(s['site_psi'] > 0) and np.all(s['site_psi'] < N)
        worst = np.abs(s['site_z'] - s['site_occ']).max() / N
        print('max |site_z - site_occ| / N:', worst, 'against', 7 / np.sqrt(N))
        assert worst <= 7 / np.sqrt(N)
        assert np.all(s['site_eta2'] * N >= s['site_eta'] ** 2 * (1 - 1e-12))
    eng.close()
    # (every site of that lattice is surveyed) the unsurveyed-site identity on a fixture where a third of the sites is not
    prob, start = _problem_from_golden('ref_queen150_ragged')
    unsurveyed = np.ones(prob.n, dtype=bool)
    unsurveyed[prob.site_id] = False
    assert unsurveyed.sum() == 50
    eng = _engine(prob, [KEY], [start])
    eng.run(60, 10)
    count, s = _read(eng)
    assert count == 50 and np.array_equal(s['site_occ'][unsurveyed], s['site_psi'][unsurveyed])
    assert not np.array_equal(s['site_occ'][~unsurveyed], s['site_psi'][~unsurveyed])
    eng.close()


# ------------------------------------------------------------------ 9: checkpoint
def test_checkpoint_and_restore_keep_the_sums():
    prob, keys, starts = _workload_a(2)
    e1 = _engine(prob, keys, starts)
    r1 = e1.run(20, 5)
    ck = e1.checkpoint()
    assert np.array_equal(ck['site_count'].ravel(), [15, 15]) and ck['site_psi'].shape == (2, prob.n)
    e1.restore(ck)
    r1 = r1 + e1.run(15, 0)
    e2 = _engine(prob, keys, starts)
    r2 = e2.run(20, 5) + e2.run(15, 0)
    s1 = _read_all(e1)
    assert [c for c, _ in s1] == [30, 30]
    _same(s1, _read_all(e2))
    for u, v in zip(r1, r2):
        assert np.array_equal(u, v)
    # switched off, the sums stay readable and no longer move; they may be written only while the switch is on
    e2.site_stats(False)
    e2.run(3, 0)
    _same(s1, _read_all(e2))
    assert e2.get('site_stats')[0] == 0.0
    with pytest.raises(ValueError, match='switched off'):
        e2.set('site_count', 3.0)
    e2.site_stats(True)
    c0, s0 = _read(e2)
    assert c0 == 0 and all(not s0[name].any() for name in SUMS)
    e1.close()
    e2.close()


# ------------------------------------------------------------------ 10: sampler level
def _sampler():
    from occuspytial_amd import LogitICARGibbs
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(30, 40, visits=3, p=2, q=2, random_state=2)
    return LogitICARGibbs(Q, W, X, y, random_state=7), X.shape[0]


def _sites_equal(a, b):
    assert a.n_draws.tolist() == b.n_draws.tolist()
    for name in ('psi', 'occupancy', 'z_mean', 'eta_mean', 'eta_sd'):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for name in a.per_chain:
        assert np.array_equal(a.per_chain[name], b.per_chain[name]), name


def test_sampler_returns_the_site_summary_of_the_kept_draws():
    s, n = _sampler()
    chunked = s.sample(60, burnin=20, chains=3, progressbar=True, site_summaries=True)   # chunks of 16: one straddles the burn-in
    one = _sampler()[0].sample(60, burnin=20, chains=3, progressbar=False, site_summaries=True)
    plain = _sampler()[0].sample(60, burnin=20, chains=3, progressbar=False)
    assert plain.sites is None
    _sites_equal(chunked.sites, one.sites)
    assert one.sites.n_draws.tolist() == [40, 40, 40]
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(one[name], plain[name]) and np.array_equal(chunked[name], plain[name])
    st = one.sites
    assert st.psi.shape == (n,) and st.per_chain['psi'].shape == (3, n)
    assert np.all((st.psi > 0) & (st.psi < 1)) and np.all((st.occupancy >= 0) & (st.occupancy <= 1)) and np.all(st.eta_sd > 0)
    for pooled, name in ((st.psi, 'psi'), (st.occupancy, 'occupancy'), (st.z_mean, 'z_mean'), (st.eta_mean, 'eta_mean')):
        merged = (st.per_chain[name] * 40.0).sum(axis=0) / 120.0       # equal lengths: the merge of the per-chain means
        assert np.max(np.abs(pooled - merged)) <= 1e-14 * max(1.0, np.abs(pooled).max())
    # resume goes on from the checkpoint's sums
    ck = s.checkpoint()
    assert 'site_psi' in ck
    more = s.resume(ck, 30, progressbar=False, site_summaries=True)
    whole = _sampler()[0].sample(90, burnin=20, chains=3, progressbar=False, site_summaries=True)
    assert more.sites.n_draws.tolist() == [70, 70, 70]
    _sites_equal(more.sites, whole.sites)
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(more[name], whole[name][:, 40:])


def test_reduced_rank_sampler_reports_k_theta():
    from occuspytial_amd import LogitRSRGibbs
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(24, 30, visits=3, p=2, q=2, random_state=4)
    out = LogitRSRGibbs(Q, W, X, y, random_state=5, q=40).sample(30, burnin=10, chains=2, progressbar=False, site_summaries=True)
    assert out.sites.n_draws.tolist() == [20, 20] and out.sites.eta_mean.shape == (X.shape[0],)
    assert np.all(np.isfinite(out.sites.eta_sd)) and np.all((out.sites.psi > 0) & (out.sites.psi < 1))


def test_probit_engine_refuses_the_state_names():
    from occuspytial_amd import ProbitRSRGibbs
    from occuspytial_amd._engine import Engine
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(12, 12, visits=3, p=2, q=2, random_state=1)
    s = ProbitRSRGibbs(Q, W, X, y, random_state=1, q=10)
    eng = Engine(s._problem, [KEY])
    for name in ('site_stats', 'site_count') + SUMS:
        with pytest.raises(ValueError, match='not available for the probit model'):
            eng.get(name)
    with pytest.raises(ValueError, match='not available for the probit model'):
        eng.set('site_stats', 1.0)
    eng.close()
