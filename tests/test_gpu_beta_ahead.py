"""The standard normals of beta's draw are drawn one iteration ahead by k_noise (ChainScalars::beta_eps, beside tau's gamma
variate) and read by every beta draw of a running chain: k_z_ob / k_z_ob_stats (p <= 8 on the fused and the launch-per-step
paths), k_beta_draw<0> (p > 8, the generic path).  However a window of iterations opens -- a graph of many, one launch per
MINRES step, one iteration per call, after new start values, after a restore on a fresh engine, in the re-run after a device-side
wait gave up -- its first beta draw must find ITS normals in place: the recorded draws are compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEY = 0x9E3779B97F4A7C15
MODE_KEYS = ('OCC_NO_PERSISTENT', 'OCC_EVENT_SYNC', 'OCC_STREAM_EVENTS', 'OCC_CU_SPLIT', 'OCC_NO_SIDE_STREAM', 'OCC_EAGER_ONLY',
             'OCC_DEBUG_BREAK_HANDOVER')


def _problem(p, lattice=(12, 15)):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(*lattice, visits=3, p=p, q=2, random_state=40 + p)
    return FlatProblem(Q, W, X, y)


def _start(prob, seed):
    rng = np.random.default_rng(seed)
    eta = rng.standard_normal(prob.n)
    return dict(alpha=rng.standard_normal(prob.q), beta=0.3 * rng.standard_normal(prob.p), tau=0.9, eta=eta - eta.mean())


def _engine(prob, chains=2, seed=5, key=KEY):
    from occuspytial_amd._engine import Engine
    eng = Engine(prob, [key + 13 * c for c in range(chains)])
    for c in range(chains):
        eng.set_start(c, **_start(prob, seed + c))
    return eng


def _one_by_one(eng, iters):
    """`iters` calls of one iteration each, the records joined as one call of `iters` returns them."""
    recs = [eng.run(1, 0) for _ in range(iters)]
    return tuple(np.concatenate([r[k] for r in recs], axis=1) for k in range(3))


def _same(u, v):
    for a, b in zip(u, v):
        assert a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize('p', [1, 2, 5, 8, 9])
def test_every_way_a_window_opens_finds_the_normals_of_its_first_beta_draw(monkeypatch, p):
    for k in MODE_KEYS:
        monkeypatch.delenv(k, raising=False)
    prob = _problem(p)
    eng = _engine(prob)
    whole = eng.run(30, 0)
    eng.close()
    assert whole[1].shape == (2, 30, p) and np.all(np.isfinite(whole[1]))
    eng = _engine(prob)
    _same(whole, _one_by_one(eng, 30))
    eng.close()
    monkeypatch.setenv('OCC_NO_PERSISTENT', '1')
    eng = _engine(prob)
    assert eng.stats()['persistent_solve'] == 0
    _same(whole, eng.run(30, 0))
    eng.close()
    eng = _engine(prob)
    _same(whole, _one_by_one(eng, 30))
    eng.close()


@pytest.mark.parametrize('p', [2, 9])
def test_new_start_values_in_mid_run_redraw_the_normals(monkeypatch, p):
    """occ_set_start puts a chain back to iteration 0: the parity slots still hold the normals of the iterations it had reached.
    The continued engine must draw what a fresh engine draws from the same start values and the same z."""
    for k in MODE_KEYS:
        monkeypatch.delenv(k, raising=False)
    prob = _problem(p)
    eng = _engine(prob)
    eng.run(13, 0)                                           # (odd: the chains stand on the other parity)
    z = [eng.get('z', c) for c in range(2)]
    for c in range(2):
        eng.set_start(c, **_start(prob, 70 + c))
    cont = eng.run(12, 0)
    cont1 = eng.run(1, 0)
    eng.close()
    fresh = _engine(prob, seed=70)
    for c in range(2):
        fresh.set('z', z[c], c)
    _same(cont, fresh.run(12, 0))
    _same(cont1, fresh.run(1, 0))
    fresh.close()


@pytest.mark.parametrize('p', [2, 9])
def test_restore_on_a_fresh_engine_continues_with_the_same_beta(monkeypatch, p):
    for k in MODE_KEYS:
        monkeypatch.delenv(k, raising=False)
    prob = _problem(p)
    eng = _engine(prob)
    whole = eng.run(25, 0)
    eng.close()
    eng = _engine(prob)
    head = eng.run(13, 0)
    ckpt = eng.checkpoint()
    eng.close()
    _same(head, tuple(w[:, :13] for w in whole))
    fresh = _engine(prob, seed=90, key=KEY + 1000)           # other keys, other start values: everything comes from the checkpoint
    fresh.run(4, 0)                                          # ... and its slots hold normals of its own
    fresh.restore(ckpt)
    _same(fresh.run(12, 0), tuple(w[:, 13:] for w in whole))
    fresh.close()


def test_rerun_after_a_device_side_wait_gave_up_draws_the_same_beta(monkeypatch):
    """The headline's shape (device-side hand-overs between the two streams); test knob: the side stream never announces its
    noise, the call is re-run from its snapshot without hand-overs.  The uninterrupted run is the same call without the knob."""
    for k in MODE_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('OCC_QUIET', '1')
    prob = _problem(2, lattice=(100, 100))

    def run():
        eng = _engine(prob, chains=4)
        rec = eng.run(5, 0)
        rec2 = eng.run(10, 0)
        st = eng.stats()
        eng.close()
        return rec + rec2, st

    ref, st = run()
    assert st['fused_fallbacks'] == 0 and st['handover_mode'] == 2
    monkeypatch.setenv('OCC_DEBUG_BREAK_HANDOVER', '1')
    alt, st = run()
    assert st['fused_fallbacks'] >= 1
    _same(ref, alt)
