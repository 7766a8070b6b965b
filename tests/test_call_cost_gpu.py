"""What a call of occ_run does around its iterations -- the order of its first launches, the long and the short captured
graphs a batch is cut into, the record buffer's floor, the end-of-call read behind a device-side join of the two streams --
never changes a bit: however 20 iterations are split into calls, the rows, the state and the Krylov count are the same, with
an optional output on as well, after a call whose window stayed closed, and when the call is re-run after a run-time fallback.

Shape: the smallest lattice (12 x 12 queen, 3 visits, p = q = 2, 2 chains) at which the fused one-XCD form, the side stream
with device-side hand-overs and the captured graphs are all in play; the next sizes are tried if the planner picks another
form there.  Every comparison is bitwise: the variates are functions of (key, iteration, index)."""
import numpy as np
import pytest

from ._outputs_gpu import engine_with
from ._outputs_gpu import time_limit as _time_limit  # noqa: F401  (autouse in this module)
from .test_gpu_parity import KEY

pytestmark = pytest.mark.gpu

SPLITS = ((20,), (7, 13), (1, 1, 18))   # odd parities between calls, the realignment sequence, a one-iteration call
SUMS = ('site_psi', 'site_occ', 'site_z', 'site_eta', 'site_eta2')
CHAINS = 2


def _workload(rows, cols):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(rows, cols, visits=3, p=2, q=2, random_state=1)
    prob = FlatProblem(Q, W, X, y)
    rng = np.random.default_rng(5)
    starts = []
    for _ in range(CHAINS):
        eta = rng.standard_normal(prob.n)
        starts.append(dict(eta=eta - eta.mean(), alpha=rng.standard_normal(2), beta=rng.standard_normal(2), tau=1.0))
    return prob, [KEY + 13 * c for c in range(CHAINS)], starts


@pytest.fixture(scope='module')
def workload():
    """The smallest of these lattices whose engine runs k_iter with one XCD per chain and hands over through the counters."""
    for rows, cols in ((12, 12), (16, 16), (24, 24), (32, 32), (40, 45)):
        w = _workload(rows, cols)
        eng = engine_with(*w)
        st = eng.stats()
        eng.close()
        if st['persistent_solve'] == 2 and st['handover_mode'] == 2:
            return w
    pytest.fail('no lattice up to 40 x 45 runs the fused one-XCD form with device-side hand-overs: %r' % (st,))


def _state(eng, site):
    out = [np.concatenate([eng.get('eta', c), eng.get('z', c)]) for c in range(CHAINS)]
    if site:
        out += [eng.get('site_count', c) for c in range(CHAINS)]
        out += [eng.get(name, c) for c in range(CHAINS) for name in SUMS]
    return out


def _run_split(eng, ckpt, split, site):
    """-> rows (alpha, beta, tau of all the calls joined), state after the last call, Krylov iterations of the calls."""
    eng.restore(ckpt)
    k0 = eng.stats()['krylov_total']
    parts = [eng.run(n, 0) for n in split]
    rows = [np.concatenate(x, axis=1) for x in zip(*parts)]
    assert rows[0].shape[1] == sum(split)
    return rows, _state(eng, site), eng.stats()['krylov_total'] - k0


def _assert_same(a, b):
    assert len(a) == len(b)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.parametrize('site', [False, True], ids=['plain', 'site_stats'])
def test_twenty_iterations_are_the_same_however_they_are_split_into_calls(workload, site):
    """From one checkpoint: one call of 20 against 7 + 13 and 1 + 1 + 18 -- rows, eta, z and the Krylov total, bit for bit; with
    the per-site sums on (whose snapshot copies stand in front of the call's first kernel) the sums and their counts too."""
    eng = engine_with(*workload, site=site)
    eng.run(5, 1)                                   # graphs captured; the chains and the sums are somewhere
    st = eng.stats()
    assert st['persistent_solve'] == 2 and st['handover_mode'] == 2
    ckpt = eng.checkpoint()
    ref = _run_split(eng, ckpt, SPLITS[0], site)
    assert ref[2] > 0 and all(np.all(np.isfinite(r)) for r in ref[0])
    for split in SPLITS[1:] + SPLITS[:1]:           # (the one call again, now behind calls that left an odd parity)
        got = _run_split(eng, ckpt, split, site)
        _assert_same(ref[0], got[0])
        _assert_same(ref[1], got[1])
        assert ref[2] == got[2], (split, ref[2], got[2])
    assert eng.stats()['fused_fallbacks'] == 0
    eng.close()


def test_a_closed_window_then_normal_calls(workload):
    """``debug_close_window`` then a normal call: the closed call ends with 'no progress' and changes nothing (what
    test_a_closed_window_ends_the_call_with_the_state_it_saw expects), and the calls after it are bit-equal to an undisturbed
    engine's."""
    from occuspytial_amd._lib import EngineUnavailable
    ref = engine_with(*workload)
    want = [ref.run(9, 0), ref.run(20, 3), ref.run(6, 0)]
    want_state = _state(ref, False)
    ref.close()
    eng = engine_with(*workload)
    got = [eng.run(9, 0)]
    eng.set('debug_close_window', 1.0)
    with pytest.raises(EngineUnavailable, match='no progress') as ei:
        eng.run(20, 3)
    assert '{9, 0 |' in str(ei.value), str(ei.value)
    got += [eng.run(20, 3), eng.run(6, 0)]
    st = eng.stats()
    assert st['fused_fallbacks'] == 0 and st['iterations'] == 35
    for w, g in zip(want, got):
        _assert_same(w, g)
    _assert_same(want_state, _state(eng, False))
    eng.close()


def test_a_fallback_in_the_middle_of_a_call_reruns_to_the_same_bits(workload, monkeypatch):
    """The broken hand-over word (OCC_DEBUG_BREAK_HANDOVER): the side stream never announces its noise, the second iteration
    of the 20-step call gives up, and the call is re-run from its snapshot on the path without device-side waits -- same
    rows, state and per-site sums as an undisturbed engine, through the same end-of-call read."""
    monkeypatch.setenv('OCC_QUIET', '1')
    ref = engine_with(*workload, site=True)
    want = ref.run(20, 0)
    want_state = _state(ref, True)
    ref.close()
    monkeypatch.setenv('OCC_DEBUG_BREAK_HANDOVER', '1')
    eng = engine_with(*workload, site=True)
    got = eng.run(20, 0)
    assert eng.stats()['fused_fallbacks'] == 1
    _assert_same(want, got)
    _assert_same(want_state, _state(eng, True))
    eng.close()
