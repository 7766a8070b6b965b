"""What a call of occ_run / occ_step decides on the host (occuspytial_amd/csrc/occ_call.hpp: call_head, call_batch,
cap_from_calibration, cap_resize, call_progress, Backoff) on the CPU, beside tests/test_call_order_cpu.py.  The expected
values are written down from the engine as it was before the header existed (run_impl's five branches in front of the first
batch, its batch size, its Krylov cap, its "no progress" exit, and the two back-off counters of try_repromote and
refresh_paths), not from the header.  Built with g++ on demand (`make plan`) and driven through ctypes."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')
RSR, FUSED, CAPTURED = 0, 1, 2                                         # occ::SeqSolve
EAGER, PROLOGUE, CALIBRATE, BUILD = range(4)                           # occ::HeadKind
ARM, FAIL, PASS, DUE = range(4)                                        # occ_call_backoff's operations
NONE = 0xffffffff

# the steps, as {kind, eager sequences, cap from the calibration, with the long pair}
prologue = (PROLOGUE, 0, 0, 0)
realign = single = (EAGER, 1, 0, 0)     # one eager sequence either way: the engine cannot tell them apart
build_cap0 = (BUILD, 0, 0, 0)
build_long = (BUILD, 0, 0, 1)
build_calibrated = (BUILD, 0, 1, 0)


@pytest.fixture(scope='module')
def lib():
    subprocess.run(['make', '-s', '-C', CSRC, 'plan'], check=True)
    lib = C.CDLL(os.path.join(ROOT, 'build', 'libocc_plan.so'))
    lib.occ_call_head.restype = C.c_int32
    lib.occ_call_head.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_int64)]
    lib.occ_call_batch.restype = C.c_int64
    lib.occ_call_batch.argtypes = [C.c_int64] * 3
    lib.occ_call_cap_from_calibration.restype = C.c_int32
    lib.occ_call_cap_from_calibration.argtypes = [C.c_int32, C.c_char_p]
    lib.occ_call_cap_resize.restype = C.c_int32
    lib.occ_call_cap_resize.argtypes = [C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64]
    lib.occ_call_progress.restype = C.c_int32
    lib.occ_call_progress.argtypes = [C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.c_int64, C.POINTER(C.c_int64)]
    lib.occ_call_backoff.restype = C.c_int32
    lib.occ_call_backoff.argtypes = [C.POINTER(C.c_int32), C.c_int32]
    return lib


def head(lib, solve, seq_per_enqueue, n_iter, graph=False, aligned=True, need_prologue=False, eager_only=False):
    out = (C.c_int64 * 12)(*([-1] * 12))
    n = lib.occ_call_head(int(eager_only), solve, seq_per_enqueue, int(graph), int(aligned), n_iter, int(need_prologue), out)
    assert 0 <= n <= 3
    return [tuple(out[4 * i:4 * i + 4]) for i in range(n)]


# ---- the head of a call ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('solve, spe', [(FUSED, 1), (FUSED, 2), (RSR, 2), (CAPTURED, 1)])
@pytest.mark.parametrize('graph', [False, True])
def test_eager_only_steps_the_whole_call_whatever_the_engine(lib, solve, spe, graph):
    assert head(lib, solve, spe, 7, graph=graph, aligned=False, need_prologue=True, eager_only=True) == [(EAGER, 7, 0, 0)]


@pytest.mark.parametrize('n_iter', [1, 2, 20])
def test_fused_with_one_sequence_per_enqueue_builds_before_the_prologue(lib, n_iter):
    assert head(lib, FUSED, 1, n_iter) == [build_cap0]
    assert head(lib, FUSED, 1, n_iter, need_prologue=True) == [build_cap0, prologue]
    assert head(lib, FUSED, 1, n_iter, graph=True) == []
    assert head(lib, FUSED, 1, n_iter, graph=True, need_prologue=True) == [prologue]


@pytest.mark.parametrize('solve', [FUSED, RSR])
@pytest.mark.parametrize('need_prologue', [False, True])
def test_graph_seq_modes_launch_the_prologue_first_then_realign_build_or_step(lib, solve, need_prologue):
    first = [prologue] if need_prologue else []

    def h(n_iter, graph, aligned):
        return head(lib, solve, 2, n_iter, graph=graph, aligned=aligned, need_prologue=need_prologue)
    # a graph whose pair starts with the engine's parity: nothing but the lone step of a one-iteration call
    assert h(20, True, True) == first and h(2, True, True) == first
    assert h(1, True, True) == first + [single]
    # the other parity: one eager sequence realigns, and is the whole of a one-iteration call
    for n_iter in (1, 2, 20):
        assert h(n_iter, True, False) == first + [realign]
    # no graph yet (the parity it was captured at means nothing): the long pair with the short one, unless the call is one step
    for aligned in (False, True):
        assert h(20, False, aligned) == first + [build_long] and h(2, False, aligned) == first + [build_long]
        assert h(1, False, aligned) == first + [single]


@pytest.mark.parametrize('need_prologue', [False, True])     # (the first eager sequence launches it itself)
def test_captured_solve_without_a_graph_calibrates_min_n_iter_3(lib, need_prologue):
    assert head(lib, CAPTURED, 1, 1, need_prologue=need_prologue) == [(CALIBRATE, 1, 0, 0)]
    assert head(lib, CAPTURED, 1, 2, need_prologue=need_prologue) == [(CALIBRATE, 2, 0, 0)]
    assert head(lib, CAPTURED, 1, 3, need_prologue=need_prologue) == [(CALIBRATE, 3, 0, 0)]       # calibration consumed the call: no build
    assert head(lib, CAPTURED, 1, 10, need_prologue=need_prologue) == [(CALIBRATE, 3, 0, 0), build_calibrated]


def test_captured_solve_with_a_graph_has_only_a_pending_prologue(lib):
    assert head(lib, CAPTURED, 1, 10, graph=True) == []
    assert head(lib, CAPTURED, 1, 10, graph=True, need_prologue=True) == [prologue]
    assert head(lib, CAPTURED, 1, 1, graph=True, need_prologue=True) == [prologue]


# ---- the size of a batch -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('left, graph_launches, spe, batch', [(5, 0, 1, 5), (5, 0, 2, 6), (1000, 0, 1, 32), (1000, 127, 2, 32),
                                                              (1000, 128, 2, 256), (100, 128, 1, 100), (33, 128, 2, 34)])
def test_batch(lib, left, graph_launches, spe, batch):
    assert lib.occ_call_batch(left, graph_launches, spe) == batch


# ---- the Krylov cap ----------------------------------------------------------------------------------------------------

def test_cap_from_calibration(lib):
    assert lib.occ_call_cap_from_calibration(0, None) == 4
    assert lib.occ_call_cap_from_calibration(7, None) == 9
    assert lib.occ_call_cap_from_calibration(7, b'0') == 1
    assert lib.occ_call_cap_from_calibration(7, b'12') == 12


def resize(lib, cap, launches):
    """-> None: no change (0: too few solves to decide; `cap`: decided, inside the hysteresis), or the new cap."""
    r = lib.occ_call_cap_resize(cap, sum(launches), sum(k * k for k in launches), len(launches))
    assert r >= 0
    return None if r in (0, cap) else r


def test_cap_resize(lib):
    assert resize(lib, 4, [40] * 31) is None                     # fewer than 32 solves
    assert lib.occ_call_cap_resize(4, 40 * 31, 1600 * 31, 31) == 0   # ... and the counters run on
    assert resize(lib, 9, [10] * 32) == 10 and resize(lib, 12, [10] * 32) == 10     # grow at once; two launches too many
    assert resize(lib, 10, [10] * 32) is None and resize(lib, 11, [10] * 32) is None
    assert lib.occ_call_cap_resize(11, 320, 3200, 32) == 11          # decided: the engine restarts the counters
    assert resize(lib, 4, [8] * 16 + [12] * 16) == 15            # mean 10, sd 2: 10 + 2.5 * 2
    assert resize(lib, 9, [1] * 64) == 4 and resize(lib, 4, [1] * 64) is None       # the floor


# ---- the progress of a batch -------------------------------------------------------------------------------------------

def progress(lib, at, seen, n_iter):
    """at: [(it, koff, it_base)], seen: [(it, koff)] -> (done_min, stuck, seen afterwards)"""
    n = len(at)
    a = (C.c_uint32 * (3 * n))(*[v for row in at for v in row])
    sn = (C.c_uint32 * (2 * n))(*[v for row in seen for v in row])
    done = C.c_int64(-1)
    stuck = lib.occ_call_progress(n, a, sn, n_iter, C.byref(done))
    return done.value, stuck, [(sn[2 * i], sn[2 * i + 1]) for i in range(n)]


def test_done_min_over_chains_at_different_iterations(lib):
    done, stuck, seen = progress(lib, [(112, 0, 100), (107, 3, 100), (540, 0, 520)], [(NONE, NONE)] * 3, 20)
    assert (done, stuck) == (7, -1)
    assert seen == [(112, 0), (107, 3), (540, 0)]


def test_the_first_batch_never_reports(lib):
    # (chains that have not moved at all: a closed window shows at the second batch)
    assert progress(lib, [(100, 0, 100), (100, 0, 100)], [(NONE, NONE)] * 2, 20)[:2] == (0, -1)


def test_a_chain_stuck_at_the_same_it_and_koff_is_reported(lib):
    done, stuck, seen = progress(lib, [(132, 0, 100), (107, 3, 100), (107, 3, 100)], [(112, 0), (107, 3), (107, 3)], 40)
    assert (done, stuck) == (7, 1)                               # the first of the two
    assert seen[0] == (132, 0)                                   # (the chains in front of it are up to date)


def test_the_same_it_with_a_larger_koff_is_progress(lib):
    done, stuck, seen = progress(lib, [(107, 9, 100)], [(107, 3)], 40)
    assert (done, stuck, seen) == (7, -1, [(107, 9)])


def test_a_finished_chain_that_does_not_move_is_not_stuck(lib):
    done, stuck, _ = progress(lib, [(120, 0, 100), (119, 0, 100)], [(120, 0), (118, 0)], 20)
    assert (done, stuck) == (19, -1)
    assert progress(lib, [(120, 0, 100), (120, 0, 100)], [(120, 0), (119, 0)], 20)[:2] == (20, -1)


# ---- the back-off ------------------------------------------------------------------------------------------------------

class Backoff:
    def __init__(self, lib):
        self.lib, self.state = lib, (C.c_int32 * 2)(0, 1)        # (as occ_sampler holds it at creation)

    def op(self, what):
        return self.lib.occ_call_backoff(self.state, what)

    def calls_until_due(self):
        for calls in range(1, 1000):
            if self.op(DUE):
                return calls
        raise AssertionError('never due')

    def failures(self, n):
        """Calls until each of n attempts, every one of them failing."""
        out = []
        for _ in range(n):
            out.append(self.calls_until_due())
            self.op(FAIL)
        return out


def test_promotion_is_tried_after_1_2_4_to_64_calls_and_a_success_starts_over(lib):
    b = Backoff(lib)
    b.op(ARM)                                                    # the fallback
    assert b.failures(8) == [1, 2, 4, 8, 16, 32, 64, 64]
    assert b.calls_until_due() == 64
    b.op(PASS)                                                   # back on the fused path
    b.op(ARM)                                                    # ... and the next fallback
    assert b.failures(3) == [1, 2, 4]


def test_fallback_after_failed_attempts_arms_with_the_step_as_it_is(lib):
    b = Backoff(lib)
    b.op(ARM)
    assert b.failures(3) == [1, 2, 4]
    b.op(ARM)                                                    # (promote_wait = promote_backoff, whatever it was)
    assert b.calls_until_due() == 8


def test_probe_after_a_negative_answer_at_creation(lib):
    b = Backoff(lib)
    b.op(ARM)                                                    # probe_wait = probe_backoff = 1
    assert b.failures(9) == [1, 2, 4, 8, 16, 32, 64, 64, 64]


def test_probe_after_a_first_negative_answer_at_run_time(lib):
    b = Backoff(lib)
    b.op(FAIL)                                                   # forced by the stream generation: doubled before it is armed
    assert b.failures(8) == [2, 4, 8, 16, 32, 64, 64, 64]
    b.op(PASS)                                                   # the streams run beside each other again
    b.op(FAIL)
    assert b.calls_until_due() == 2


def test_a_forced_probe_does_not_consume_the_counter(lib):
    b = Backoff(lib)
    b.op(FAIL)
    b.op(FAIL)                                                   # step 4, four calls to wait
    assert b.op(DUE) == 0 and b.op(DUE) == 0                     # two calls counted
    assert tuple(b.state) == (2, 4)
    b.op(FAIL)                                                   # a forced probe in between (no due()): negative again
    assert tuple(b.state) == (8, 8)                              # armed anew from the step, not from what was left
    assert b.calls_until_due() == 8
