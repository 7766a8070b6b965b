"""The order of a launch sequence and the engine's scheduling modes (occuspytial_amd/csrc/occ_plan.hpp: seq_mode,
seq_launches, seq_parts) on the CPU.  The engine walks these descriptions and names no kernel itself, so what is pinned
here is what it launches.  The expected lists were written down by reading the engine's hand-written launch code as it was
before the descriptions existed (build_graph, eager_sequence, enqueue_sequence); they are not produced by the functions
under test.  Built with g++ on demand (`make plan`, occ_plan_capi.cpp) and driven through ctypes."""
import ctypes as C
import itertools
import os
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')

# occ::Kind -- occ_profile's indices, then the internal kinds
(OMEGA_B, NOISE, ETA_INIT, MINRES, BETA_PARTIAL, OMEGA_A, ALPHA_DRAW, Z_OB, ITER, GATE, RSR_GRAM, RSR_SOLVE,
 RSR_ETA_BETA) = range(13)
COUNTERS, RSR_ONE_STREAM, EVENT_NODES, STREAM_EVENTS, ONE_STREAM = range(5)  # occ::SeqMode
S_RSR, S_FUSED, S_CAPTURED, S_EAGER = range(4)                               # occ::SeqSolve
MAIN, SIDE, BEHIND, EAGER = range(4)                                         # occ::SeqWhere; 3: an eager sequence
WAIT, RECORD = -1, -2            # event nodes, as occ_order_launches reports them
HOST_WATCHED, K_LAST = -1, -2    # extras of an eager per-step solve: the host-watched stretch, its last launch's number
GRAPH_SEQ = 2


@pytest.fixture(scope='module')
def order():
    subprocess.run(['make', '-s', '-C', CSRC, 'plan'], check=True)
    lib = C.CDLL(os.path.join(ROOT, 'build', 'libocc_plan.so'))
    lib.occ_order_mode.restype = C.c_int32
    lib.occ_order_mode.argtypes = [C.c_int32] * 5
    lib.occ_order_sequences_per_enqueue.restype = C.c_int32
    lib.occ_order_sequences_per_enqueue.argtypes = [C.c_int32]
    lib.occ_order_launches.restype = C.c_int32
    lib.occ_order_launches.argtypes = [C.c_int32] * 6 + [C.POINTER(C.c_int32), C.c_int32]

    def launches(mode, where, solve, p=0, cap=0, gate_kernel=False):
        out = (C.c_int32 * (3 * 64))()
        n = lib.occ_order_launches(mode, where, solve, p, cap, int(gate_kernel), out, 64)
        assert n >= 0
        return [tuple(out[3 * i:3 * i + 3]) for i in range(n)]
    launches.mode = lib.occ_order_mode
    launches.per_enqueue = lib.occ_order_sequences_per_enqueue
    return launches


# (flag_sync, rsr, event_nodes, side_enabled) -> mode: counters > reduced rank > event nodes > stream events > one stream
MODES = {
    (0, 0, 0, 0): ONE_STREAM, (0, 0, 0, 1): STREAM_EVENTS, (0, 0, 1, 0): EVENT_NODES, (0, 0, 1, 1): EVENT_NODES,
    (0, 1, 0, 0): RSR_ONE_STREAM, (0, 1, 0, 1): RSR_ONE_STREAM, (0, 1, 1, 0): RSR_ONE_STREAM, (0, 1, 1, 1): RSR_ONE_STREAM,
    (1, 0, 0, 0): COUNTERS, (1, 0, 0, 1): COUNTERS, (1, 0, 1, 0): COUNTERS, (1, 0, 1, 1): COUNTERS,
    (1, 1, 0, 0): COUNTERS, (1, 1, 0, 1): COUNTERS, (1, 1, 1, 0): COUNTERS, (1, 1, 1, 1): COUNTERS,
}


@pytest.mark.parametrize('flags', sorted(MODES))
def test_mode_of_every_flag_combination(order, flags):
    assert order.mode(*flags, S_RSR if flags[1] else S_FUSED) == MODES[flags]


def test_sequences_per_enqueue(order):
    assert [order.per_enqueue(m) for m in range(5)] == [GRAPH_SEQ, GRAPH_SEQ, 1, 1, 1]


@pytest.mark.parametrize('solve', [S_CAPTURED, S_EAGER])
def test_counters_without_a_one_launch_solve_are_refused(order, solve):
    for rest in itertools.product((0, 1), repeat=2):
        assert order.mode(1, 0, *rest, solve) == -1
    assert order.mode(1, 0, 1, 1, S_FUSED) == COUNTERS and order.mode(1, 1, 1, 1, S_RSR) == COUNTERS
    assert order.mode(0, 0, 1, 1, solve) == EVENT_NODES  # (every other mode holds a per-step solve)


def side(e, gate=0):  # plain; gate 1: in the head of k_omega_a; gate 2: as a kernel
    return ([(GATE, 0, 0)] if gate == 2 else []) + [(OMEGA_A, e, 1 if gate == 1 else 0), (NOISE, e, 1)]


def solve_of(shape, e, cap=4):
    if shape == S_RSR:
        return [(RSR_GRAM, e, 0), (RSR_SOLVE, e, 0), (RSR_ETA_BETA, e, 0)]
    if shape == S_FUSED:
        return [(ITER, e, 0)]
    if shape == S_EAGER:
        return [(ETA_INIT, e, 0), (MINRES, e, HOST_WATCHED), (BETA_PARTIAL, e, K_LAST)]
    return [(ETA_INIT, e, 0)] + [(MINRES, e, k) for k in range(1, cap + 4)] + [(BETA_PARTIAL, e, cap + 3)]


def test_the_captured_per_step_solve_written_out(order):
    assert order(STREAM_EVENTS, MAIN, S_CAPTURED, p=1, cap=4) == [
        (ETA_INIT, 1, 0), (MINRES, 1, 1), (MINRES, 1, 2), (MINRES, 1, 3), (MINRES, 1, 4), (MINRES, 1, 5), (MINRES, 1, 6),
        (MINRES, 1, 7), (BETA_PARTIAL, 1, 7)]


@pytest.mark.parametrize('p', [0, 1])
def test_counters_graphs(order, p):
    q = p ^ 1
    assert order(COUNTERS, MAIN, S_FUSED, p) == [(ITER, p, 0), (Z_OB, p, 0), (ITER, q, 0), (Z_OB, q, 0)]
    assert order(COUNTERS, MAIN, S_RSR, p) == [
        (RSR_GRAM, p, 0), (RSR_SOLVE, p, 0), (RSR_ETA_BETA, p, 0), (Z_OB, p, 0),
        (RSR_GRAM, q, 0), (RSR_SOLVE, q, 0), (RSR_ETA_BETA, q, 0), (Z_OB, q, 0)]
    for solve in (S_FUSED, S_RSR):
        assert order(COUNTERS, SIDE, solve, p) == [(OMEGA_A, p, 1), (NOISE, p, 1), (OMEGA_A, q, 1), (NOISE, q, 1)]
        assert order(COUNTERS, SIDE, solve, p, gate_kernel=True) == [
            (GATE, 0, 0), (OMEGA_A, p, 0), (NOISE, p, 1), (GATE, 0, 0), (OMEGA_A, q, 0), (NOISE, q, 1)]
        assert order(COUNTERS, BEHIND, solve, p) == []


@pytest.mark.parametrize('p', [0, 1])
def test_reduced_rank_one_stream_graph(order, p):
    q = p ^ 1
    assert order(RSR_ONE_STREAM, MAIN, S_RSR, p) == [
        (OMEGA_A, p, 0), (NOISE, p, 1), (RSR_GRAM, p, 0), (RSR_SOLVE, p, 0), (RSR_ETA_BETA, p, 0), (Z_OB, p, 0),
        (OMEGA_A, q, 0), (NOISE, q, 1), (RSR_GRAM, q, 0), (RSR_SOLVE, q, 0), (RSR_ETA_BETA, q, 0), (Z_OB, q, 0)]
    assert order(RSR_ONE_STREAM, SIDE, S_RSR, p) == [] and order(RSR_ONE_STREAM, BEHIND, S_RSR, p) == []
    # (the gate is the counters' alone)
    assert order(RSR_ONE_STREAM, MAIN, S_RSR, p, gate_kernel=True) == order(RSR_ONE_STREAM, MAIN, S_RSR, p)


@pytest.mark.parametrize('p', [0, 1])
@pytest.mark.parametrize('solve', [S_FUSED, S_CAPTURED])
def test_per_parity_graphs(order, solve, p):
    head = solve_of(solve, p, cap=4)
    assert order(EVENT_NODES, MAIN, solve, p, cap=4) == head + [(WAIT, p, 0), (Z_OB, p, 0), (RECORD, p, 0)]
    assert order(EVENT_NODES, SIDE, solve, p, cap=4) == [(WAIT, p, 0), (OMEGA_A, p, 0), (NOISE, p, 1), (RECORD, p, 0)]
    assert order(EVENT_NODES, BEHIND, solve, p, cap=4) == []
    for mode in (STREAM_EVENTS, ONE_STREAM):
        assert order(mode, MAIN, solve, p, cap=4) == head
        assert order(mode, SIDE, solve, p, cap=4, gate_kernel=True) == [(OMEGA_A, p, 0), (NOISE, p, 1)]
        assert order(mode, BEHIND, solve, p, cap=4) == [(Z_OB, p, 0)]


@pytest.mark.parametrize('p', [0, 1])
@pytest.mark.parametrize('mode', range(5))
def test_eager_sequence_is_side_solve_tail_in_every_mode(order, mode, p):
    assert order(mode, EAGER, S_FUSED, p) == [(OMEGA_A, p, 0), (NOISE, p, 1), (ITER, p, 0), (Z_OB, p, 0)]
    assert order(mode, EAGER, S_EAGER, p, gate_kernel=True) == [
        (OMEGA_A, p, 0), (NOISE, p, 1), (ETA_INIT, p, 0), (MINRES, p, HOST_WATCHED), (BETA_PARTIAL, p, K_LAST), (Z_OB, p, 0)]
    assert order(mode, EAGER, S_RSR, p) == [
        (OMEGA_A, p, 0), (NOISE, p, 1), (RSR_GRAM, p, 0), (RSR_SOLVE, p, 0), (RSR_ETA_BETA, p, 0), (Z_OB, p, 0)]


# every mode with the shapes of solve it can hold
HOLDS = [(COUNTERS, S_RSR), (COUNTERS, S_FUSED), (RSR_ONE_STREAM, S_RSR)] + \
    [(m, sv) for m in (EVENT_NODES, STREAM_EVENTS, ONE_STREAM) for sv in (S_FUSED, S_CAPTURED)]


@pytest.mark.parametrize('gate_kernel', [False, True])
@pytest.mark.parametrize('p', [0, 1])
@pytest.mark.parametrize('mode,solve', HOLDS)
def test_invariants_of_every_mode(order, mode, solve, p, gate_kernel):
    n_seq = order.per_enqueue(mode)
    where = {w: order(mode, w, solve, p, cap=3, gate_kernel=gate_kernel) for w in (MAIN, SIDE, BEHIND)}
    eager = Counter(k for k, _, _ in order(mode, EAGER, solve, p, cap=3))
    # (an eager per-step solve has the same kinds as a captured one)
    assert set(eager) == {k for k, _, _ in order(mode, EAGER, S_EAGER if solve == S_CAPTURED else solve, p)}
    for t in range(n_seq):
        seq = {w: l[t * len(l) // n_seq:(t + 1) * len(l) // n_seq] for w, l in where.items()}
        launches = {w: [x for x in l if x[0] >= 0] for w, l in seq.items()}
        # the parities of consecutive sequences alternate from p (the gate takes none)
        assert {e for l in launches.values() for k, e, _ in l if k != GATE} == {p ^ (t & 1)}
        # exactly one k_z_ob, the last launch on the main stream
        main = launches[MAIN] + launches[BEHIND]
        assert [k for k, _, _ in main].count(Z_OB) == 1 and main[-1][0] == Z_OB
        assert all(k != Z_OB for k, _, _ in launches[SIDE])
        # k_omega_a before k_noise on the stream that holds them, and the noise is the coming iteration's
        for l in launches.values():
            kinds = [k for k, _, _ in l]
            assert (OMEGA_A in kinds) == (NOISE in kinds)
            if OMEGA_A in kinds:
                assert kinds.index(OMEGA_A) < kinds.index(NOISE) and l[kinds.index(NOISE)][2] == 1
        # together the streams launch what an eager sequence launches, apart from the gate
        assert Counter(k for l in launches.values() for k, _, _ in l if k != GATE) == eager
    # the gate exists with the counters alone, once per sequence, in one of its two forms
    gates = [x for x in where[SIDE] if x[0] == GATE], [x for x in where[SIDE] if x[0] == OMEGA_A and x[2] == 1]
    if mode == COUNTERS:
        assert (len(gates[0]), len(gates[1])) == ((n_seq, 0) if gate_kernel else (0, n_seq))
    else:
        assert gates == ([], [])
