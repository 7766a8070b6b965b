"""How a call of occ_run lays its graphs (occuspytial_amd/csrc/occ_plan.hpp: GRAPH_SEQ_LONG, graph_len, seq_main_first) on
the CPU, beside tests/test_order_cpu.py.  The expected values are written down from the design: a batch is
cut into replays of the long graph while that many sequences are left, then of the short one, and only the counters'
mode launches its main-stream graph first.  Built with g++ on demand (`make plan`) and driven through ctypes."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')
COUNTERS, RSR_ONE_STREAM, EVENT_NODES, STREAM_EVENTS, ONE_STREAM = range(5)  # occ::SeqMode
SHORT, LONG = 2, 8


@pytest.fixture(scope='module')
def lib():
    subprocess.run(['make', '-s', '-C', CSRC, 'plan'], check=True)
    lib = C.CDLL(os.path.join(ROOT, 'build', 'libocc_plan.so'))
    lib.occ_order_graph_seq_long.restype = C.c_int32
    lib.occ_order_graph_len.restype = C.c_int32
    lib.occ_order_graph_len.argtypes = [C.c_int64, C.c_int32]
    lib.occ_order_main_first.restype = C.c_int32
    lib.occ_order_main_first.argtypes = [C.c_int32]
    lib.occ_order_sequences_per_enqueue.restype = C.c_int32
    lib.occ_order_sequences_per_enqueue.argtypes = [C.c_int32]
    return lib


def _cut(lib, batch, have_long):
    out = []
    while batch > 0:
        out.append(lib.occ_order_graph_len(batch, int(have_long)))
        assert out[-1] > 0
        batch -= out[-1]
    assert batch == 0          # (a batch is a whole number of short graphs: nothing beyond it is enqueued)
    return out


def test_the_long_graph_is_a_whole_number_of_short_ones(lib):
    assert lib.occ_order_graph_seq_long() == LONG
    assert lib.occ_order_sequences_per_enqueue(COUNTERS) == SHORT and LONG % SHORT == 0   # the sequence parity survives a replay


@pytest.mark.parametrize('batch, want', [(2, [2]), (6, [2, 2, 2]), (8, [8]), (10, [8, 2]), (20, [8, 8, 2, 2]), (32, [8] * 4),
                                         (256, [8] * 32)])
def test_a_batch_is_cut_into_long_replays_then_short_ones(lib, batch, want):
    assert _cut(lib, batch, True) == want
    assert _cut(lib, batch, False) == [SHORT] * (batch // SHORT)      # no long pair captured: as before


def test_only_the_counters_mode_launches_its_main_graph_first(lib):
    assert [lib.occ_order_main_first(m) for m in range(5)] == [1, 0, 0, 0, 0]
