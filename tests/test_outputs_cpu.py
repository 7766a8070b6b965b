"""The z update's optional outputs (occuspytial_amd/csrc/occ_plan.hpp: OUT_*, OUTPUTS, output_level) on the CPU: the bits of
ChainScalars::site_on, the kernel family (level) that serves each, and the level the engine launches for a given OR of
the chains' switches.  The expectations are restated here from include/occ_gibbs.h and the kernels' STATS values; they are
not produced by the functions under test.  Built with g++ on demand (`make plan`, occ_plan_capi.cpp), driven through ctypes."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')

# switch name -> (bit of site_on, STATS value of the family k_z_ob_stats / _ll / _occ / _ppc, available to the probit model)
EXPECTED = {'site_stats': (1, 1, False), 'll_stats': (2, 2, False), 'region_stats': (4, 3, True), 'ppc_stats': (8, 4, False)}


@pytest.fixture(scope='module')
def outputs():
    subprocess.run(['make', '-s', '-C', CSRC, 'plan'], check=True)
    lib = C.CDLL(os.path.join(ROOT, 'build', 'libocc_plan.so'))
    lib.occ_output_count.restype = C.c_int32
    lib.occ_output_row.restype = C.c_uint32
    lib.occ_output_row.argtypes = [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_char_p), C.POINTER(C.c_int32)]
    lib.occ_output_level.restype = C.c_int32
    lib.occ_output_level.argtypes = [C.c_uint32]
    rows = {}
    for k in range(lib.occ_output_count()):
        level, sw, probit = C.c_int32(), C.c_char_p(), C.c_int32()
        bit = lib.occ_output_row(k, C.byref(level), C.byref(sw), C.byref(probit))
        rows[sw.value.decode()] = (bit, level.value, bool(probit.value))
    return rows, lib.occ_output_level


def highest_set_bits_level(word):
    level = 0
    for bit, lv, _ in EXPECTED.values():
        if word & bit:
            level = max(level, lv)
    return level


def test_bits_are_distinct_single_bits(outputs):
    rows, _ = outputs
    bits = sorted(bit for bit, _, _ in rows.values())
    assert bits == [1, 2, 4, 8]
    assert all(b & (b - 1) == 0 for b in bits)
    assert sorted(lv for _, lv, _ in rows.values()) == [1, 2, 3, 4]


def test_names_bits_levels_and_probit(outputs):
    rows, _ = outputs
    assert rows == EXPECTED


def test_names_are_the_headers_switches():
    # include/occ_gibbs.h documents every switch as `name(1) ... the chain's switch, 0 / 1`, in bit order
    text = open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    found = re.findall(r"(\w+)\(1\)\s+the chain's switch, 0 / 1", text)
    assert found == sorted(EXPECTED, key=lambda nm: EXPECTED[nm][0])


@pytest.mark.parametrize('word', range(16))
def test_level_is_the_highest_set_bits(outputs, word):
    _, level = outputs
    assert level(word) == highest_set_bits_level(word)
    assert 0 <= level(word) <= 4 and (level(word) == 0) == (word == 0)


@pytest.mark.parametrize('word', [0x10, 0x13, 0xfffffff0, 0x80000004, 0xffffffff])
def test_unknown_bits_do_not_count(outputs, word):
    _, level = outputs
    assert level(word) == highest_set_bits_level(word & 0xf)
