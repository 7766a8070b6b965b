"""The draws of a call (occuspytial_amd/csrc/occ_draws.hpp: DRAWS, draws_lookup, draws_value, draws_length) on the CPU: the
table the engine's host code reads the names, refusals, element types and widths of region_draws, ppc_draws and moran_draws
off.  The expectations are restated here from include/occ_gibbs.h, the kernels' headers and the GPU tests; they are not
produced by the functions under test.  Built with g++ on demand (`make plan`, occ_plan_capi.cpp), driven through ctypes."""
import ctypes as C
import os
import re
import subprocess

import pytest

from ._launch_text import unit_text
from .test_accum_cpu import EXPECTED as ACCUM_EXPECTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')

KINDS = ('region', 'ppc', 'moran')
SWITCH, ROWS, INPUT = range(3)
# kind -> (switch, rows, input), bytes per element, signed, width (0: set by the input), fixed-point columns, the bit of
# site_on (0: a word of the handle), the probit handle has it
EXPECTED = {
    'region': (('region_stats', 'region_draws', 'region_id'), 4, False, 0, 0, 4, True),
    'ppc': (('ppc_stats', 'ppc_draws', None), 8, False, 4, 2, 8, False),
    'moran': (('moran_stats', 'moran_draws', None), 8, True, 8, 8, 0, False),
}
# kind -> its GPU test and, by refusal (not ready, no probit, bad switch, read-only, input locked), the pattern that test
# matches the message with (None: the kind has no such refusal)
GPU_TESTS = {
    'region': ('test_gpu_regions.py', ('set region_id first', None, '0 or 1', 'read-only', 'while a chain has region_stats on')),
    'ppc': ('test_gpu_ppc.py', ('set ppc_stats first', 'posterior predictive checks are not available for the probit model',
                                'ppc_stats is 0 or 1', 'read-only', None)),
    'moran': ('test_gpu_spatial.py', ('set moran_stats first', 'the spatial residual check is not available for the probit model',
                                      'moran_stats is 0 or 1', 'read-only', None)),
}
SITE_NAMES = ('site_stats', 'site_count', 'site_psi', 'site_occ', 'site_z', 'site_eta', 'site_eta2', 'll_stats', 'll_count', 'll_lik', 'll_log', 'll_log2')


@pytest.fixture(scope='module')
def lib():
    subprocess.run(['make', '-s', '-C', CSRC, 'plan'], check=True)
    so = C.CDLL(os.path.join(ROOT, 'build', 'libocc_plan.so'))
    so.occ_draws_count.restype = C.c_int32
    so.occ_draws_row.restype = None
    so.occ_draws_row.argtypes = [C.c_int32, C.c_char_p * 3, C.c_char_p * 5, C.c_int32 * 6]
    so.occ_draws_lookup.restype = C.c_int32
    so.occ_draws_lookup.argtypes = [C.c_char_p, C.POINTER(C.c_int32)]
    so.occ_draws_value.restype = C.c_double
    so.occ_draws_value.argtypes = [C.c_int32, C.c_uint64, C.c_int64]
    so.occ_draws_length.restype = C.c_int64
    so.occ_draws_length.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_int64]
    return so


def row(lib, k):
    names, refusals, num = (C.c_char_p * 3)(), (C.c_char_p * 5)(), (C.c_int32 * 6)()
    lib.occ_draws_row(k, names, refusals, num)
    text = lambda b: None if b is None else b.decode()  # noqa: E731
    return (tuple(text(b) for b in names), num[0], bool(num[1]), num[2], num[3], num[4], bool(num[5])), tuple(text(b) for b in refusals)


def lookup(lib, name):
    field = C.c_int32(-7)
    return lib.occ_draws_lookup(name.encode(), C.byref(field)), field.value


def test_the_table_is_the_three_kinds(lib):
    assert lib.occ_draws_count() == 3
    for k, kind in enumerate(KINDS):
        assert row(lib, k)[0] == EXPECTED[kind], kind
    # the kernels' headers: the widths the table restates (occ_gibbs.hip asserts the same at compile time)
    assert re.search(r'PPC_NCOL = 4 \};', unit_text('occ_kernels.hpp')) and re.search(r'SP_NCOL = 8 \};', unit_text('occ_spatial.hpp'))
    assert re.search(r'OUT_REGION = 4u, OUT_PPC = 8u;', unit_text('occ_plan.hpp'))


def test_every_name_is_found_once_and_no_other(lib):
    seen = {}
    for k, kind in enumerate(KINDS):
        for f, nm in enumerate(EXPECTED[kind][0]):
            if nm is not None:
                assert lookup(lib, nm) == (k, f), nm
                seen[nm] = (k, f)
    assert len(seen) == 7
    accum = [nm for _, names, *_ in ACCUM_EXPECTED.values() for nm in names if nm]
    for nm in accum + list(SITE_NAMES) + ['', 'region', 'region_stat', 'ppc_draws ', 'MORAN_STATS', 'moran', 'eta', 'no_such_name']:
        assert lookup(lib, nm) == (-1, -1), nm


def test_the_three_families_share_no_name():
    from occuspytial_amd import _lib
    families = [{nm for k in table.values() for nm in k.fields} for table in (_lib.SUMS_KINDS, _lib.DRAWS_KINDS, _lib.ACCUM_KINDS)]
    assert [len(f) for f in families] == [12, 7, 10]
    assert families[0] == set(SITE_NAMES)
    for a in range(3):
        for b in range(a + 1, 3):
            assert not families[a] & families[b]


def test_the_binding_equals_the_table(lib):
    from occuspytial_amd import _lib
    assert tuple(_lib.DRAWS_KINDS) == KINDS
    for k, (kind, py) in enumerate(_lib.DRAWS_KINDS.items()):
        names, _, _, width, *_ = row(lib, k)[0]
        assert py.fields == tuple(nm for nm in (names[INPUT],) + names[:INPUT] if nm) and py.input == names[INPUT]
        assert py.fields == {'region': _lib.REGION_FIELDS, 'ppc': _lib.PPC_FIELDS, 'moran': _lib.MORAN_FIELDS}[kind]
        assert py.width == (width or None)
        assert py.on == '_%s_on' % kind
    from occuspytial_amd.gibbs.options import OPTIONS
    rows = {o.draws: o for o in OPTIONS if o.draws}
    assert sorted(rows) == sorted(k.fields[-1] for k in _lib.DRAWS_KINDS.values())
    assert rows['ppc_draws'].width(True) == 4 and rows['moran_draws'].width(True) == 8


def test_what_a_rows_name_returns(lib):
    region, ppc, moran = range(3)
    for raw in (0, 1, 270, 2 ** 32 - 1):                              # a uint32 count: exact, at any column
        assert lib.occ_draws_value(region, raw, 0) == float(raw) and lib.occ_draws_value(region, raw, 6) == float(raw)
    for raw in (0, 1, 3 * 2 ** 32 + 2 ** 31, 2 ** 53 - 1):            # PPC: columns 0 and 1 in 2^-32 quanta, 2 and 3 whole
        for col in range(4):
            assert lib.occ_draws_value(ppc, raw, col) == (raw * 2.0 ** -32 if col < 2 else float(raw)), (raw, col)
    assert lib.occ_draws_value(ppc, 2 ** 53 - 1, 0) * 2.0 ** 32 == 2 ** 53 - 1     # the largest sum below 2^53 quanta: exact
    for raw in (-1, -(5 * 2 ** 32 + 2 ** 30), 7 * 2 ** 32, -(2 ** 53 - 1)):     # Moran: signed, every column in quanta
        for col in (0, 3, 7):
            assert lib.occ_draws_value(moran, raw % 2 ** 64, col) == raw * 2.0 ** -32, (raw, col)
    assert lib.occ_draws_value(moran, (-3 * 2 ** 31) % 2 ** 64, 0) == -1.5
    assert lib.occ_draws_value(ppc, 2 ** 64 - 1, 2) == 2.0 ** 64                  # (unsigned: no sign from the top bit)


def test_lengths(lib):
    n = 270
    assert lib.occ_draws_length(SWITCH, n, 4, 7) == 1 and lib.occ_draws_length(INPUT, n, 4, 7) == n
    assert lib.occ_draws_length(ROWS, n, 4, 7) == 28 and lib.occ_draws_length(ROWS, n, 0, 7) == 0 and lib.occ_draws_length(ROWS, n, 4, 0) == 0
    assert lib.occ_draws_length(ROWS, n, 2 ** 20, 2 ** 13) == 2 ** 33                # (no wrap at 32 bits)


@pytest.mark.parametrize('kind', KINDS)
def test_the_refusals_are_what_the_gpu_tests_expect(lib, kind):
    """The patterns are read from the GPU tests' own text, so the table cannot drift from what they match."""
    file, patterns = GPU_TESTS[kind]
    gpu_test = open(os.path.join(ROOT, 'tests', file)).read()
    refusals = row(lib, KINDS.index(kind))[1]
    for text, pattern in zip(refusals, patterns):
        if pattern is None:
            assert text is None
            continue
        assert "match='%s'" % pattern in gpu_test, pattern
        assert text is not None and re.search(pattern, text), (text, pattern)
    header = re.sub(r'\s*\n \*\s*', ' ', open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read())
    for text in (refusals[1],):                                        # the header quotes the probit refusal
        assert text is None or text in header


def test_the_host_names_them_through_the_table_only():
    """No state name of the three kinds stands as a literal in occ_gibbs.hip: outside comments they come from DRAWS."""
    src = re.sub(r'//[^\n]*', '', unit_text('occ_gibbs.hip'))
    for kind in KINDS:
        for nm in EXPECTED[kind][0][:INPUT]:
            assert nm not in src, nm
    # occ_get_state and occ_set_state ask one router (occ_names.hpp: name_route), which looks a name up here once
    assert len(re.findall(r'\bname_route\(', src)) == 2 and not re.findall(r'\bdraws_lookup\(', src)
    assert len(re.findall(r'\bdraws_lookup\(', re.sub(r'//[^\n]*', '', unit_text('occ_names.hpp')))) == 1
    assert '#include "occ_draws.hpp"' in src
