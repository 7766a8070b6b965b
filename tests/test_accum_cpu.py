"""The accumulators behind the z update (occuspytial_amd/csrc/occ_accum.hpp: ACCUM, accum_words, accum_offset, accum_lookup,
accum_switch_ok, accum_write_refusal) on the CPU: the table the engine's host code, its snapshot loops and its state access
read everything off.  The expectations are restated here from include/occ_gibbs.h and the kernels' headers; they are not
produced by the functions under test.  Built with g++ on demand (`make plan`, occ_plan_capi.cpp), driven through ctypes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')

KINDS = ('hist', 'conv', 'holdout')
# kind -> what messages call it, (switch, count, data, input), bytes per element, slots, slot 0 is the columns' count, the
# switch's range while on
EXPECTED = {
    'hist': ('per-site intervals', ('hist_stats', 'hist_count', 'hist_counts', None), 4, 1, False, (4.0, 1024.0)),
    'conv': ('per-site convergence diagnostics', ('conv_stats', 'conv_count', 'conv_sums', None), 8, 11, True, (1.0, 2.0 ** 30)),
    'holdout': ('held-out scoring', ('holdout_stats', 'holdout_count', 'holdout_sums', 'holdout_data'), 8, 5, True, (1.0, 1.0)),
}
# kind -> not ready, bad switch, bad count, bad data: what tests/test_gpu_*.py::test_refusals match
REFUSALS = {
    'hist': ('per-site intervals have not been switched on for this handle (set hist_stats first)',
             'hist_stats is 0 or a number of bins from 4 to 1024',
             'hist_count and hist_counts are whole numbers in [0, 2^32)', 'hist_count and hist_counts are whole numbers in [0, 2^32)'),
    'conv': ('per-site convergence diagnostics have not been switched on for this handle (set conv_stats first)',
             'conv_stats is 0 or a batch length from 1 to 2^30',
             'conv_count is a whole number >= 0', 'the cnt slot of conv_sums holds one whole number >= 0 at every site'),
    'holdout': ('no held-out data have been set for this handle (set holdout_data first)', 'holdout_stats is 0 or 1',
                'holdout_count is a whole number >= 0', 'the cnt slot of holdout_sums holds one whole number >= 0 at every entry'),
}
SWITCH, COUNT, DATA, INPUT = range(4)


@pytest.fixture(scope='module')
def lib():
    subprocess.run(['make', '-s', '-C', CSRC, 'plan'], check=True)
    so = C.CDLL(os.path.join(ROOT, 'build', 'libocc_plan.so'))
    so.occ_accum_count.restype = C.c_int32
    so.occ_accum_row.restype = None
    so.occ_accum_row.argtypes = [C.c_int32, C.POINTER(C.c_char_p), C.c_char_p * 4, C.c_char_p * 4, C.c_int32 * 3, C.c_double * 2]
    so.occ_accum_words.restype = C.c_int64
    so.occ_accum_words.argtypes = [C.c_int32, C.c_int64, C.c_int64]
    so.occ_accum_offset.restype = C.c_int64
    so.occ_accum_offset.argtypes = [C.c_int64] * 4
    so.occ_accum_lookup.restype = C.c_int32
    so.occ_accum_lookup.argtypes = [C.c_char_p, C.POINTER(C.c_int32)]
    so.occ_accum_switch_ok.restype = C.c_int32
    so.occ_accum_switch_ok.argtypes = [C.c_int32, C.c_double]
    so.occ_accum_write_refusal.restype = C.c_char_p
    so.occ_accum_write_refusal.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int64, C.c_int64]
    return so


def row(lib, k):
    what, names, refusals, num, rng = C.c_char_p(), (C.c_char_p * 4)(), (C.c_char_p * 4)(), (C.c_int32 * 3)(), (C.c_double * 2)()
    lib.occ_accum_row(k, C.byref(what), names, refusals, num, rng)
    text = lambda b: None if b is None else b.decode()  # noqa: E731
    return (what.value.decode(), tuple(text(b) for b in names), num[0], num[1], bool(num[2]), (rng[0], rng[1])), tuple(text(b) for b in refusals)


def refusal(lib, k, field, values, unit):
    v = np.ascontiguousarray(values, dtype=np.float64)
    got = lib.occ_accum_write_refusal(k, field, v.ctypes.data_as(C.POINTER(C.c_double)), v.size, unit)
    return None if got is None else got.decode()


def test_the_table_is_the_three_kinds_in_launch_order(lib):
    assert lib.occ_accum_count() == 3
    for k, kind in enumerate(KINDS):
        got, refusals = row(lib, k)
        assert got == EXPECTED[kind], kind
        assert refusals == REFUSALS[kind], kind


def test_the_table_agrees_with_the_binding_and_the_headers(lib):
    from occuspytial_amd import _lib
    header = re.sub(r'\s*\n \*\s*', ' ', open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read())
    assert tuple(_lib.ACCUM_KINDS) == KINDS
    per_column = {'hist': r'4 B bytes per site and chain', 'conv': r'88 bytes per site and chain', 'holdout': r'40 bytes per entry and chain'}
    length = {'hist': 'B n', 'conv': '11 n', 'holdout': '5 H'}
    span = {'hist': '4 <= B <= 1024', 'conv': '1 <= L <= 2^30', 'holdout': 'a word of the handle per chain, 0 or 1'}
    for kind, py in _lib.ACCUM_KINDS.items():
        what, names, elem, slots, _, _ = EXPECTED[kind]
        assert py.fields == tuple(nm for nm in (names[INPUT],) + names[:INPUT] if nm) and py.input == names[INPUT]
        assert py.fields == {'hist': _lib.HIST_FIELDS, 'conv': _lib.CONV_FIELDS, 'holdout': _lib.HOLDOUT_FIELDS}[kind]
        assert py.slots == slots and np.dtype(py.dtype).itemsize == elem
        assert py.shape[0] == (slots if slots > 1 else -1)
        # include/occ_gibbs.h: the names with their lengths, the bytes per column (slots x element), the range, the probit refusal
        assert '%s(%s)' % (names[DATA], length[kind]) in header and '%s(1)' % names[SWITCH] in header and '%s(1)' % names[COUNT] in header
        assert per_column[kind] in header and span[kind] in header
        assert elem * slots == int(per_column[kind].split()[0])          # (the histograms: 4 bytes per bin, B of them)
        assert '"%s %s not available for the probit model"' % (what, 'is' if kind == 'holdout' else 'are') in header
    # the kernels' headers: the constants the table restates (occ_gibbs.hip asserts the same at compile time)
    assert re.search(r'constexpr int HIST_BINS_MIN = 4, HIST_BINS_MAX = 1024;', open(os.path.join(CSRC, 'occ_hist.hpp')).read())
    conv = open(os.path.join(CSRC, 'occ_conv.hpp')).read()
    assert re.search(r'constexpr int CONV_SLOTS = 11;', conv) and re.search(r'constexpr int CONV_BATCH_MAX = 1 << 30;', conv)
    assert re.search(r'constexpr int HOLD_SLOTS = 5;', open(os.path.join(CSRC, 'occ_holdout.hpp')).read())


def test_every_name_is_found_once_and_no_other(lib):
    seen = {}
    for k, kind in enumerate(KINDS):
        for f, nm in enumerate(EXPECTED[kind][1]):
            if nm is None:
                continue
            field = C.c_int32(-7)
            assert lib.occ_accum_lookup(nm.encode(), C.byref(field)) == k and field.value == f
            seen[nm] = (k, f)
    assert len(seen) == 10
    for nm in ('', 'hist', 'hist_stat', 'hist_stats ', 'conv_sum', 'holdout', 'site_stats', 'moran_stats', 'HIST_STATS', 'eta'):
        field = C.c_int32(-7)
        assert lib.occ_accum_lookup(nm.encode(), C.byref(field)) == -1 and field.value == -1


@pytest.mark.parametrize('chains', [1, 3])
@pytest.mark.parametrize('kind', KINDS)
def test_parts_lie_where_the_reshape_puts_them(lib, kind, chains):
    """unit is no multiple of 64.  The buffer as the kernels index it -- [C][B][n] for the histograms (occ_hist.hpp: cnt[(c B + b)
    n + i]), [slots][C][unit] for the others (slot-major, [slot][c unit + i]) -- holds its own flat index; every (slot, chain)
    part must start where numpy finds it, and the parts must tile the buffer without overlap."""
    k = KINDS.index(kind)
    slots = EXPECTED[kind][3]
    B, n = 5, 37
    unit = B * n if kind == 'hist' else n            # 185 and 37
    words = lib.occ_accum_words(k, chains, unit)
    assert words == slots * chains * unit
    flat = np.arange(words)
    shaped = flat.reshape(chains, B, n) if kind == 'hist' else flat.reshape(slots, chains, unit)
    covered = np.zeros(words, dtype=np.int64)
    for slot in range(slots):
        for c in range(chains):
            at = lib.occ_accum_offset(chains, unit, slot, c)
            want = shaped[c].ravel() if kind == 'hist' else shaped[slot, c]
            assert 0 <= at and at + unit <= words
            assert np.array_equal(flat[at:at + unit], want), (slot, c)
            covered[at:at + unit] += 1
    assert np.all(covered == 1)


def test_offsets_do_not_wrap_at_32_bits(lib):
    C_, unit = 64, 1024 * 100_000                    # one chain's histograms of 1024 bins at 100 000 sites
    assert lib.occ_accum_offset(C_, unit, 0, 63) == 63 * unit > 2 ** 32
    assert lib.occ_accum_offset(C_, unit // 1024, 10, 63) == 10 * C_ * (unit // 1024) + 63 * (unit // 1024)
    assert lib.occ_accum_words(1, C_, 100_000_000) == 11 * 64 * 100_000_000 > 2 ** 32


@pytest.mark.parametrize('kind', KINDS)
def test_switch_values(lib, kind):
    k = KINDS.index(kind)
    lo, hi = EXPECTED[kind][5]
    for v in (0.0, lo, hi, float(int((lo + hi) // 2))):
        assert lib.occ_accum_switch_ok(k, v) == 1, v
    for v in (-1.0, lo - 1.0 if lo > 1.0 else 0.5, hi + 1.0, lo + 0.5, float('nan'), float('inf'), -0.5):
        assert lib.occ_accum_switch_ok(k, v) == 0, v


def test_hist_writes_hold_whole_numbers_below_2_to_the_32(lib):
    k, unit = 0, 6
    bad = REFUSALS['hist'][2]
    assert refusal(lib, k, COUNT, [0.0], unit) is None and refusal(lib, k, COUNT, [2.0 ** 32 - 1], unit) is None
    for v in (-1.0, 0.5, 2.0 ** 32, 2.0 ** 53, float('nan')):
        assert refusal(lib, k, COUNT, [v], unit) == bad
    good = np.array([0.0, 1.0, 7.0, 2.0 ** 32 - 1, 3.0, 3.0])       # (unequal columns are what histograms are)
    assert refusal(lib, k, DATA, good, unit) is None
    for at in range(unit):                                          # every element is bound, the last one too
        for v in (-1.0, 0.5, 2.0 ** 32):
            data = good.copy()
            data[at] = v
            assert refusal(lib, k, DATA, data, unit) == bad, (at, v)


@pytest.mark.parametrize('kind', ['conv', 'holdout'])
def test_sum_writes_bind_the_count_and_the_cnt_slot_only(lib, kind):
    k, unit = KINDS.index(kind), 7
    slots = EXPECTED[kind][3]
    _, _, bad_count, bad_data = REFUSALS[kind]
    assert refusal(lib, k, COUNT, [0.0], unit) is None and refusal(lib, k, COUNT, [2.0 ** 53 - 1], unit) is None
    assert refusal(lib, k, COUNT, [2.0 ** 32], unit) is None                     # (a float64 count goes past 32 bits)
    for v in (-1.0, 0.5, 2.0 ** 53, float('nan')):
        assert refusal(lib, k, COUNT, [v], unit) == bad_count
    rng = np.random.default_rng(5)
    good = rng.standard_normal(slots * unit) * 1e3                               # the other slots hold any float64
    good[:unit] = 12.0
    good[unit] = -0.5
    assert refusal(lib, k, DATA, good, unit) is None
    for at in range(unit):
        for v in (-1.0, 0.5, 2.0 ** 53, 13.0):                                   # 13: whole, but not the other columns' count
            data = good.copy()
            data[at] = v
            assert refusal(lib, k, DATA, data, unit) == bad_data, (at, v)
    for v in (-1.0, 0.5, 2.0 ** 53):                                             # equal at every column is not enough
        data = good.copy()
        data[:unit] = v
        assert refusal(lib, k, DATA, data, unit) == bad_data
    data = good.copy()
    data[:unit] = 2.0 ** 32
    assert refusal(lib, k, DATA, data, unit) is None
