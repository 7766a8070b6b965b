"""Registers, scratch and occupancy of k_z_ob_occ and k_pb_z_occ, the z updates that count the occupied sites per region,
as the compiler reports them for gfx950 (no GPU needed; the helpers and the session's one compilation are those of
test_kernel_resources_cpu.py).  Conditions on the generated code, not measurements of speed:

  k_z_ob_occ<P>, P = 1, 2   what k_z_ob<P>, k_z_ob_stats<P> and k_z_ob_ll<P> are held to: no scratch, no spilled vector
                            register, three waves per SIMD
  k_z_ob_occ<3 .. 8>        no more scratch or spilled vector registers than k_z_ob_ll<P> of the same build, three waves per SIMD
  k_pb_z_occ                no scratch
  every other kernel        the SGPRs, VGPRs, AGPRs, scratch, spills, LDS and occupancy it had before the family was added: the
                            committed listing profiles/regions_resource_usage.txt holds them (its lines without NEW are the
                            parent build's values, symbol for symbol), and this build must reproduce every line
"""
import os
import re

import pytest

from .test_kernel_resources_cpu import ROOT, kernel, usage  # noqa: F401  (the session-scoped compilation)

LISTING = os.path.join(ROOT, 'profiles', 'regions_resource_usage.txt')
COLUMNS = {'SGPRs': 'sgprs', 'VGPRs': 'vgprs', 'AGPRs': 'agprs', 'ScratchSize [bytes/lane]': 'scratch', 'VGPRs Spill': 'vgpr_spill',
           'SGPRs Spill': 'sgpr_spill', 'LDS Size [bytes/block]': 'lds', 'Occupancy [waves/SIMD]': 'occupancy'}


def read_listing():
    """-> ({symbol: {field: int}} of every line, the set of symbols marked NEW, the header's three counts)."""
    rows, new, head = {}, set(), None
    for line in open(LISTING):
        if line.startswith('#'):
            m = re.search(r'Parent build: (\d+) kernel symbols; this build: (\d+)\..*differ: (\d+)\.', line)
            head = tuple(int(v) for v in m.groups()) if m else head
            continue
        m = re.match(r'\s*(NEW)?\s*Function Name: (\S+)(.*)$', line)
        if not m:
            continue
        rows[m.group(2)] = {COLUMNS[k]: int(v) for k, v in re.findall(r'   ([A-Za-z][A-Za-z \[\]/]*?): (\d+)', m.group(3))}
        if m.group(1):
            new.add(m.group(2))
    return rows, new, head


@pytest.mark.parametrize('p', [1, 2])
def test_z_ob_occ_small_p_runs_out_of_registers_alone(usage, p):  # noqa: F811
    k = kernel(usage, 'k_z_ob_occ', p)
    assert k['scratch'] == 0
    assert k['vgpr_spill'] == 0
    assert k['occupancy'] == 3


@pytest.mark.parametrize('p', [3, 4, 5, 6, 7, 8])
def test_z_ob_occ_larger_p_spills_no_more_than_the_ll_family(usage, p):  # noqa: F811
    k, twin = kernel(usage, 'k_z_ob_occ', p), kernel(usage, 'k_z_ob_ll', p)
    assert k['scratch'] <= twin['scratch']
    assert k['vgpr_spill'] <= twin['vgpr_spill']
    assert k['occupancy'] == 3


def test_pb_z_occ_has_no_scratch(usage):  # noqa: F811
    assert kernel(usage, 'k_pb_z_occ')['scratch'] == 0
    assert kernel(usage, 'k_pb_z')['scratch'] == 0


def test_every_kernel_of_the_parent_build_keeps_its_resources(usage):  # noqa: F811
    rows, new, head = read_listing()
    assert head is not None and head[2] == 0 and head[1] == len(rows) and head[0] == len(rows) - len(new)
    assert len(new) == 10 and all(re.match(r'_ZN3occ10k_(z_ob_occI|pb_z_occE)', name) for name in new), sorted(new)
    assert set(usage) == set(rows), set(usage) ^ set(rows)
    moved = {name: (rows[name], usage[name]) for name in rows if name not in new and rows[name] != usage[name]}
    assert not moved, moved
    assert all(set(r) == set(COLUMNS.values()) for r in rows.values())
