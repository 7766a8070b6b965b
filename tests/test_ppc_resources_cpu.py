"""Registers, scratch and occupancy of k_z_ob_ppc, the z update that forms the posterior predictive check, as the compiler
reports them for gfx950 (no GPU needed; the helpers and the session's one compilation are those of
test_kernel_resources_cpu.py).  Conditions on the generated code, not measurements of speed:

  k_z_ob_ppc<P>, P = 1, 2        what every family before was held to: no scratch, no spilled vector register, three waves
                                 per SIMD
  k_z_ob_ppc<0>, <3 .. 8>        three waves per SIMD; scratch and spilled vector registers no more than the values the
                                 compiler reported when the family was added, which the committed listing
                                 profiles/ppc_resource_usage.txt holds in its lines marked NEW
  every other kernel             the SGPRs, VGPRs, AGPRs, scratch, spills, LDS and occupancy it had before the family was added:
                                 the listing's lines without NEW are the parent build's values, symbol for symbol, and this
                                 build must reproduce every one
"""
import os
import re

import pytest

from .test_kernel_resources_cpu import ROOT, kernel, usage  # noqa: F401  (the session-scoped compilation)

LISTING = os.path.join(ROOT, 'profiles', 'ppc_resource_usage.txt')
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


def listed(p):
    """The listing's line of k_z_ob_ppc<p>."""
    rows, new, _ = read_listing()
    hits = [name for name in new if name.startswith('_ZN3occ10k_z_ob_ppcILi%dEE' % p)]
    assert len(hits) == 1, hits
    return rows[hits[0]]


@pytest.mark.parametrize('p', [1, 2])
def test_z_ob_ppc_small_p_runs_out_of_registers_alone(usage, p):  # noqa: F811
    k = kernel(usage, 'k_z_ob_ppc', p)
    assert k['scratch'] == 0
    assert k['vgpr_spill'] == 0
    assert k['occupancy'] == 3


@pytest.mark.parametrize('p', [0, 3, 4, 5, 6, 7, 8])
def test_z_ob_ppc_larger_p_spills_no_more_than_when_it_was_added(usage, p):  # noqa: F811
    k, was = kernel(usage, 'k_z_ob_ppc', p), listed(p)
    assert k['scratch'] <= was['scratch']
    assert k['vgpr_spill'] <= was['vgpr_spill']
    assert k['occupancy'] == 3


def test_every_kernel_of_the_parent_build_keeps_its_resources(usage):  # noqa: F811
    rows, new, head = read_listing()
    assert head == (174, 183, 0) and len(rows) == 183
    assert len(new) == 9 and all(name.startswith('_ZN3occ10k_z_ob_ppcILi') for name in new), sorted(new)
    assert set(usage) == set(rows), set(usage) ^ set(rows)
    moved = {name: (rows[name], usage[name]) for name in rows if name not in new and rows[name] != usage[name]}
    assert not moved, moved
    assert all(set(r) == set(COLUMNS.values()) for r in rows.values())
