"""Registers, scratch and occupancy of k_sp_resid and k_sp_moran, the two kernels of the spatial residual check, as the compiler
reports them for gfx950 (no GPU needed).  They live in a translation unit of their own, occ_spatial.hip, so only its device
code is compiled here, once per module, with the helpers and the Makefile's flags of test_kernel_resources_cpu.py plus
-Rpass-analysis=kernel-resource-usage.  Conditions on the generated code, not measurements of speed:

  k_sp_resid, k_sp_moran     no scratch, no spilled vector or scalar register; every figure equals its line of the committed
                             listing profiles/spatial_resource_usage.txt
  the unit                   defines these two kernels and no other
  occ_gibbs.hip's unit       does not define them: its listings (the other resource tests) keep their symbols
"""
import os
import subprocess

import pytest

from . import test_ppc_resources_cpu
from .test_kernel_resources_cpu import CSRC, ROOT, find_hipcc, kernel, makefile_flags, parse_remarks, usage  # noqa: F401
from .test_ppc_resources_cpu import COLUMNS

LISTING = os.path.join(ROOT, 'profiles', 'spatial_resource_usage.txt')
KERNELS = ('k_sp_resid', 'k_sp_moran')


@pytest.fixture(scope='module')
def spatial_usage(tmp_path_factory):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip('hipcc not found')
    out = os.path.join(str(tmp_path_factory.mktemp('spatial_resources')), 'occ_spatial_device.o')
    cmd = [hipcc] + makefile_flags() + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', '-o', out, 'occ_spatial.hip']
    r = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    res = parse_remarks(r.stdout)
    assert res, 'the compiler printed no kernel-resource-usage remarks'
    return res


def read_listing(monkeypatch):
    monkeypatch.setattr(test_ppc_resources_cpu, 'LISTING', LISTING)
    return test_ppc_resources_cpu.read_listing()[0]


@pytest.mark.parametrize('name', KERNELS)
def test_spatial_kernels_need_no_scratch_and_spill_nothing(spatial_usage, name):
    k = kernel(spatial_usage, name)
    assert k['scratch'] == 0
    assert k['vgpr_spill'] == 0
    assert k['sgpr_spill'] == 0


def test_spatial_kernels_equal_their_listing(spatial_usage, monkeypatch):
    rows = read_listing(monkeypatch)
    assert len(rows) == 2 and set(rows) == set(spatial_usage)                    # (the unit defines these two kernels alone)
    for name in KERNELS:
        hits = [sym for sym in rows if sym.startswith('_ZN3occ%d%sE' % (len(name), name))]
        assert len(hits) == 1, (name, sorted(rows))
        got = kernel(spatial_usage, name)
        want = {k: v for k, v in rows[hits[0]].items() if k in got}              # (a column the compiler does not print for a kernel is not held)
        assert got == want and set(rows[hits[0]]) == set(COLUMNS.values())
    assert rows[[s for s in rows if 'k_sp_moran' in s][0]]['lds'] == 64          # the eight 64-bit sums of a workgroup


def test_the_engines_own_unit_does_not_define_them(usage):  # noqa: F811
    assert not [sym for sym in usage if 'k_sp_' in sym]
