"""Registers, scratch and occupancy of k_holdout_sites, the kernel of the held-out predictive scoring, as the compiler reports
them for gfx950 (no GPU needed).  It lives in a translation unit of its own, occ_holdout.hip, so only its device code is compiled
here, once per module, with the helpers and the Makefile's flags of test_kernel_resources_cpu.py plus
-Rpass-analysis=kernel-resource-usage.  Conditions on the generated code, not measurements of speed:

  k_holdout_sites            no scratch, no spilled vector or scalar register, no LDS; every figure equals its line of the
                             committed listing profiles/holdout_resource_usage.txt
  the unit                   defines this kernel and no other
  occ_gibbs.hip's unit       does not define it: its listings (the other resource tests) keep their symbols
"""
import os
import subprocess

import pytest

from . import test_ppc_resources_cpu
from .test_kernel_resources_cpu import CSRC, ROOT, find_hipcc, kernel, makefile_flags, parse_remarks, usage  # noqa: F401
from .test_ppc_resources_cpu import COLUMNS

LISTING = os.path.join(ROOT, 'profiles', 'holdout_resource_usage.txt')
KERNEL = 'k_holdout_sites'


@pytest.fixture(scope='module')
def holdout_usage(tmp_path_factory):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip('hipcc not found')
    out = os.path.join(str(tmp_path_factory.mktemp('holdout_resources')), 'occ_holdout_device.o')
    cmd = [hipcc] + makefile_flags() + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', '-o', out, 'occ_holdout.hip']
    r = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    res = parse_remarks(r.stdout)
    assert res, 'the compiler printed no kernel-resource-usage remarks'
    return res


def read_listing(monkeypatch):
    monkeypatch.setattr(test_ppc_resources_cpu, 'LISTING', LISTING)
    return test_ppc_resources_cpu.read_listing()[0]


def test_holdout_kernel_needs_no_scratch_and_spills_nothing(holdout_usage):
    k = kernel(holdout_usage, KERNEL)
    assert k['scratch'] == 0
    assert k['vgpr_spill'] == 0
    assert k['sgpr_spill'] == 0
    assert k['lds'] == 0


def test_holdout_kernel_equals_its_listing(holdout_usage, monkeypatch):
    rows = read_listing(monkeypatch)
    assert len(rows) == 1 and set(rows) == set(holdout_usage)                    # (the unit defines this kernel alone)
    (sym,) = rows
    assert sym.startswith('_ZN3occ%d%sE' % (len(KERNEL), KERNEL))
    got = kernel(holdout_usage, KERNEL)
    want = {k: v for k, v in rows[sym].items() if k in got}                      # (a column the compiler does not print for a kernel is not held)
    assert got == want and set(rows[sym]) == set(COLUMNS.values())
    assert rows[sym]['lds'] == 0                                                 # an entry's column belongs to one thread: nothing is shared


def test_the_engines_own_unit_does_not_define_it(usage):  # noqa: F811
    assert not [s for s in usage if 'k_holdout_' in s]
