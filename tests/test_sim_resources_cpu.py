"""Registers and scratch of the field simulator's kernels, as the compiler reports them for gfx950 (no GPU needed: only the
device code of occ_sim.hip is compiled, once per session, with the Makefile's flags plus -Rpass-analysis=kernel-resource-usage,
as tests/test_kernel_resources_cpu.py does for occ_gibbs.hip).  Conditions on the generated code, not measurements of speed:
every kernel runs out of registers alone -- no scratch, no spilled vector register.
"""
import os
import subprocess

import pytest

from .test_kernel_resources_cpu import CSRC, find_hipcc, makefile_flags, parse_remarks

KERNELS = ('k_sim_draw', 'k_sim_start', 'k_sim_scal_start', 'k_sim_spmv', 'k_sim_scal_alpha', 'k_sim_update', 'k_sim_scal_beta', 'k_sim_dir',
           'k_sim_scal_res', 'k_sim_comp_chunk', 'k_sim_comp_mean', 'k_sim_comp_apply')


@pytest.fixture(scope='module')
def usage(tmp_path_factory):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip('hipcc not found')
    out = os.path.join(str(tmp_path_factory.mktemp('sim_resources')), 'occ_sim_device.o')
    cmd = [hipcc] + makefile_flags() + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c', '-o', out, 'occ_sim.hip']
    r = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    res = parse_remarks(r.stdout)
    assert res, 'the compiler printed no kernel-resource-usage remarks'
    return res


def test_every_kernel_is_there(usage):
    for name in KERNELS:
        hits = [k for k in usage if '%d%s' % (len(name), name) in k]
        assert len(hits) == (2 if name == 'k_sim_spmv' else 1), (name, hits)     # (k_sim_spmv<0> and <1>)
    assert len(usage) == len(KERNELS) + 1, sorted(usage)


def test_no_kernel_has_scratch_or_spills(usage):
    for name, k in sorted(usage.items()):
        print(name, k)
        assert k['scratch'] == 0, name
        assert k['vgpr_spill'] == 0, name
        assert k['sgpr_spill'] == 0, name
