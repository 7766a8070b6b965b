"""Registers, scratch and occupancy of the kernels on the headline's critical path, as the compiler reports them for gfx950
(no GPU needed: only the device code of occ_gibbs.hip is compiled, once per session, with the Makefile's flags plus
-Rpass-analysis=kernel-resource-usage).  These are conditions on the generated code, not measurements of speed:

  k_z_ob<P>, k_z_ob_stats<P>, P = 1, 2   no scratch, no spilled vector register, three waves per SIMD -- the Polya-Gamma waves
                                         of a kernel that touches scratch at all run ~ 20 % slower (HISTORY.md, round 4)
  k_z_ob<3 .. 8>                         no more scratch than before the head of k_z_ob was shortened
  k_omega_b<2>                           no scratch (the same draw as a kernel of its own: what k_z_ob is held against)
  k_iter<8, 1, 1>                        the headline's solve: at most 171 VGPRs, no scratch, two waves per SIMD (a guard: work on
                                         k_z_ob must not move it)
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')

FIELDS = {
    'VGPRs': 'vgprs', 'ScratchSize [bytes/lane]': 'scratch', 'Occupancy [waves/SIMD]': 'occupancy',
    'SGPRs Spill': 'sgpr_spill', 'VGPRs Spill': 'vgpr_spill', 'TotalSGPRs': 'sgprs', 'SGPRs': 'sgprs', 'AGPRs': 'agprs', 'LDS Size [bytes/block]': 'lds',
}


def find_hipcc():
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.isfile(cand) and os.access(cand, os.X_OK):
            return cand
    return None


def makefile_flags():
    """HIPFLAGS of csrc/Makefile with $(ARCH) resolved: the flags the library is built with."""
    text = open(os.path.join(CSRC, 'Makefile')).read()
    arch = re.search(r'^ARCH \?= (\S+)', text, re.M).group(1)
    flags = re.search(r'^HIPFLAGS \?= (.*)$', text, re.M).group(1)
    return flags.replace('$(ARCH)', arch).split()


def parse_remarks(text):
    """{mangled kernel name: {field: int}} from the compiler's kernel-resource-usage remarks."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r'remark: .*?Function Name: (\S+)', line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r'remark: (?:\S+: )?\s*([A-Za-z][A-Za-z \[\]/]*?): (\d+)\s*(?:\[-R\S*\])?\s*$', line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def compile_remarks(workdir):
    hipcc = find_hipcc()
    cmd = [hipcc] + makefile_flags() + ['--cuda-device-only', '-Rpass-analysis=kernel-resource-usage', '-c',
                                        '-o', os.path.join(str(workdir), 'occ_gibbs_device.o'), 'occ_gibbs.hip']
    r = subprocess.run(cmd, cwd=CSRC, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return parse_remarks(r.stdout)


@pytest.fixture(scope='session')
def usage(tmp_path_factory):
    if find_hipcc() is None:
        pytest.skip('hipcc not found')
    res = compile_remarks(tmp_path_factory.mktemp('kernel_resources'))
    assert res, 'the compiler printed no kernel-resource-usage remarks'
    return res


def kernel(usage, name, *targs):
    """The one kernel occ::<name><targs...>(...) by its mangled name (Itanium: _ZN3occ<len><name>I Li<t>E ... E)."""
    prefix = '_ZN3occ%d%s' % (len(name), name) + ('I' + ''.join('Li%dE' % t for t in targs) + 'E' if targs else '')
    hits = [k for k in usage if k.startswith(prefix) and not k[len(prefix):len(prefix) + 1].isdigit()]
    assert len(hits) == 1, (prefix, hits)
    print(hits[0], usage[hits[0]])
    return usage[hits[0]]


@pytest.mark.parametrize('name', ['k_z_ob', 'k_z_ob_stats'])
@pytest.mark.parametrize('p', [1, 2])
def test_z_ob_small_p_runs_out_of_registers_alone(usage, name, p):
    k = kernel(usage, name, p)
    assert k['scratch'] == 0
    assert k['vgpr_spill'] == 0
    assert k['occupancy'] == 3


@pytest.mark.parametrize('p, most', [(3, 76), (4, 76), (5, 92), (6, 104), (7, 216), (8, 400)])
def test_z_ob_larger_p_scratch_not_above_its_old_size(usage, p, most):
    assert kernel(usage, 'k_z_ob', p)['scratch'] <= most


def test_omega_b_has_no_scratch(usage):
    assert kernel(usage, 'k_omega_b', 2)['scratch'] == 0


def test_headline_solve_is_where_it_was(usage):
    k = kernel(usage, 'k_iter', 8, 1, 1)
    assert k['vgprs'] <= 171
    assert k['scratch'] == 0
    assert k['occupancy'] == 2
