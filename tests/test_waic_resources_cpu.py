"""Registers, scratch and occupancy of k_z_ob_ll, the z update that keeps the log-likelihood sums of streaming WAIC, as the
compiler reports them for gfx950 (no GPU needed; the helpers and the session's one compilation are those of
test_kernel_resources_cpu.py).  Conditions on the generated code, not measurements of speed:

  k_z_ob_ll<P>, P = 1, 2   what k_z_ob<P> and k_z_ob_stats<P> are held to: no scratch, no spilled vector register, three waves
                           per SIMD
  k_z_ob_ll<3 .. 8>        no more scratch than k_z_ob_stats<P> of the same build (the family may spill what its twin spills)
"""
import pytest

from .test_kernel_resources_cpu import kernel, usage  # noqa: F401  (the session-scoped compilation)


@pytest.mark.parametrize('p', [1, 2])
def test_z_ob_ll_small_p_runs_out_of_registers_alone(usage, p):  # noqa: F811
    k = kernel(usage, 'k_z_ob_ll', p)
    assert k['scratch'] == 0
    assert k['vgpr_spill'] == 0
    assert k['occupancy'] == 3


@pytest.mark.parametrize('p', [3, 4, 5, 6, 7, 8])
def test_z_ob_ll_larger_p_spills_what_its_twin_spills(usage, p):  # noqa: F811
    k, twin = kernel(usage, 'k_z_ob_ll', p), kernel(usage, 'k_z_ob_stats', p)
    assert k['scratch'] <= twin['scratch']
    assert k['vgpr_spill'] <= twin['vgpr_spill']
    assert k['occupancy'] == 3
