"""The device primitives of the Moran basis (include/occ_basis.h) with MORE THAN 8 columns of X: the projection kernels
(k_basis_xt, k_basis_xt_solve, k_basis_combine) then run their instantiation with 32 register sums.

Cases: p in {9, 12, 32} (the first above the instantiation with 8, one inside, the last column of the wide one) and p = 8 (the
last of the narrow one) on the 12 x 13 lattice -- n = 156 is no multiple of 64 or 256, so the last slice and tile are ragged --
with b = 16 and b = 40 (padded to 48).  The reference is the dense float64 operator of tests/test_basis_cpu.py (dense_omega),
the bounds are those of tests/test_gpu_basis.py for the same primitives: 1e-12 relative per column for apply and project,
the Davis-Kahan bounds of its end-to-end test for the basis itself.  p = 33 is refused.  Without the wide instantiation every
case above 8 fails at the handle's creation ("p must lie in [1, 8]")."""
import signal

import numpy as np
import pytest
from scipy import sparse

from .test_basis_cpu import best_gap, dense_omega, gershgorin_rho
from .test_gpu_basis import _davis_kahan, col_err

pytestmark = pytest.mark.gpu
_cases = {}


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(signum, frame):
        raise TimeoutError('a device-basis covariate test ran longer than 60 s')
    signal.signal(signal.SIGALRM, stop)
    signal.alarm(60)
    yield
    signal.alarm(0)


def case(p):
    """The lattice problem with p occupancy covariates and its dense operator: computed once per p and left unchanged."""
    if p not in _cases:
        from occuspytial_amd._problem import FlatProblem
        from occuspytial_amd.utils import make_lattice_problem
        Q, W, X, y, *_ = make_lattice_problem(12, 13, visits=2, p=p, q=2, random_state=p)
        prob = FlatProblem(Q, W, X, y)
        omega, P, _ = dense_omega(prob.Q, prob.X)
        omega.setflags(write=False)
        w = np.linalg.eigvalsh(omega)
        _cases[p] = {'prob': prob, 'omega': omega, 'P': P, 'w': w, 'norm': np.abs(w).max(), 'rho': gershgorin_rho(prob.Q)}
    return _cases[p]


@pytest.mark.parametrize('b', [16, 40])
@pytest.mark.parametrize('p', [8, 9, 12, 32])
def test_apply_and_project_with_many_columns_of_X(p, b):
    from occuspytial_amd._basis_lib import DeviceBasisOps
    d = case(p)
    prob = d['prob']
    assert prob.X.shape == (156, p)
    ops = DeviceBasisOps(sparse.csr_matrix(prob.Q), np.ascontiguousarray(prob.X), b)
    V = np.random.default_rng(100 * p + b).standard_normal((156, b))
    ops.set_block(V)
    ops.apply(0, 1)
    err = col_err(ops.get_block(1), d['omega'] @ V) / (d['norm'] * np.linalg.norm(V, axis=0))
    print('apply p =', p, 'b =', b, 'worst relative error', err.max())
    assert err.max() <= 1e-12
    assert np.array_equal(ops.get_block(0), V)
    ops.project()
    got = ops.get_block(0)
    err = col_err(got, d['P'] @ V) / np.linalg.norm(V, axis=0)
    print('project p =', p, 'b =', b, 'worst relative error', err.max())
    assert err.max() <= 1e-12
    assert np.abs(prob.X.T @ got).max() <= 1e-10 * np.linalg.norm(prob.X) * np.linalg.norm(V, axis=0).max()
    ops.close()


@pytest.mark.parametrize('p', [9, 32])
def test_the_device_basis_spans_what_the_host_basis_spans(p):
    d = case(p)
    prob = d['prob']
    m, _ = best_gap(d['w'], 20, 40)
    K_host = prob.enable_rsr(q=m)['K'].copy()
    dev = dict(prob.enable_rsr(q=m, basis='device'))
    _davis_kahan(d, dev, K_host, m)
    again = prob.enable_rsr(q=m, basis='device')
    assert np.array_equal(dev['K'], again['K'])


def test_thirty_three_columns_are_refused():
    from occuspytial_amd._basis_lib import DeviceBasisOps
    d = case(9)
    X = np.random.default_rng(0).standard_normal((156, 33))
    with pytest.raises(ValueError, match='1 to 32 occupancy covariates'):
        DeviceBasisOps(sparse.csr_matrix(d['prob'].Q), X, 16)
