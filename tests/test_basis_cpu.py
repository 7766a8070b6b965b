"""``basis='device'`` without a GPU: the driver of ``occuspytial_amd.basis.moran_basis`` run against an ``ops`` object made of
numpy matrix products on the dense Moran operator of ``FlatProblem.enable_rsr``, the refusals, and the names the header, the
binding and the built library agree on.  (``tests/test_gpu_basis.py`` holds every device primitive to numpy.)

The subspace is checked by Davis-Kahan's bound: with ``R = Omega K - K diag(theta)``, ``||R||_2 <= ||R||_F <= tol * rho`` is the
driver's stopping rule, so the Ritz values lie within ``||R||^2 / gap`` of eigenvalues and the largest principal-angle sine
between span(K) and the host's span is at most ``||R|| / gap'`` with ``gap' >= g / 2``, ``g = lambda_m - lambda_(m+1)`` of the
host's spectrum -- hence ``2 tol rho / g``.  ``g >= 10 tol rho`` is asserted first: a condition on the input.
"""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy import sparse
from scipy.linalg import solve_triangular, subspace_angles

from .conftest import ROOT

TOL = 1e-9


def dense_omega(Q, X):
    """The Moran operator exactly as ``FlatProblem.enable_rsr`` forms it, and the scale ``n / sum(A)``."""
    Q = sparse.csr_matrix(Q).astype(float)
    n, p = X.shape
    chol = np.linalg.cholesky(X.T @ X)
    zi = solve_triangular(chol, np.eye(p), lower=True)
    XTX_i = solve_triangular(chol, zi, lower=True, trans=1)
    P = -np.linalg.multi_dot([X, XTX_i, X.T])
    P[np.diag_indices_from(P)] += 1
    A = Q.copy()
    A.data = -A.data
    A.setdiag(0)
    return n * (P.T @ A @ P) / A.sum(), P, A.tocsr()


def gershgorin_rho(Q):
    Q = sparse.csr_matrix(Q).astype(float)
    A = -(Q - sparse.diags(Q.diagonal()))
    return Q.shape[0] / A.sum() * abs(A).sum(axis=1).max()


class NumpyOps:
    """The driver's ``ops`` as dense matrix products."""

    def __init__(self, Q, X):
        self.omega, self.P, _ = dense_omega(Q, X)
        self.rho = gershgorin_rho(Q)
        self.V = None

    def set_block(self, V):
        self.V = np.array(V, dtype=float)

    def get_block(self):
        return self.V.copy()

    def project(self):
        self.V = self.P @ self.V

    def filter(self, degree, lo, hi, top):
        self.V = cheb_filter(self.omega, self.V, degree, lo, hi, top)

    def gram(self, which):
        G = self.V.T @ (self.omega @ self.V if which else self.V)
        return (G + G.T) / 2

    def rotate(self, Y):
        self.V = self.V @ Y

    def residual(self, lam):
        return np.linalg.norm(self.omega @ self.V - self.V * lam, axis=0)


def cheb_filter(omega, V, degree, lo, hi, top):
    """T_d((omega - c) / e) V / T_d((top - c) / e) by the plain recurrence, numerator and denominator side by side."""
    c, e = (lo + hi) / 2, (hi - lo) / 2
    L = (omega - c * np.eye(omega.shape[0])) / e
    x0 = (top - c) / e
    y0, y1, t0, t1 = V, L @ V, 1.0, x0
    for _ in range(degree - 1):
        y0, y1 = y1, 2 * (L @ y1) - y0
        t0, t1 = t1, 2 * x0 * t1 - t0
    return y1 / t1


def lattice_case():
    """12 x 13 queen lattice, p = 2."""
    from occuspytial_amd.utils import make_lattice_problem
    Q, _, X, *_ = make_lattice_problem(12, 13, visits=2, p=2, q=2, random_state=3)
    return sparse.csr_matrix(Q), np.ascontiguousarray(X)


def graph300_case():
    """300 nodes: the 15 x 20 queen lattice of ``rand_precision_mat`` plus two sets of long edges (every node gains two
    neighbours: 10 at most), 40 lattice edges dropped, weights uniform in [0.5, 2]; Q = D - W, p = 3."""
    from occuspytial_amd.utils import rand_precision_mat
    rng = np.random.default_rng(300)
    Q0 = sparse.csr_matrix(rand_precision_mat(15, 20)).astype(float)
    W = sparse.triu(-(Q0 - sparse.diags(Q0.diagonal())), k=1).tocoo()
    edges = list(zip(W.row.tolist(), W.col.tolist()))
    drop = set(rng.choice(len(edges), size=40, replace=False).tolist())
    edges = [e for k, e in enumerate(edges) if k not in drop]
    edges += [(i, i + 150) for i in range(150)] + [(i, i + 75) for i in list(range(75)) + list(range(150, 225))]
    r, c = np.array(edges).T
    w = rng.uniform(0.5, 2.0, size=r.size)
    Wm = sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(300, 300)).tocsr()
    Q = (sparse.diags(np.asarray(Wm.sum(axis=1)).ravel()) - Wm).tocsr()
    X = np.column_stack([np.ones(300), rng.standard_normal((300, 2))])
    return Q, X


CASES = {'lattice': lattice_case, 'graph300': graph300_case}


@pytest.fixture(scope='module', params=sorted(CASES))
def case(request):
    Q, X = CASES[request.param]()
    omega, _, _ = dense_omega(Q, X)
    w, v = np.linalg.eigh(omega)
    return {'Q': Q, 'X': X, 'omega': omega, 'w': w, 'v': v, 'rho': gershgorin_rho(Q), 'ops': lambda: NumpyOps(Q, X)}


def best_gap(w, lo, hi):
    """m in [lo, hi] with the largest gap lambda_m - lambda_(m+1) (descending count: the m largest eigenvalues)."""
    desc = w[::-1]
    gaps = {m: desc[m - 1] - desc[m] for m in range(lo, hi + 1)}
    m = max(gaps, key=gaps.get)
    return m, gaps[m]


def check_basis(K, info, case, m):
    w, v, X, rho = case['w'], case['v'], case['X'], case['rho']
    n = X.shape[0]
    g = w[n - m] - w[n - m - 1]
    assert g >= 10 * TOL * rho                                  # a condition on the input
    assert K.shape == (n, m)
    assert np.abs(info['eigenvalues'] - w[-m:]).max() <= (TOL * rho) ** 2 / g + 1e-12
    assert np.sin(subspace_angles(K, v[:, -m:])).max() <= 2 * TOL * rho / g
    assert np.abs(K.T @ K - np.eye(m)).max() <= 1e-12
    assert np.abs(X.T @ K).max() <= 1e-10 * np.linalg.norm(X)
    assert np.linalg.norm(info['residuals']) <= TOL * rho
    assert np.all(np.diff(info['eigenvalues']) >= -1e-12)       # ascending, as eigh orders them


def test_driver_fixed_q_against_numpy(case):
    from occuspytial_amd.basis import moran_basis
    m, _ = best_gap(case['w'], 20, 40)
    K, info = moran_basis(case['Q'], case['X'], q=m, ops=case['ops'](), tol=TOL, return_info=True)
    check_basis(K, info, case, m)
    assert info['block'] % 16 == 0 and info['block'] >= m + 32


def test_driver_threshold_against_numpy(case):
    """r is moved off the spectrum if an eigenvalue lies within 1e-6 of 0.5 (it does not in either case; asserted)."""
    from occuspytial_amd.basis import moran_basis
    r, w = 0.5, case['w']
    assert np.abs(w - r).min() >= 1e-6
    m = int((w >= r).sum())
    assert m >= 1
    K, info = moran_basis(case['Q'], case['X'], r=r, ops=case['ops'](), tol=TOL, return_info=True)
    assert K.shape[1] == m
    check_basis(K, info, case, m)


def test_threshold_mode_grows_the_block():
    """A threshold low enough that the first block (n / 16 + 32 columns, rounded to 16: 48) cannot hold the answer, which
    needs the wanted columns and one converged value below r."""
    from occuspytial_amd.basis import moran_basis
    Q, X = lattice_case()
    w = np.linalg.eigvalsh(dense_omega(Q, X)[0])
    r = 0.05
    assert np.abs(w - r).min() >= 1e-6
    m = int((w >= r).sum())
    assert m >= 48
    K, info = moran_basis(Q, X, r=r, ops=NumpyOps(Q, X), tol=TOL, return_info=True)
    assert K.shape[1] == m and info['block'] > 48
    assert np.abs(info['eigenvalues'] - w[-m:]).max() <= 1e-11


def test_the_same_inputs_give_the_same_bits():
    from occuspytial_amd.basis import moran_basis
    Q, X = lattice_case()
    a = moran_basis(Q, X, q=20, ops=NumpyOps(Q, X))
    b = moran_basis(Q, X, q=20, ops=NumpyOps(Q, X))
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ refusals
def test_an_unconverged_basis_is_never_returned():
    from occuspytial_amd.basis import moran_basis
    Q, X = lattice_case()
    with pytest.raises(RuntimeError, match=r'did not converge in 1 outer iterations: residual \d\.\d+e[-+]\d+'):
        moran_basis(Q, X, q=20, ops=NumpyOps(Q, X), degree=2, max_outer=1)


def test_the_references_two_value_errors_keep_their_texts():
    from occuspytial_amd.basis import moran_basis
    Q, X = lattice_case()
    with pytest.raises(ValueError, match=r'^Threshold value needs to be in \[0, 1\]$'):
        moran_basis(Q, X, r=1.5, ops=NumpyOps(Q, X))
    # the complete graph with an intercept: P A P = -P, every eigenvalue of the Moran operator is negative or zero
    n = 40
    Qk = sparse.csr_matrix(n * np.eye(n) - np.ones((n, n)))
    Xk = np.ones((n, 1))
    with pytest.raises(ValueError, match='^The Moran Operator Matrix of the data has no positive eigenvalues. Set threshold to a lower value$'):
        moran_basis(Qk, Xk, r=0.5, ops=NumpyOps(Qk, Xk))


def test_more_columns_than_the_samplers_take_are_refused_in_their_text():
    from occuspytial_amd.basis import moran_basis
    with pytest.raises(ValueError, match=r'^5000 basis columns selected; the device path supports at most 4096 '):
        moran_basis(None, np.ones((6000, 1)), q=5000, ops=object())


def test_a_failure_right_after_the_block_grew_reports_no_residual_it_does_not_have():
    """max_outer runs out on the round that grew the block: the residuals of the grown block are not known yet (inf), and the
    message says so instead of the norm of an empty slice."""
    from occuspytial_amd.basis import moran_basis
    Q, X = lattice_case()
    with pytest.raises(RuntimeError, match='residual inf'):
        moran_basis(Q, X, r=0.05, ops=NumpyOps(Q, X), max_outer=1)


def _problem():
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(6, 7, visits=2, p=2, q=2, random_state=1)
    return FlatProblem(Q, W, X, y), (Q, W, X, y)


def test_any_other_basis_is_refused_at_every_call_site():
    from occuspytial_amd import LogitRSRGibbs, ProbitRSRGibbs
    prob, data = _problem()
    for call in (lambda: prob.enable_rsr(q=5, basis='nonsense'), lambda: prob.enable_probit(q=5, basis='nonsense'),
                 lambda: LogitRSRGibbs(*data, q=5, basis='nonsense'), lambda: ProbitRSRGibbs(*data, q=5, basis='nonsense')):
        with pytest.raises(ValueError, match="basis must be 'host' or 'device'"):
            call()


def test_the_default_is_the_host_and_unchanged():
    prob, _ = _problem()
    a = prob.enable_rsr(q=5)
    b = prob.enable_rsr(q=5, basis='host')
    assert all(np.array_equal(a[k], b[k]) for k in ('K', 'Q', 'E')) and a['dim'] == b['dim'] == 5
    omega, _, _ = dense_omega(prob.Q, prob.X)
    assert np.array_equal(a['K'], np.linalg.eigh(omega)[1][:, -5:])


def test_device_basis_without_the_library_is_an_error(monkeypatch, tmp_path):
    from occuspytial_amd import _basis_lib
    from occuspytial_amd._lib import EngineUnavailable
    monkeypatch.setattr(_basis_lib, 'LIB_PATH', str(tmp_path / 'libocc_basis.so'))
    monkeypatch.setattr(_basis_lib, '_lib', None)
    prob, _ = _problem()
    with pytest.raises(EngineUnavailable, match='libocc_basis.so is missing'):
        prob.enable_rsr(q=5, basis='device')
    with pytest.raises(EngineUnavailable):
        prob.enable_probit(q=5, basis='device')
    assert prob.rsr is None


# ------------------------------------------------------------------ names
def _header():
    return open(os.path.join(ROOT, 'include', 'occ_basis.h')).read()


def test_header_and_binding_agree_on_names_and_version():
    from occuspytial_amd import _basis_lib
    text = re.sub(r'/\*.*?\*/', '', _header(), flags=re.S)
    declared = re.findall(r'\b(occ_basis_\w+)\s*\(', text)
    assert sorted(declared) == sorted(name for name, _, _ in _basis_lib.SYMBOLS) and len(set(declared)) == len(declared)
    assert int(re.search(r'#define OCC_BASIS_VERSION (\d+)', text).group(1)) == _basis_lib.VERSION
    assert int(re.search(r'#define OCC_BASIS_MAX_P (\d+)', text).group(1)) == _basis_lib.MAX_P
    # argument counts
    for name, _, argtypes in _basis_lib.SYMBOLS:
        args = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1).strip()
        assert (0 if args == 'void' else args.count(',') + 1) == len(argtypes), name


def test_the_built_library_exports_every_declared_symbol():
    from occuspytial_amd import _basis_lib
    assert _basis_lib.LIB_PATH == os.path.join(ROOT, 'occuspytial_amd', 'libocc_basis.so')
    assert os.path.exists(_basis_lib.LIB_PATH), 'run __graft_entry__.build()'
    lib = ctypes.CDLL(_basis_lib.LIB_PATH)
    for name, _, _ in _basis_lib.SYMBOLS:
        assert hasattr(lib, name), name
    assert _basis_lib.load().occ_basis_version() == _basis_lib.VERSION


def test_the_engines_abi_does_not_know_the_basis_library():
    from occuspytial_amd import _lib
    assert not any('occ_basis' in name for name, _, _ in _lib.SYMBOLS)
    assert 'occ_basis' not in open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    assert 'occ_basis' not in open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'occ_gibbs.hip')).read()
    mk = open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^all:.*\$\(OUT\).*\$\(BASIS_OUT\)', mk, flags=re.M)
