"""occuspytial_amd.simulate and graph.scale on the CPU, with a numpy stand-in for the device: fields drawn from the dense
``pinvh(Q)``, a pure function of (key, draw number) as the device's draws are.

The bound on a scaling factor is derived, not measured: ``nu var_i / P_ii`` is chi-square with ``nu`` degrees of freedom, the
variance of its logarithm is ``psi'(nu / 2)``, and the mean of the log-variances over a component's (correlated) sites cannot
have a larger standard deviation than one of them.  So a factor lies within ``exp(+-5 sqrt(psi'(nu / 2)))`` of the exact
``exp(mean_i log P_ii)`` -- five standard deviations.
"""
import numpy as np
import pytest
from scipy import sparse
from scipy.linalg import pinvh
from scipy.special import polygamma

from occuspytial_amd import graph
from occuspytial_amd.simulate import icar_field, make_spatial_data, marginal_variance
from occuspytial_amd.utils import rand_precision_mat

from . import _components_graphs as cg


class DenseOps:
    """The stand-in ``ops``: draw ``s`` of ``key`` is ``F eps`` with ``F F' = pinvh(Q)`` and ``eps`` the standard normals of
    numpy's generator seeded by ``(key, s)`` -- the same bits whichever batch the draw is part of."""

    def __init__(self, Q):
        w, v = np.linalg.eigh(Q.toarray())
        keep = w > 1e-9 * w.max()                               # (pinvh's own cut: the null space carries nothing)
        self.F = v[:, keep] / np.sqrt(w[keep])
        assert np.allclose(self.F @ self.F.T, pinvh(Q.toarray()), atol=1e-10)
        self.n = Q.shape[0]
        self.calls = []

    def draw(self, key, first, b):
        self.calls.append((first, b))
        cols = [self.F @ np.random.default_rng([int(key) & 0xFFFFFFFF, int(key) >> 32, first + c]).standard_normal(self.F.shape[1]) for c in range(b)]
        self.x = np.column_stack(cols)

    def solve(self, tol=1e-10, max_iter=None, check_every=16):
        b = self.x.shape[1]
        return {'iterations': np.full(b, 7), 'residual': np.full(b, 0.5 * tol)}

    def get(self, which=0):
        return self.x


def dense_field(Q, tau=1.0, size=1, random_state=None):
    return icar_field(Q, tau, size, random_state=random_state, ops=DenseOps(sparse.csr_matrix(Q)), batch=min(size, 64))


def lattice(rows=12, cols=12):
    return sparse.csr_matrix(rand_precision_mat(rows, cols)).astype(float)


def test_icar_field_shapes_and_tau():
    Q = lattice(5, 6)
    ops = DenseOps(Q)
    x, info = icar_field(Q, size=5, random_state=3, ops=ops, batch=2, return_info=True)
    assert x.shape == (5, 30) and x.dtype == np.float64 and ops.calls == [(0, 2), (2, 2), (4, 1)]
    assert info['iterations'].shape == (5,) and info['residual'].shape == (5,) and 0 <= info['key'] < 2 ** 64
    assert np.abs(x.sum(axis=1)).max() <= 1e-12 * np.abs(x).max()
    assert icar_field(Q, random_state=3, ops=ops).shape == (1, 30)
    tau = np.array([0.5, 2.0, 1.0, 4.0, 0.25])
    xt = icar_field(Q, tau=tau, size=5, random_state=3, ops=ops)
    assert np.array_equal(xt, x / np.sqrt(tau)[:, None])
    assert np.array_equal(icar_field(Q, tau=4.0, size=5, random_state=3, ops=ops), x / 2.0)
    assert not np.array_equal(icar_field(Q, size=5, random_state=4, ops=ops), x)


@pytest.mark.parametrize('batch', [1, 16, 64])
def test_the_same_bits_whatever_the_batch(batch):
    Q = lattice(5, 6)
    ref = icar_field(Q, size=70, random_state=11, ops=DenseOps(Q), batch=7)
    assert np.array_equal(icar_field(Q, size=70, random_state=11, ops=DenseOps(Q), batch=batch), ref)


def test_icar_field_refuses_before_a_handle_exists(monkeypatch):
    from occuspytial_amd import _sim_lib

    def no_handle(*a, **k):
        raise AssertionError('a handle was asked for')
    monkeypatch.setattr(_sim_lib, 'DeviceFieldOps', no_handle)
    Q = lattice(5, 6)
    with pytest.raises(ValueError, match='must be singular'):
        icar_field(Q + sparse.identity(30))
    with pytest.raises(ValueError, match='non-positive off-diagonal'):
        icar_field(-Q)
    with pytest.raises(ValueError, match='tau must be positive'):
        icar_field(Q, tau=0.0)
    with pytest.raises(ValueError, match='tau must be positive'):
        icar_field(Q, tau=[1.0, -1.0], size=2)
    with pytest.raises(ValueError, match='tau is a scalar or one value per draw'):
        icar_field(Q, tau=[1.0, 1.0], size=3)
    with pytest.raises(ValueError, match='size must be'):
        icar_field(Q, size=0)
    for batch in (0, 65):
        with pytest.raises(ValueError, match=r'batch must lie in \[1, 64\]'):
            icar_field(Q, batch=batch)


def test_icar_field_without_the_library_is_an_error(monkeypatch, tmp_path):
    from occuspytial_amd import _sim_lib
    from occuspytial_amd._lib import EngineUnavailable
    monkeypatch.setattr(_sim_lib, 'LIB_PATH', str(tmp_path / 'libocc_sim.so'))
    monkeypatch.setattr(_sim_lib, '_lib', None)
    with pytest.raises(EngineUnavailable, match='libocc_sim.so is missing.*There is no CPU fallback for icar_field'):
        icar_field(lattice(5, 6))
    assert _sim_lib._lib is None


def test_csr_arrays_are_what_the_libraries_take():
    from occuspytial_amd._native import csr_arrays
    # row 0 holds (0, 2) twice and its columns out of order; as COO, so that nothing is summed or sorted beforehand
    rows, cols = [0, 0, 0, 0, 1, 2, 2], [2, 0, 2, 1, 1, 2, 0]
    vals = [-1.0, 3, -1.0, -1, 1, 2, -2]
    Q = sparse.coo_matrix((np.array(vals, dtype=np.float32), (rows, cols)), shape=(3, 3))
    n, indptr, indices, data = csr_arrays(Q)
    assert n == 3 and indptr.tolist() == [0, 3, 4, 6] and indices.tolist() == [0, 1, 2, 1, 0, 2]
    assert data.tolist() == [3.0, -1.0, -2.0, 1.0, -2.0, 2.0]
    assert (indptr.dtype, indices.dtype, data.dtype) == (np.int32, np.int32, np.float64)
    assert all(a.flags['C_CONTIGUOUS'] and a.ndim == 1 for a in (indptr, indices, data))
    assert Q.nnz == 7                                          # the caller's matrix is left as it was
    same = csr_arrays(Q.toarray(), 3)                          # a dense array, and n given: the same arrays
    assert same[0] == 3 and all(np.array_equal(a, b) for a, b in zip(same[1:], (indptr, indices, data)))
    with pytest.raises(ValueError, match='^Q must be square$'):
        csr_arrays(sparse.csr_matrix(np.ones((3, 4))))
    with pytest.raises(ValueError, match=r'^Q must be n x n with n = X.shape\[0\]$'):
        csr_arrays(Q, 4)
    with pytest.raises(ValueError, match=r'^Q must be n x n with n = X.shape\[0\]$'):
        csr_arrays(sparse.csr_matrix(np.ones((3, 4))), 3)


def test_make_spatial_data_contract():
    from occuspytial_amd._problem import FlatProblem
    Q = lattice()
    n = 144
    surveyed = np.arange(0, n, 2)
    visits = 2 + (np.arange(surveyed.size) % 3)
    out = make_spatial_data(Q, visits=visits, surveyed=surveyed, p=3, q=2, tau=0.7, random_state=5, field=dense_field)
    Qo, W, X, y, alpha, beta, tau, z, eta = out
    assert sparse.issparse(Qo) and Qo.shape == (n, n) and X.shape == (n, 3) and np.all(X[:, 0] == 1)
    assert alpha.shape == (2,) and beta.shape == (3,) and tau == 0.7 and z.shape == (n,) and eta.shape == (n,)
    assert sorted(W) == sorted(y) == surveyed.tolist()
    for s, v in zip(surveyed, visits):
        assert W[s].shape == (v, 2) and y[s].shape == (v,) and np.all(W[s][:, 0] == 1)
        assert z[s] == 1 or not y[s].any()                     # y = 0 wherever z = 0
    assert abs(eta.sum()) <= 1e-12 * np.abs(eta).max() and np.abs(eta).max() > 0
    assert set(np.unique(z)) <= {0, 1}
    prob = FlatProblem(Qo, W, X, y)
    assert prob.n == n
    again = make_spatial_data(Q, visits=visits, surveyed=surveyed, p=3, q=2, tau=0.7, random_state=5, field=dense_field)
    assert np.array_equal(again[8], eta) and np.array_equal(again[7], z)
    # scalar visits, every site, given coefficients
    out = make_spatial_data(Q, visits=3, alpha=[0.1, 0.2], beta=[0.3, -0.4], random_state=6, field=dense_field)
    assert len(out[1]) == n and all(w.shape == (3, 2) for w in out[1].values()) and np.array_equal(out[4], [0.1, 0.2])
    with pytest.raises(ValueError, match='tau must be positive'):
        make_spatial_data(Q, tau=0.0, field=dense_field)


def _bound(nu):
    return 5.0 * np.sqrt(float(polygamma(1, 0.5 * nu)))


@pytest.fixture(scope='module', params=['lattice144', 'small'])
def scaled(request):
    """Q, its labels, the exact factors, and graph.scale's result at draws = 1024: computed once, left unchanged."""
    Q = lattice() if request.param == 'lattice144' else sparse.csr_matrix(cg.small()['Q'])
    k, labels = graph.components(Q)
    P = pinvh(Q.toarray())
    size = np.bincount(labels)
    exact = np.ones(k)
    for m in range(k):
        if size[m] > 1:
            exact[m] = np.exp(np.log(np.diag(P)[labels == m]).mean())
    Qs, factors = graph.scale(Q, draws=1024, random_state=9, field=dense_field)
    return dict(Q=Q, labels=labels, size=size, exact=exact, P=P, Qs=Qs, factors=factors)


def test_marginal_variance_estimates_the_diagonal_of_pinv(scaled):
    var, nu = marginal_variance(scaled['Q'], draws=1024, random_state=9, field=dense_field)
    assert nu == 1024 and var.shape == (scaled['Q'].shape[0],)
    many = scaled['size'][scaled['labels']] > 1
    assert np.all(var[~many] <= 1e-24)                         # (the dense stand-in's rounding; the device writes exact zeros)
    dev = np.abs(np.log(var[many] / np.diag(scaled['P'])[many]) - (float(polygamma(0, 512.0)) - np.log(512.0)))
    print('worst log-variance deviation', dev.max(), 'in standard deviations', dev.max() / np.sqrt(float(polygamma(1, 512.0))))
    assert dev.max() <= _bound(1024)


def test_scale_factors_within_the_derived_bound(scaled):
    dev = np.abs(np.log(scaled['factors'] / scaled['exact']))
    print('factors', scaled['factors'], 'exact', scaled['exact'], 'worst |log ratio|', dev.max(), 'bound', _bound(1024))
    assert dev.max() <= _bound(1024)
    assert np.all(scaled['factors'][scaled['size'] == 1] == 1.0)


def test_scaled_precision_is_still_an_icar_precision(scaled):
    from occuspytial_amd._problem import _verify_spatial_precision
    Q, Qs, labels = scaled['Q'], scaled['Qs'], scaled['labels']
    assert sparse.issparse(Qs) and Qs.shape == Q.shape
    _verify_spatial_precision(sparse.csr_matrix(Qs))
    assert np.abs(np.asarray(Qs.sum(axis=1))).max() <= 1e-12 * abs(Qs).max()
    # every block is its component's factor times the block of Q; singletons are untouched
    assert np.allclose(Qs.toarray(), scaled['factors'][labels][:, None] * Q.toarray(), rtol=1e-15, atol=0)
    single = scaled['size'][labels] == 1
    assert np.array_equal(Qs.toarray()[single], Q.toarray()[single])
    # the geometric mean of the exact marginal variances under Q_scaled is 1 to within the bound
    Ps = np.diag(pinvh(Qs.toarray()))
    for m in np.flatnonzero(scaled['size'] > 1):
        assert abs(np.log(Ps[labels == m]).mean()) <= _bound(1024)


def test_scaling_twice_gives_factors_near_one(scaled):
    _, again = graph.scale(scaled['Qs'], draws=1024, random_state=10, field=dense_field)
    print('second factors', again)
    assert np.abs(np.log(again)).max() <= _bound(1024)
