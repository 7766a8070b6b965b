"""``libocc_sim.so`` on the device: the right-hand sides against the oracle's edge-form prior term, the solve against the dense
pseudo-inverse, the centring, the independence of a draw from its batch, the law of the draws, a loud failure, the Python
layer end to end, and a size at which no dense operator can exist.

Every bound is derived, none is measured (each test prints its worst case before it asserts):
  right-hand side   2e-13 sum_j sqrt(w_ij): 1e-13 per normal, which tests/test_gpu_rng.py holds block_normal to, doubled for the
                    rounding of the row sum; a component's sum of u is an exact cancellation, so only rounding is left:
                    1e-12 sum |terms|
  solve             x - Q^+ u = Q^+ (Q x - u) on the range of Q, so ||x - Q^+ u|| <= ||u - Q x|| / lambda_min+ <= 2 tol ||u|| /
                    lambda_min+ with the residual's own bound of 2 tol (tol reported, twice that recomputed in numpy)
  centring          n 2^-52 max|x|: one rounding of 2^-53 |x_i| per site from the second centring pass, doubled
  law               S draws: an entry of the sample covariance has standard error sqrt((P_ii P_jj + P_ij^2) / S) (Wishart), x'Qx
                    is chi-square with n - k degrees of freedom, so its mean has standard error sqrt(2 (n - k) / S)
"""
import resource

import numpy as np
import pytest
from scipy import sparse

from . import _components_graphs as cg
from .test_basis_cpu import graph300_case
from .test_sim_plan_cpu import REFUSALS, star

pytestmark = pytest.mark.gpu
KEY = 0x1234ABCD5678EF01
TOL = 1e-10
STREAM_ETA_EDGE = 4

GRAPHS = {
    'small': lambda: sparse.csr_matrix(cg.small()['Q']),
    'large': lambda: sparse.csr_matrix(cg.large()['Q']),
    'graph300': lambda: graph300_case()[0],
    'star200': star,
}
_cache = {}


def case(name):
    """Q, its components, the dense pseudo-inverse and lambda_min+: computed once per graph and left unchanged."""
    if name not in _cache:
        from occuspytial_amd.graph import components
        Q = sparse.csr_matrix(GRAPHS[name]()).astype(np.float64)
        Q.sort_indices()
        k, labels = components(Q)
        dense = Q.toarray()
        w = np.linalg.eigvalsh(dense)
        P = np.linalg.pinv(dense, hermitian=True)
        P.setflags(write=False)
        off = -(Q - sparse.diags(Q.diagonal()))
        roots = np.asarray(off.sqrt().sum(axis=1)).ravel()
        _cache[name] = dict(Q=Q, n=Q.shape[0], k=k, labels=labels, P=P, lam_min=w[k], lam=w, roots=roots, size=np.bincount(labels), edges={})
        assert w[k - 1] < 1e-9 * w[-1] < w[k]                  # k zero eigenvalues, one per component
    return _cache[name]


def handle(name, b_max):
    from occuspytial_amd._sim_lib import DeviceFieldOps
    d = case(name)
    return d, DeviceFieldOps(d['Q'], d['labels'], b_max)


def abs_terms(oracle, d, it):
    """sum_i sum_j sqrt(w_ij) |e_ij| over each component (both endpoints of an edge count it), for draw number `it`."""
    if it not in d['edges']:
        C = sparse.triu(d['Q'], k=1).tocoo()
        L = oracle.lib()
        e = np.array([L.orc_block_normal(KEY, int(i), int(j), it, STREAM_ETA_EDGE) for i, j in zip(C.row, C.col)])
        t = np.sqrt(-C.data) * np.abs(e)
        d['edges'][it] = 2.0 * np.bincount(d['labels'][C.row], weights=t, minlength=d['k'])
    return d['edges'][it]


def comp_sums(d, M):
    """(k, b): every component's sum of every column"""
    ind = sparse.csr_matrix((np.ones(d['n']), (d['labels'], np.arange(d['n']))), shape=(d['k'], d['n']))
    return ind @ M


# ------------------------------------------------------------------ 1. right-hand side
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_right_hand_side_is_the_oracles_edge_term(oracle, name):
    d, ops = handle(name, 64)
    worst, worst_sum = 0.0, 0.0
    for b in (1, 16, 17, 64):
        for first in (0, 5):
            ops.draw(KEY, first, b)
            U = ops.get(1)
            assert U.shape == (d['n'], b)
            ref = np.column_stack([oracle.edge_prior_term(d['Q'], KEY, first + c) for c in range(b)])
            alone = d['roots'] == 0
            assert np.all(U[alone] == 0.0) and np.all(ref[alone] == 0.0)           # (a site without neighbours: exactly 0)
            worst = max(worst, (np.abs(U - ref)[~alone] / d['roots'][~alone, None]).max())
            sums = np.abs(comp_sums(d, U))
            terms = np.column_stack([abs_terms(oracle, d, first + c) for c in range(b)])
            worst_sum = max(worst_sum, (sums / np.maximum(terms, 1e-300))[terms > 0].max())
            assert np.all(sums[terms == 0] == 0.0)
    print('right-hand side', name, 'worst |u - oracle| / sum sqrt(w)', worst, 'bound 2e-13; worst component sum / sum|terms|', worst_sum, 'bound 1e-12')
    assert worst <= 2e-13
    assert worst_sum <= 1e-12
    with pytest.raises(ValueError, match=r'first \+ b must not exceed 2\^32'):
        ops.draw(KEY, 2 ** 32 - 4, 5)
    assert REFUSALS['first'] == 'first + b must not exceed 2^32'
    ops.draw(KEY, 2 ** 32 - 4, 4)                              # the last four draw numbers there are
    ops.close()


# ------------------------------------------------------------------ 2. solve, 3. centring
@pytest.fixture(scope='module', params=sorted(GRAPHS))
def solved(request):
    d, ops = handle(request.param, 17)
    ops.draw(KEY, 0, 17)
    info = ops.solve(tol=TOL)
    out = dict(d=d, name=request.param, U=ops.get(1), X=ops.get(0), info=info)
    ops.close()
    return out


def test_solve_is_the_pseudo_inverse(solved):
    d, U, X, info = solved['d'], solved['U'], solved['X'], solved['info']
    un = np.linalg.norm(U, axis=0)
    err = np.linalg.norm(X - d['P'] @ U, axis=0) / (un / d['lam_min'])
    res = np.linalg.norm(U - d['Q'] @ X, axis=0) / un
    print('solve', solved['name'], 'worst ||x - pinv u|| lam_min / ||u||', err.max(), 'bound', 2 * TOL, 'reported residual', info['residual'].max(),
          'recomputed', res.max(), 'iterations', info['iterations'].min(), '-', info['iterations'].max(), 'n', d['n'])
    assert err.max() <= 2 * TOL
    assert info['residual'].max() <= TOL
    assert res.max() <= 2 * TOL
    assert info['iterations'].max() <= d['n'] and info['iterations'].min() >= 1


def test_centred_on_every_component(solved):
    d, X = solved['d'], solved['X']
    sums = np.abs(comp_sums(d, X))
    bound = d['n'] * 2.0 ** -52 * np.abs(X).max()
    print('centring', solved['name'], 'worst component sum', sums.max(), 'bound', bound)
    assert sums.max() <= bound
    single = d['size'][d['labels']] == 1
    assert np.all(X[single] == 0.0) and not np.any(np.signbit(X[single]))


# ------------------------------------------------------------------ 4. a draw is its own
@pytest.mark.parametrize('name', ['large', 'star200'])
def test_a_draw_does_not_depend_on_its_batch(name):
    d, one = handle(name, 1)
    one.draw(KEY, 7, 1)
    i1 = one.solve(tol=TOL)
    alone = one.get(0)[:, 0].copy()
    d, ops = handle(name, 64)
    ops.draw(KEY, 0, 64)
    i64 = ops.solve(tol=TOL)
    batch = ops.get(0)
    ops.draw(KEY, 5, 3)
    i3 = ops.solve(tol=TOL, check_every=1)
    three = ops.get(0)
    print('a draw is its own', name, 'iterations', i1['iterations'][0], i64['iterations'][7], i3['iterations'][2])
    assert np.array_equal(alone, batch[:, 7]) and np.array_equal(alone, three[:, 2])
    assert i1['iterations'][0] == i64['iterations'][7] == i3['iterations'][2]
    assert i1['residual'][0] == i64['residual'][7] == i3['residual'][2]
    assert np.array_equal(batch[:, 5:8], three)
    ops.draw(KEY, 0, 64)                                       # a repeated call returns the same bits
    ops.solve(tol=TOL)
    assert np.array_equal(ops.get(0), batch)
    one.close()
    ops.close()


# ------------------------------------------------------------------ 5. law
def test_the_draws_have_the_law_of_the_field():
    d, ops = handle('small', 64)
    S, key = 4096, 77
    draws = []
    for first in range(0, S, 64):
        ops.draw(key, first, 64)
        ops.solve(tol=TOL)
        draws.append(ops.get(0))
    ops.close()
    x = np.concatenate(draws, axis=1)                          # n x S
    many = d['size'][d['labels']] > 1
    assert many.sum() == 32
    P = d['P'][np.ix_(many, many)]
    C = (x[many] @ x[many].T) / S
    se = np.sqrt((np.outer(np.diag(P), np.diag(P)) + P ** 2) / S)
    zc = np.abs(C - P) / se
    quad = np.einsum('is,is->s', x, d['Q'] @ x)
    zq = abs(quad.mean() - 29.0) / np.sqrt(2.0 * 29.0 / S)
    print('law: worst covariance entry in standard errors', zc.max(), 'bound 5; mean x\'Qx', quad.mean(), 'in standard errors', zq, 'bound 4')
    assert d['n'] - d['k'] == 29
    assert zc.max() <= 5.0
    assert zq <= 4.0


# ------------------------------------------------------------------ 6. failure is loud
def test_a_column_that_is_not_done_is_an_error_and_the_handle_lives():
    d, ops = handle('large', 16)
    ops.draw(KEY, 0, 16)
    with pytest.raises(ValueError, match=r'column \d+ is not done after 3 iterations: relative residual \d\.\d{3}e[-+]\d\d') as e:
        ops.solve(tol=TOL, max_iter=3)
    print('failure:', e.value)
    info = ops.solve(tol=TOL)
    X, U = ops.get(0), ops.get(1)
    res = np.linalg.norm(U - d['Q'] @ X, axis=0) / np.linalg.norm(U, axis=0)
    assert info['residual'].max() <= TOL and res.max() <= 2 * TOL
    for bad, text in ((dict(tol=0.0), REFUSALS['tol']), (dict(max_iter=0), REFUSALS['max_iter']), (dict(check_every=0), REFUSALS['check_every'])):
        with pytest.raises(ValueError) as e:
            ops.solve(**bad)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        ops.draw(KEY, 0, 17)
    assert str(e.value) == REFUSALS['b']
    ops.close()
    from occuspytial_amd._sim_lib import DeviceFieldOps
    for kw, text in ((dict(b_max=65), REFUSALS['b_max']), (dict(labels=np.arange(d['n'], dtype=np.int32)), REFUSALS['labels'])):
        with pytest.raises(ValueError) as e:
            DeviceFieldOps(d['Q'], kw.get('labels', d['labels']), kw.get('b_max', 16))
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        DeviceFieldOps(d['Q'] + sparse.identity(d['n']), d['labels'], 16)
    assert str(e.value) == REFUSALS['singular']


def test_a_refused_create_leaves_the_library_usable_and_close_is_idempotent():
    """10 x 13 queen lattice, n = 130 (three SELL-64 slices, the last partial; one partial tile of 256 sites), cut into rows 0-4,
    rows 5-9 without the last site, and the last site alone; b = 5 padded to 16 columns.  A device number past the last is the
    bad-argument path: nothing is launched.  The bounds are those of tests 2 and 3 above."""
    from occuspytial_amd import _lib
    from occuspytial_amd._sim_lib import DeviceFieldOps
    from occuspytial_amd.graph import components
    from occuspytial_amd.utils import lattice_adjacency
    n, b = 130, 5
    part = (np.arange(n) >= 65).astype(int)
    part[n - 1] = 2
    W = lattice_adjacency(10, 13, 'queen').tocoo()
    keep = part[W.row] == part[W.col]
    W = sparse.csr_matrix((W.data[keep].astype(float), (W.row[keep], W.col[keep])), shape=(n, n))
    Q = (sparse.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()
    k, labels = components(Q)
    assert k == 3 and np.bincount(labels).tolist() == [65, 64, 1]
    with pytest.raises(ValueError, match='no such device'):
        DeviceFieldOps(Q, labels, b, device=_lib.load().occ_device_count())
    ops = DeviceFieldOps(Q, labels, b, device=0)
    assert (ops.info()['ld'], ops.info()['components']) == (16, 3)
    ops.draw(KEY, 0, b)
    info = ops.solve(tol=TOL)
    X, U = ops.get(0), ops.get(1)
    res = np.linalg.norm(U - Q @ X, axis=0) / np.linalg.norm(U, axis=0)
    sums = np.abs(sparse.csr_matrix((np.ones(n), (labels, np.arange(n))), shape=(k, n)) @ X)
    bound = n * 2.0 ** -52 * np.abs(X).max()
    print('after a refused create: reported residual', info['residual'].max(), 'recomputed', res.max(), 'bound', 2 * TOL, 'worst component sum',
          sums.max(), 'bound', bound)
    assert info['residual'].max() <= TOL and res.max() <= 2 * TOL
    assert sums.max() <= bound and np.all(X[n - 1] == 0.0) and np.all(U[n - 1] == 0.0)
    ops.close()
    ops.close()                                                # a second close is a no-op
    assert not ops._h


# ------------------------------------------------------------------ 7. Python, end to end
def test_icar_field_tau_and_batch():
    from occuspytial_amd.simulate import icar_field
    Q = case('large')['Q']
    one = icar_field(Q, size=2, random_state=1)
    two, info = icar_field(Q, tau=[0.5, 2.0], size=2, random_state=1, return_info=True)
    assert one.shape == (2, 360) and np.array_equal(two, one / np.sqrt(np.array([0.5, 2.0]))[:, None])
    assert info['residual'].max() <= TOL and info['iterations'].max() <= 360
    a = icar_field(Q, size=20, random_state=4, batch=1)
    b = icar_field(Q, size=20, random_state=4, batch=16)
    assert np.array_equal(a, b) and not np.array_equal(a[:2], one)


def test_make_spatial_data_feeds_the_sampler():
    from occuspytial_amd import LogitICARGibbs
    from occuspytial_amd.simulate import make_spatial_data
    from occuspytial_amd.utils import rand_precision_mat
    Q0 = sparse.csr_matrix(rand_precision_mat(12, 12)).astype(float)
    Q, W, X, y, alpha, beta, tau, z, eta = make_spatial_data(Q0, visits=3, random_state=2)
    print('eta: sum', eta.sum(), 'max', np.abs(eta).max())
    assert eta.shape == (144,) and abs(eta.sum()) <= 144 * 2.0 ** -52 * np.abs(eta).max() and np.abs(eta).max() > 0
    out = LogitICARGibbs(Q, W, X, y, random_state=3).sample(60, burnin=10, chains=2, progressbar=False)
    assert out['alpha'].shape == (2, 50, 2) and out['beta'].shape == (2, 50, 2) and out['tau'].shape == (2, 50)
    assert all(np.all(np.isfinite(out[k])) for k in ('alpha', 'beta', 'tau'))


def test_scale_on_the_device_lands_on_the_exact_factors():
    from occuspytial_amd import graph
    from .test_simulate_cpu import _bound
    d = case('small')
    Qs, factors = graph.scale(d['Q'], draws=1024, random_state=8)
    exact = np.ones(d['k'])
    for m in np.flatnonzero(d['size'] > 1):
        exact[m] = np.exp(np.log(np.diag(d['P'])[d['labels'] == m]).mean())
    dev = np.abs(np.log(factors / exact))
    print('scale: factors', factors, 'exact', exact, 'worst |log ratio|', dev.max(), 'bound', _bound(1024))
    assert dev.max() <= _bound(1024)
    assert np.all(factors[d['size'] == 1] == 1.0)
    assert np.abs(np.asarray(Qs.sum(axis=1))).max() <= 1e-12 * abs(Qs).max()


# ------------------------------------------------------------------ 8. a size with no dense operator
def test_a_300_by_300_lattice_needs_no_n_by_n_array():
    """n = 90 000: an n x n float64 array would be 65 GB.  The peak resident set of this process grows by less than 2 GB
    (ru_maxrss is in kilobytes)."""
    from occuspytial_amd._sim_lib import DeviceFieldOps
    from occuspytial_amd.utils import rand_precision_mat
    n = 300 * 300
    Q = sparse.csr_matrix(rand_precision_mat(300, 300)).astype(float)
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    ops = DeviceFieldOps(Q, np.zeros(n, dtype=np.int32), 16)
    ops.draw(KEY, 0, 16)
    info = ops.solve(tol=TOL)                                  # the default max_iter, 4 n + 100: every column is done or this raises
    X, U = ops.get(0), ops.get(1)
    ops.close()
    after = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    res = np.linalg.norm(U - Q @ X, axis=0) / np.linalg.norm(U, axis=0)
    quad = np.einsum('ic,ic->c', X, Q @ X)
    z = abs(quad.mean() - (n - 1)) / np.sqrt(2.0 * (n - 1) / 16)
    print('300 x 300: iterations', info['iterations'].min(), '-', info['iterations'].max(), 'reported residual', info['residual'].max(), 'recomputed',
          res.max(), "mean x'Qx", quad.mean(), 'in standard errors', z, 'rss growth (MB)', (after - before) / 1024)
    assert info['iterations'].max() <= 4 * n + 100
    assert res.max() <= 2 * TOL
    assert z <= 5.0
    assert (after - before) * 1024 < 2e9
