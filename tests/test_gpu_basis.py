"""``basis='device'`` on the device: every primitive of ``libocc_basis.so`` against numpy on the dense Moran operator, the basis end
to end against ``enable_rsr``'s host basis (Davis-Kahan, see tests/test_basis_cpu.py), through both samplers, and at a size
where the dense operator cannot exist.

Tolerances are rounding-error bounds, u = 2^-53 = 1.1e-16 times the number of terms of the longest sum.  Every test prints its
worst case before it asserts; the measured column is that figure on an MI355X over all shapes below.

  primitive  bound asserted                      terms                                              bound's size   measured
  apply      1e-12 ||Omega|| ||v||               two projections of n terms, a sparse row <= 199:   2 n u = 2.7e-13 at n = 1 200    1.9e-15
  project    1e-12 ||v||                         n terms                                            n u = 1.3e-13                   7.1e-16
  filter     1e-12 min(1, ||Omega||^d) ||v||     d applications: d times apply's bound, 1.9e-12 at d = 7, n = 1 200, which is
                                                 ABOVE the constant; the constant is kept           --                              5.1e-16
  gram       1e-13 n ||u|| ||w||                 n terms: n u; the constant is 900 u                1.2e-10 at n = 1 200            1.4e-15
  rotate     1e-13 b ||row|| ||col||             b terms                                            1.1e-11 at b = 112              3.1e-16
  residual   1e-12 (||Omega|| + |lam|) ||v||     an apply, one more term, a sum of n squares        as apply                        7.6e-16

The filter is normalised to 1 at `top`, so its output is never larger than about ||v|| whatever the degree: its error is held
against ||v|| where ||Omega|| > 1 (the weighted graph has ||Omega|| = 0.99, the lattices 1.0, the star 1.0 under rho = 100), and
`top` is placed just above the spectrum so that the output is of ||v||'s size and the bound means something.
"""
import resource

import numpy as np
import pytest
from scipy import sparse
from scipy.linalg import subspace_angles

from .test_basis_cpu import TOL, best_gap, cheb_filter, dense_omega, gershgorin_rho, graph300_case, lattice_case

pytestmark = pytest.mark.gpu
KEY = 0x1234ABCD5678EF01


def star_case():
    """A star of 200 nodes: slice 0 is 199 wide, the others 1 -- uniform width would waste most of it, so true SELL-64."""
    n = 200
    r = np.zeros(n - 1, dtype=int)
    c = np.arange(1, n)
    W = sparse.coo_matrix((np.ones(2 * (n - 1)), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)).tocsr()
    Q = (sparse.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()
    X = np.column_stack([np.ones(n), np.random.default_rng(5).standard_normal(n)])
    return Q, X


def lattice_30x40():
    from occuspytial_amd.utils import make_lattice_problem
    Q, _, X, *_ = make_lattice_problem(30, 40, visits=2, p=2, q=2, random_state=7)
    return sparse.csr_matrix(Q), np.ascontiguousarray(X)


GRAPHS = {'lattice156': lattice_case, 'lattice1200': lattice_30x40, 'graph300': graph300_case, 'star200': star_case}
# (graph, b): n = 156 is no multiple of 64; b = 40 is padded to 48; 112 columns span two column chunks of 64
SHAPES = [('lattice156', 16), ('lattice156', 40), ('lattice156', 48), ('lattice1200', 112), ('graph300', 32), ('star200', 16)]
_dense = {}


def dense(name):
    """Q, X, the dense operator, its norm and rho: computed once per graph and left unchanged."""
    if name not in _dense:
        Q, X = GRAPHS[name]()
        omega, P, _ = dense_omega(Q, X)
        omega.setflags(write=False)
        _dense[name] = {'Q': Q, 'X': X, 'omega': omega, 'P': P, 'norm': np.abs(np.linalg.eigvalsh(omega)).max(), 'rho': gershgorin_rho(Q)}
    return _dense[name]


def handle(name, b):
    from occuspytial_amd._basis_lib import DeviceBasisOps
    d = dense(name)
    ops = DeviceBasisOps(d['Q'], d['X'], b)
    V = np.random.default_rng(b).standard_normal((d['X'].shape[0], b))
    ops.set_block(V)
    return d, ops, V


def col_err(a, b):
    return np.linalg.norm(a - b, axis=0)


def test_layouts_and_bounds():
    """ELL of width 10 for the weighted graph, true SELL-64 for the star, the scale and Gershgorin's bound as numpy has them."""
    for name, ell, wmax in (('graph300', 10, 10), ('star200', 0, 199), ('lattice156', 8, 8)):
        d, ops, _ = handle(name, 16)
        info = ops.info()
        A = -(d['Q'] - sparse.diags(d['Q'].diagonal()))
        assert (info['ell_w'], info['wmax']) == (ell, wmax), (name, info)
        assert abs(info['s'] - d['X'].shape[0] / A.sum()) <= 1e-14 * info['s']
        assert abs(info['rho'] - d['rho']) <= 1e-14 * d['rho'] and d['norm'] <= info['rho']
        ops.close()


@pytest.mark.parametrize('name, b', SHAPES)
def test_apply_and_project(name, b):
    d, ops, V = handle(name, b)
    ops.apply(0, 1)
    got = ops.get_block(1)
    err = col_err(got, d['omega'] @ V) / (d['norm'] * np.linalg.norm(V, axis=0))
    print('apply', name, b, 'worst relative error', err.max())
    assert err.max() <= 1e-12
    assert np.array_equal(ops.get_block(0), V)            # the source is untouched
    ops.project()
    got = ops.get_block(0)
    err = col_err(got, d['P'] @ V) / np.linalg.norm(V, axis=0)
    print('project', name, b, 'worst relative error', err.max())
    assert err.max() <= 1e-12
    ops.close()


@pytest.mark.parametrize('degree', [1, 2, 7])
@pytest.mark.parametrize('name, b', SHAPES)
def test_filter(name, b, degree):
    d, ops, V = handle(name, b)
    lo, hi, top = -d['rho'], 0.3 * d['norm'], min(d['rho'], 1.2 * d['norm'])   # (the star: rho = 100, ||Omega|| = 1.0)
    ops.filter(degree, lo, hi, top)
    got = ops.get_block(0)
    ref = cheb_filter(d['omega'], V, degree, lo, hi, top)
    err = col_err(got, ref) / (min(1.0, d['norm'] ** degree) * np.linalg.norm(V, axis=0))
    print('filter', name, b, degree, 'worst relative error', err.max())
    assert err.max() <= 1e-12
    ops.close()


@pytest.mark.parametrize('name, b', SHAPES)
def test_gram(name, b):
    d, ops, V = handle(name, b)
    n = V.shape[0]
    norms = np.linalg.norm(V, axis=0)
    for which, ref in ((0, V.T @ V), (1, V.T @ (d['omega'] @ V))):
        G = ops.gram(which)
        scale = np.outer(norms, norms) * (d['norm'] if which else 1.0)
        err = (np.abs(G - ref) / scale).max()
        print('gram', which, name, b, 'worst relative error', err, 'bound', 1e-13 * n)
        assert err <= 1e-13 * n
        assert np.array_equal(G, G.T)
        assert np.array_equal(G, ops.gram(which))         # the same bits on a second call
    ops.close()


@pytest.mark.parametrize('name, b', SHAPES)
def test_rotate(name, b):
    d, ops, V = handle(name, b)
    rng = np.random.default_rng(b + 1)
    for b_out in (b, max(1, b - 7)):                       # square, then fewer columns than the block has
        Y = rng.standard_normal((V.shape[1], b_out))
        ops.rotate(Y)
        got = ops.get_block(0)
        ref = V @ Y
        scale = np.outer(np.linalg.norm(V, axis=1), np.linalg.norm(Y, axis=0))
        err = (np.abs(got - ref) / scale).max()
        print('rotate', name, V.shape[1], b_out, 'worst relative error', err, 'bound', 1e-13 * V.shape[1])
        assert got.shape == ref.shape and err <= 1e-13 * V.shape[1]
        V = got
    # the columns past the block stay zero: a Gram matrix after the shrink is the shrunken block's
    assert np.abs(ops.gram(0) - V.T @ V).max() <= 1e-13 * V.shape[0] * np.abs(V.T @ V).max()
    ops.close()


@pytest.mark.parametrize('name, b', SHAPES)
def test_residual(name, b):
    d, ops, V = handle(name, b)
    lam = np.random.default_rng(b + 2).uniform(-1, 1, size=b) * d['norm']
    got = ops.residual(lam)
    ref = np.linalg.norm(d['omega'] @ V - V * lam, axis=0)
    err = np.abs(got - ref) / ((d['norm'] + np.abs(lam)) * np.linalg.norm(V, axis=0))
    print('residual', name, b, 'worst relative error', err.max())
    assert err.max() <= 1e-12
    assert np.array_equal(got, ops.residual(lam))
    ops.close()


def test_bad_arguments_are_refused():
    d, ops, V = handle('lattice156', 16)
    with pytest.raises(ValueError):
        ops.apply(1, 1)
    with pytest.raises(ValueError):
        ops.filter(0, -1.0, 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.filter(3, 0.5, 0.0, 1.0)
    with pytest.raises(ValueError):
        ops.set_block(np.zeros((156, 17)))
    with pytest.raises(ValueError):
        ops.rotate(np.zeros((16, 17)))
    ops.close()


def test_a_refused_create_leaves_the_library_usable_and_close_is_idempotent():
    """10 x 13 queen lattice, n = 130 (three SELL-64 slices, the last partial; one partial tile of 256 sites), p = 2, b = 5 padded
    to 16 columns.  A device number past the last is the bad-argument path: nothing is launched."""
    from occuspytial_amd import _lib
    from occuspytial_amd._basis_lib import DeviceBasisOps
    from occuspytial_amd.utils import rand_precision_mat
    n, b = 130, 5
    Q = sparse.csr_matrix(rand_precision_mat(10, 13)).astype(float)
    X = np.column_stack([np.ones(n), np.random.default_rng(5).standard_normal(n)])
    with pytest.raises(ValueError, match='no such device'):
        DeviceBasisOps(Q, X, b, device=_lib.load().occ_device_count())
    ops = DeviceBasisOps(Q, X, b, device=0)
    assert (ops.ld, ops.info()['ell_w']) == (16, 8)
    V = np.random.default_rng(11).standard_normal((n, b))
    ops.set_block(V)
    omega, _, _ = dense_omega(Q, X)
    G = ops.gram(1)
    norms = np.linalg.norm(V, axis=0)
    err = (np.abs(G - V.T @ (omega @ V)) / (np.outer(norms, norms) * np.abs(np.linalg.eigvalsh(omega)).max())).max()
    print('gram(1) after a refused create: worst relative error', err, 'bound', 1e-13 * n)
    assert err <= 1e-13 * n                                  # (test_gram's bound)
    ops.close()
    ops.close()                                              # a second close is a no-op
    assert not ops._h


# ------------------------------------------------------------------ end to end, 30 x 40, p = 2
@pytest.fixture(scope='module')
def e2e():
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(30, 40, visits=2, p=2, q=2, random_state=7)
    prob = FlatProblem(Q, W, X, y)
    omega, _, _ = dense_omega(prob.Q, prob.X)
    w = np.linalg.eigvalsh(omega)
    return {'data': (Q, W, X, y), 'prob': prob, 'omega': omega, 'w': w, 'rho': gershgorin_rho(prob.Q)}


def _davis_kahan(e2e, rsr_dev, K_host, m):
    w, rho, prob, omega = e2e['w'], e2e['rho'], e2e['prob'], e2e['omega']
    n = prob.n
    g = w[n - m] - w[n - m - 1]
    assert g >= 10 * TOL * rho                              # a condition on the input, from the host's spectrum
    K = rsr_dev['K']
    assert K.shape == (n, m) and rsr_dev['dim'] == m
    theta = np.einsum('ij,ij->j', K, omega @ K)
    sine = np.sin(subspace_angles(K, K_host)).max()
    print('eigenvalue error', np.abs(theta - w[-m:]).max(), 'bound', (TOL * rho) ** 2 / g + 1e-12, 'sine', sine, 'bound', 2 * TOL * rho / g)
    assert np.abs(theta - w[-m:]).max() <= (TOL * rho) ** 2 / g + 1e-12
    assert sine <= 2 * TOL * rho / g
    # K'(QK) is formed as the host branch forms it, which does not symmetrise: symmetric to the rounding of its two products,
    # (n + 16) terms each, 2^-53 apiece, times ||K_a|| ||Q|| ||K_b|| <= ||Q||_1 -- not bit for bit
    Qr = rsr_dev['Q']
    assert np.abs(Qr - Qr.T).max() <= 2 * (n + 16) * 2.0 ** -53 * abs(prob.Q).sum(axis=0).max()
    assert np.array_equal(Qr, K.T @ (prob.Q @ K))
    s, u = np.linalg.eigh(Qr)
    assert np.array_equal(rsr_dev['E'], u * np.sqrt(np.clip(s, 0.0, None)))
    assert np.abs(K.T @ K - np.eye(m)).max() <= 1e-12
    assert np.abs(prob.X.T @ K).max() <= 1e-10 * np.linalg.norm(prob.X)


def test_fixed_q_spans_what_the_host_basis_spans(e2e):
    prob = e2e['prob']
    m, _ = best_gap(e2e['w'], 80, 120)
    K_host = prob.enable_rsr(q=m)['K'].copy()
    dev = dict(prob.enable_rsr(q=m, basis='device'))
    assert prob.tau_shape == 0.5 + 0.5 * m
    _davis_kahan(e2e, dev, K_host, m)
    # reproducibility: the same bits on a second call
    again = prob.enable_rsr(q=m, basis='device')
    assert np.array_equal(dev['K'], again['K'])


def test_threshold_keeps_the_hosts_count(e2e):
    prob, w = e2e['prob'], e2e['w']
    assert np.abs(w - 0.5).min() >= 1e-6
    host = prob.enable_rsr(r=0.5)
    m, K_host = host['dim'], host['K'].copy()
    assert m == int((w >= 0.5).sum())
    dev = dict(prob.enable_rsr(r=0.5, basis='device'))
    _davis_kahan(e2e, dev, K_host, m)
    pb = prob.enable_probit(r=0.5, basis='device')
    assert np.array_equal(pb['K'], dev['K']) and pb['dim'] == m


# ------------------------------------------------------------------ through the samplers, 12 x 13
def _data_156():
    from occuspytial_amd.utils import make_lattice_problem
    return make_lattice_problem(12, 13, visits=3, p=2, q=2, random_state=3)[:4]


@pytest.mark.parametrize('cls', ['LogitRSRGibbs', 'ProbitRSRGibbs'])
def test_samplers_take_the_keyword(cls):
    import occuspytial_amd
    from occuspytial_amd.basis import moran_basis
    Q, W, X, y = _data_156()
    m = 20
    s = getattr(occuspytial_amd, cls)(Q, W, X, y, random_state=10, q=m, basis='device')
    out = s.sample(60, burnin=10, chains=2, progressbar=False)
    assert out['alpha'].shape == (2, 50, 2) and out['beta'].shape == (2, 50, 2) and out['tau'].shape == (2, 50)
    assert all(np.all(np.isfinite(out[k])) for k in ('alpha', 'beta', 'tau'))
    K = moran_basis(sparse.csr_matrix(Q), X, q=m)
    assert s.fixed.q == m and np.array_equal(s.fixed.K, K)
    assert np.array_equal(s.fixed.Q, K.T @ (s._problem.Q @ K)) and s.fixed.tau_shape == 0.5 + 0.5 * m


def test_the_engine_takes_a_device_built_basis_like_any_other(oracle):
    """K from the device re-seated into a host-built problem, Qr and E recomputed as enable_rsr does; ten iterations in lock
    step with the oracle at the tolerances of test_gpu_parity.test_reduced_rank_lockstep_iterations_match_oracle."""
    from occuspytial_amd._engine import Engine
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.basis import moran_basis
    from .test_gpu_parity import _rel
    Q, W, X, y = _data_156()
    m = 20
    prob = FlatProblem(Q, W, X, y)
    prob.enable_rsr(q=m)
    K = moran_basis(prob.Q, prob.X, q=m)
    Qr = np.ascontiguousarray(K.T @ (prob.Q @ K))
    s, u = np.linalg.eigh(Qr)
    prob.rsr = {'K': K, 'Q': Qr, 'E': np.ascontiguousarray(u * np.sqrt(np.clip(s, 0.0, None))), 'dim': m}
    rng = np.random.default_rng(2)
    start = dict(alpha=rng.standard_normal(2), beta=rng.standard_normal(2), tau=1.5, eta=rng.standard_normal(m))
    eng = Engine(prob, [KEY])
    orc = oracle.OracleSampler(prob, KEY)
    eng.set_start(0, **start)
    orc.set_start(**start)
    for it in range(10):
        eng.step()
        orc.step()
        for name, tol in (('omega_b', 1e-10), ('tau', 1e-11), ('theta', 1e-9), ('eta', 1e-9), ('beta', 1e-9), ('alpha', 1e-9)):
            assert _rel(eng.get(name), orc.get(name)) < tol, (it, name, _rel(eng.get(name), orc.get(name)))
        assert np.array_equal(eng.get('z'), orc.get('z'))
        for name in ('alpha', 'beta', 'tau', 'theta', 'z'):
            eng.set(name, orc.get(name))
    eng.close()


# ------------------------------------------------------------------ a size the host cannot do
def test_a_300_by_300_lattice_needs_no_n_by_n_array():
    """n = 90 000: the dense operator would be 65 GB.  q = 64, p = 2; the peak resident set of this process grows by less than
    1 GB (ru_maxrss is in kilobytes)."""
    from occuspytial_amd.basis import moran_basis
    from occuspytial_amd.utils import rand_precision_mat
    n, q = 300 * 300, 64
    Q = sparse.csr_matrix(rand_precision_mat(300, 300)).astype(float)
    X = np.column_stack([np.ones(n), np.random.default_rng(9).standard_normal(n)])
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    K, info = moran_basis(Q, X, q=q, tol=TOL, return_info=True)
    after = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    print('300 x 300:', {k: v for k, v in info.items() if k not in ('eigenvalues', 'residuals')}, 'rss growth (MB)', (after - before) / 1024)
    assert K.shape == (n, q)
    assert np.linalg.norm(info['residuals']) <= TOL * info['rho']
    assert np.abs(K.T @ K - np.eye(q)).max() <= 1e-12
    assert np.abs(X.T @ K).max() <= 1e-10 * np.linalg.norm(X)
    # the residuals again, from the sparse operator on the host: Omega K = s P A P K
    A = -(Q - sparse.diags(Q.diagonal()))
    XtXi = np.linalg.inv(X.T @ X)
    proj = lambda M: M - X @ (XtXi @ (X.T @ M))  # noqa: E731
    R = n / A.sum() * proj(A @ proj(K)) - K * info['eigenvalues']
    assert np.linalg.norm(R, axis=0).max() <= 2 * TOL * info['rho']
    assert (after - before) * 1024 < 1e9
