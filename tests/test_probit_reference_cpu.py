"""The numpy restatement of ProbitRSRGibbs (tests/_probit_reference.py) against independent answers: the truncated normal
against mpmath, the c form of the theta draw against the Cholesky form, and the device's Gauss-Legendre table against
numpy's."""
import os
import re

import numpy as np
import pytest

from . import _probit_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOCS = [0.0, 1.0, 5.0, 10.0, 38.0, 40.0, 100.0, 1e3, 1e6]
US = [2.0 ** -53, 1e-16, 1e-12, 1e-6, 0.01, 0.3, 0.5, 0.7, 0.99, 1 - 1e-6, 1 - 1e-12, 1 - 1e-16]


def _exact(loc, U, positive):
    """The draw to 50 digits: x with Q(a + x) = Q(a) v (a = -loc, v = 1 - U above; a = loc, v = U below)."""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    a, v = (-mp.mpf(loc), 1 - mp.mpf(U)) if positive else (mp.mpf(loc), mp.mpf(U))
    logQ = lambda t: mp.log(mp.erfc(t / mp.sqrt(2)) / 2)
    target = logQ(a) + mp.log(v)
    x0 = float(pr.tn_pos(loc, U)) if positive else -float(pr.tn_neg(loc, U))
    x = mp.findroot(lambda x: logQ(a + x) - target, mp.mpf(x0))
    return x if positive else -x


@pytest.mark.parametrize('positive', [True, False])
def test_truncated_normal_matches_mpmath(positive):
    for loc0 in LOCS:
        for loc in (loc0, -loc0):
            for U in US:
                got = float((pr.tn_pos if positive else pr.tn_neg)(loc, U))
                assert np.isfinite(got), (loc, U)
                assert (got > 0) if positive else (got < 0), (loc, U, got)
                ex = _exact(loc, U, positive)
                assert abs((got - ex) / ex) < 1e-13, (loc, U, got, float(ex))


def test_truncated_normal_equals_the_reference_formula_where_that_is_accurate():
    rng = np.random.default_rng(3)
    loc = rng.uniform(-5, 5, 4000)
    U = rng.uniform(0.001, 0.999, 4000)
    for positive, fn in ((True, pr.tn_pos), (False, pr.tn_neg)):
        ref = pr.tn_reference_formula(loc, U, positive)
        np.testing.assert_allclose(fn(loc, U), ref, rtol=1e-12, atol=1e-12)


def test_truncated_normal_is_finite_where_the_reference_formula_is_not():
    loc = np.array([-40.0, -100.0, -1e3, -1e6])
    U = np.full(4, 0.5)
    with np.errstate(all='ignore'):
        assert not np.all(np.isfinite(pr.tn_reference_formula(loc, U, True)))
    x = pr.tn_pos(loc, U)
    assert np.all(np.isfinite(x)) and np.all(x > 0)
    np.testing.assert_allclose(x, -np.log(0.5) / -loc, rtol=1e-3)   # the exponential limit E / |loc|


def test_ndtri_as241_against_mpmath():
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 40
    for p in [1e-300, 1e-100, 1e-20, 1e-17, 1e-10, 1e-3, 0.02, 0.2, 0.5 - 1e-9, 0.7, 0.99, 1 - 1e-10]:
        ex = mp.sqrt(2) * mp.erfinv(2 * mp.mpf(p) - 1)
        got = float(pr.ndtri_as241(p))
        assert abs(got - ex) <= 4e-16 * max(abs(ex), 1e-300) + 1e-300, (p, got, float(ex))


def test_device_gauss_legendre_table_is_numpys():
    src = open(os.path.join(ROOT, 'occuspytial_amd', 'csrc', 'occ_probit.hpp')).read()

    def table(name):
        body = re.search(r'__constant__ double %s\[16\] = \{(.*?)\};' % name, src, re.S).group(1)
        return np.array([eval(e) for e in body.replace('\n', ' ').split(',')])
    np.testing.assert_allclose(table('kPbGlT'), pr.GL_T, rtol=0, atol=2e-16)
    np.testing.assert_allclose(table('kPbGlW'), pr.GL_W, rtol=0, atol=2e-16)


def _basis(m=12, n=40, seed=0):
    rng = np.random.default_rng(seed)
    K = np.linalg.qr(rng.standard_normal((n, m)))[0]
    B = rng.standard_normal((n, n))
    Qr = K.T @ (B @ B.T) @ K
    return K, K.T @ K, Qr


@pytest.mark.parametrize('tau', [1e-6, 1e-3, 1.0, 1e3, 1e6])
def test_eigen_basis_inverts_the_eta_precision(tau):
    K, KTK, Qr = _basis()
    G, lam = pr.eigen_basis(KTK, Qr)
    A = KTK + tau * Qr
    Ainv = G @ np.diag(1.0 / (1.0 + tau * lam)) @ G.T
    np.testing.assert_allclose(Ainv @ A, np.eye(A.shape[0]), atol=1e-10)


def test_c_form_equals_cholesky_form_at_zero_noise():
    K, KTK, Qr = _basis(m=9, n=30, seed=2)
    G, lam = pr.eigen_basis(KTK, Qr)
    rng = np.random.default_rng(5)
    s = rng.standard_normal(30)
    for tau in (1e-3, 0.7, 50.0):
        A = KTK + tau * Qr
        theta_chol = pr.precision_draw(A, K.T @ s, np.zeros(9))
        c = (1.0 / (1.0 + tau * lam)) * ((K @ G).T @ s)
        np.testing.assert_allclose(G @ c, theta_chol, rtol=1e-11, atol=1e-12)


# ------------------------------------------------------------------ the reference's own first calls (tests/golden/ref_probit_*.npz)
PROBIT_CASES = ['ref_probit_r05', 'ref_probit_q10']


def _fixture(name):
    from .conftest import load_golden
    return load_golden(name)


@pytest.mark.parametrize('case', PROBIT_CASES)
def test_restatement_reproduces_every_conditional_of_the_reference(case):
    """Each _update_* of the reference's probit.py, its first call from a moderate state, restated with the reference's
    own variates: omega_b and omega_a to 1e-12 where |loc| <= 5 (where the reference's inverse CDF is accurate), theta in
    the Cholesky form with the reference's normals, z exactly."""
    from scipy.special import ndtr
    g = _fixture(case)
    X, K, KTK, Qr = g['X'], g['K'], g['KTK'], g['Qr']
    n = X.shape[0]
    close = dict(rtol=1e-12, atol=1e-12)
    # omega_b (sites with z = 1 truncated to (0, inf), the others to (-inf, 0))
    loc = X @ g['in_beta'] + g['in_spatial'] + g['in_eps']
    z = g['in_z']
    ob = np.where(z == 1, pr.tn_pos(loc, g['ob_u']), pr.tn_neg(loc, g['ob_u']))
    ok = np.abs(loc) <= 5
    assert ok.sum() > 0.9 * n
    np.testing.assert_allclose(ob[ok], g['omega_b'][ok], **close)
    assert np.all(np.where(z == 1, ob > 0, ob < 0))
    # tau, from the current theta
    rate = 0.5 * g['in_theta'] @ Qr @ g['in_theta'] + g['tau_rate']
    np.testing.assert_allclose(g['tau_g'] / rate, g['tau'], **close)
    # eps: N((omega_b - X beta - eta) / 2, 1/2)
    xb = X @ g['in_beta']
    eps = 0.5 * (g['omega_b'] - xb - g['in_spatial']) + pr.SQRT_HALF * g['eps_n']
    np.testing.assert_allclose(eps, g['eps'], **close)
    # theta: N(A^-1 b, A^-1), A = K'K + tau Qr, b = K'(omega_b - X beta - eps); the Cholesky form and the reference's normals
    A = KTK + g['tau'] * Qr
    theta = pr.precision_draw(A, K.T @ (g['omega_b'] - xb - g['eps']), g['theta_n'])
    np.testing.assert_allclose(theta, g['theta'], rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(K @ g['theta'], g['spatial'], **close)
    # ... and the engine's c form gives the same mean
    G, lam = pr.eigen_basis(KTK, Qr)
    mean_c = G @ ((1.0 / (1.0 + g['tau'] * lam)) * ((K @ G).T @ (g['omega_b'] - xb - g['eps'])))
    np.testing.assert_allclose(mean_c, pr.precision_draw(A, K.T @ (g['omega_b'] - xb - g['eps']), np.zeros(len(lam))),
                               rtol=1e-10, atol=1e-12)
    # beta, from the intact precision X'X + b_prec
    M = X.T @ X + g['b_prec']
    np.testing.assert_array_equal(M, g['XTX_plus_bprec'])
    bb = g['b_prec'] @ g['b_mu'] + X.T @ (g['omega_b'] - g['spatial'] - g['eps'])
    np.testing.assert_allclose(pr.precision_draw(M, bb, g['beta_n']), g['beta'], **close)
    # omega_a on the rows of the existing sites (reference order), y = 1 rows truncated to (0, inf)
    la = g['oa_W'] @ g['in_alpha']
    oa = np.where(g['oa_y'] == 1, pr.tn_pos(la, g['oa_u']), pr.tn_neg(la, g['oa_u']))
    ok = np.abs(la) <= 5
    np.testing.assert_allclose(oa[ok], g['omega_a'][ok], **close)
    # alpha
    Wa = g['oa_W']
    alpha = pr.precision_draw(Wa.T @ Wa + g['a_prec'], g['a_prec'] @ g['a_mu'] + Wa.T @ g['omega_a'], g['alpha_n'])
    np.testing.assert_allclose(alpha, g['alpha'], **close)
    # z: p = Phi(loc) prod(1 - Phi(w alpha)) / (1 - Phi(loc) + that product) on the surveyed sites without a detection,
    # Phi(loc) on the unsurveyed ones
    loc = X @ g['beta'] + g['spatial'] + g['eps']
    znew = g['in_z'].copy()
    cur, starts = 0, {}
    Wf = g['W_flat']
    for site, v in zip(g['sites'], g['visits']):
        starts[int(site)] = (cur, cur + v)
        cur += v
    for u, i in zip(g['z_u_no'], g['z_no']):
        a, b = starts[int(i)]
        num = ndtr(loc[i]) * np.prod(ndtr(-(Wf[a:b] @ g['alpha'])))
        znew[i] = float(u < num / (ndtr(-loc[i]) + num))
    for u, i in zip(g['z_u_ns'], g['z_ns']):
        znew[i] = float(u < ndtr(loc[i]))
    np.testing.assert_array_equal(znew, g['z'])


@pytest.mark.parametrize('case', PROBIT_CASES)
def test_restatement_step_reproduces_the_reference_iteration(case):
    """The whole restated iteration (tests/_probit_reference.step, Cholesky form) against the reference's first calls:
    the variates are mapped onto the restatement's per-site / per-row layout."""
    from .test_api_cpu import _inputs
    g = _fixture(case)
    Q, W, X, y, _ = _inputs(g)
    n, p = X.shape
    site_ptr = np.concatenate([[0], np.cumsum(g['visits'])])
    yf = g['y_flat']
    obs = np.array([yf[site_ptr[t]:site_ptr[t + 1]].any() for t in range(len(g['sites']))])
    G, lam = pr.eigen_basis(g['KTK'], g['Qr'])
    prob = dict(X=X, W=g['W_flat'], y=yf.astype(float), site_ptr=site_ptr, site_id=g['sites'], obs_site=obs,
                a_mu=g['a_mu'], a_prec=g['a_prec'], b_mu=g['b_mu'], b_prec=g['b_prec'], tau_rate=g['tau_rate'],
                tau_shape=g['tau_shape'], K=g['K'], KTK=g['KTK'], Qr=g['Qr'], Phi=g['K'] @ G, G=G, lam=lam)
    # omega_a's uniforms by flat visit row: the reference's rows are those of the existing sites, in its order
    u_oa = np.full(len(yf), 0.5)
    order = [int(np.flatnonzero(g['sites'] == s)[0]) for s in g['oa_exists']]
    rows = np.concatenate([np.arange(site_ptr[t], site_ptr[t + 1]) for t in order])
    u_oa[rows] = g['oa_u']
    u_z = np.full(n, 0.5)
    u_z[g['z_no']] = g['z_u_no']
    u_z[g['z_ns']] = g['z_u_ns']
    var = dict(u_ob=g['ob_u'], n_eps=g['eps_n'], gamma=g['tau_g'], xi=g['theta_n'], n_beta=g['beta_n'], u_oa=u_oa,
               n_alpha=g['alpha_n'], u_z=u_z)
    st = dict(alpha=g['in_alpha'], beta=g['in_beta'], tau=g['in_tau'], c=np.linalg.solve(G, g['in_theta']),
              eta=g['in_spatial'], eps=g['in_eps'], z=g['in_z'])
    out = pr.step(prob, st, var, theta_form='chol')
    loc_ok = np.abs(X @ g['in_beta'] + g['in_spatial'] + g['in_eps']) <= 5
    np.testing.assert_allclose(out['omega_b'][loc_ok], g['omega_b'][loc_ok], rtol=1e-12, atol=1e-12)
    # (the moderate state keeps every location where the reference's inverse CDF is accurate: all of it is compared)
    assert loc_ok.all() and (np.abs(g['oa_W'] @ g['in_alpha']) <= 5).all()
    for name, tol in (('tau', 1e-12), ('eps', 1e-12), ('theta', 1e-11), ('beta', 1e-11), ('alpha', 1e-11)):
        np.testing.assert_allclose(out[name], g[name], rtol=tol, atol=1e-12, err_msg=name)
    np.testing.assert_allclose(out['omega_a'][rows], g['omega_a'], rtol=1e-12, atol=1e-12)
    np.testing.assert_array_equal(out['z'], g['z'])
