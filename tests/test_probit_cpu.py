"""ProbitRSRGibbs on the host: the class, its set-up against the reference's rules, and the refusal of a library that does
not implement the probit model (the CPU oracle's C ABI ignores ``link`` and would run the logit model)."""
import os

import numpy as np
import pytest
from scipy import sparse

from . import _probit_reference as pr
from .conftest import ROOT

ABI_LIB = os.path.join(ROOT, 'oracle', 'liboccoracle_abi.so')


def _data(n=150, seed=10):
    from occuspytial_amd.utils import make_data
    return make_data(n, min_v=2, max_v=4, ns=n // 2, p=3, q=2, random_state=seed)[:4]


def test_the_class_is_exported():
    import occuspytial_amd
    from occuspytial_amd import ProbitRSRGibbs
    from occuspytial_amd.gibbs import ProbitRSRGibbs as P2
    assert ProbitRSRGibbs is P2 and 'ProbitRSRGibbs' in occuspytial_amd.__all__


def test_reference_sampler_rules():
    """reference gibbs/tests/test_samplers.py for this class, on the host-only paths."""
    from occuspytial_amd import ProbitRSRGibbs
    Q, W, X, y = _data()
    with pytest.raises(ValueError, match='Threshold value needs to be in'):
        ProbitRSRGibbs(Q, W, X, y, r=1.1)
    hp = dict(a_mu=np.ones(2), a_prec=np.eye(2) * 2, b_mu=np.ones(3), b_prec=np.eye(3) * 3, tau_rate=2.0, tau_shape=3.0)
    s = ProbitRSRGibbs(Q, W, X, y, hparams=hp, random_state=1)
    for k, v in hp.items():
        assert np.array_equal(s.fixed[k], v)
    Qn = sparse.csr_matrix(Q.toarray() + np.eye(Q.shape[0]))
    with pytest.raises(ValueError, match='must be singular'):
        ProbitRSRGibbs(Qn, W, X, y)


def test_fixed_quantities_and_default_start():
    """The reference's _configure and default start, restated: K from the Moran operator, Qr = K'QK, KTK = K'K,
    tau_shape = 0.5 + 0.5 q, XTX_plus_bprec untouched; the start draws base values, then eta, then eps, bit for bit."""
    from occuspytial_amd import ProbitRSRGibbs
    from occuspytial_amd.utils import get_generator
    Q, W, X, y = _data()
    for kw in ({}, {'q': 10}):
        s = ProbitRSRGibbs(Q, W, X, y, random_state=10, **kw)
        P = np.eye(X.shape[0]) - X @ np.linalg.inv(X.T @ X) @ X.T
        A = -Q.toarray()
        np.fill_diagonal(A, 0)
        w, v = np.linalg.eigh(X.shape[0] * (P.T @ A @ P) / A.sum())
        m = kw.get('q') or int(np.sum(w >= 0.5))
        K = v[:, -m:]
        assert s.fixed.q == m
        np.testing.assert_allclose(np.abs(s.fixed.K), np.abs(K), atol=1e-8)   # (eigenvector signs are arbitrary)
        np.testing.assert_allclose(s.fixed.Q, s.fixed.K.T @ Q.toarray() @ s.fixed.K, atol=1e-10)
        np.testing.assert_allclose(s.fixed.KTK, s.fixed.K.T @ s.fixed.K, atol=1e-12)
        assert s.fixed.tau_shape == 0.5 + 0.5 * m
        np.testing.assert_array_equal(s.fixed.XTX_plus_bprec, X.T @ X + np.eye(3) / 10)
        s._initialize_posterior_state(None)
        rng = get_generator(10)
        tau = rng.gamma(0.5, 1 / 0.005)
        rng.standard_normal(X.shape[0])
        alpha = rng.multivariate_normal(np.zeros(2), 100 * np.eye(2) / 10, method='cholesky')
        beta = rng.multivariate_normal(np.zeros(3), 100 * np.eye(3) / 10, method='cholesky')
        eta = rng.normal(scale=5, size=m)
        eps = rng.standard_normal(X.shape[0])
        assert s.state.tau == tau
        for name, ref in (('alpha', alpha), ('beta', beta), ('eta', eta), ('eps', eps)):
            assert np.array_equal(getattr(s.state, name), ref), name
        assert np.array_equal(s.state.spatial, s.fixed.K @ eta)


@pytest.mark.parametrize('tau', [1e-6, 1e-2, 1.0, 1e2, 1e6])
def test_the_uploaded_eigenvectors_invert_the_eta_precision(tau):
    from occuspytial_amd import ProbitRSRGibbs
    Q, W, X, y = _data()
    s = ProbitRSRGibbs(Q, W, X, y, random_state=0)
    pb = s._problem.probit
    G, lam = pb['G'], pb['lam']
    A = s.fixed.KTK + tau * s.fixed.Q
    np.testing.assert_allclose(G @ np.diag(1 / (1 + tau * lam)) @ G.T @ A, np.eye(s.fixed.q), atol=1e-10)
    np.testing.assert_allclose(pb['Phi'], s.fixed.K @ G, atol=1e-13)
    assert np.all(lam >= 0)


def test_limits_are_value_errors():
    from occuspytial_amd import ProbitRSRGibbs
    from occuspytial_amd.utils import make_data
    Q, W, X, y = make_data(150, min_v=2, max_v=3, ns=60, p=9, q=2, random_state=3)[:4]
    with pytest.raises(ValueError, match='at most 8'):
        ProbitRSRGibbs(Q, W, X, y, q=5)


def test_a_library_without_the_probit_model_is_refused(monkeypatch, oracle):
    """The oracle's C ABI rebuilds with the new occ_problem layout but ignores `link`: it must not run the logit model
    on a probit problem in silence."""
    from occuspytial_amd import ProbitRSRGibbs, _lib
    if not os.path.exists(ABI_LIB) or os.path.getmtime(ABI_LIB) < os.path.getmtime(os.path.join(ROOT, 'oracle', 'occ_oracle_abi.c')):
        oracle.build()
    monkeypatch.setattr(_lib, 'LIB_PATH', ABI_LIB)
    monkeypatch.setattr(_lib, '_lib', None)
    assert _lib.load().occ_device_count() == 0
    Q, W, X, y = _data()
    s = ProbitRSRGibbs(Q, W, X, y, random_state=10, q=10)
    with pytest.raises(_lib.EngineUnavailable, match='does not implement the probit model'):
        s.sample(3, chains=1, progressbar=False)


def test_restatement_runs_the_dispersed_start_without_nans():
    """The restatement (with numpy's variates) stays finite from the default start that sends the reference to NaN."""
    from occuspytial_amd import ProbitRSRGibbs
    Q, W, X, y = _data()
    s = ProbitRSRGibbs(Q, W, X, y, random_state=10)
    s._initialize_posterior_state(None)
    prob = restatement_problem(s)
    st = dict(alpha=s.state.alpha, beta=s.state.beta, tau=s.state.tau, c=prob['Phi'].T @ s.state.spatial,
              eta=s.state.spatial, eps=s.state.eps, z=s._problem.z0.copy())
    rng = np.random.default_rng(1)
    n, m, R = X.shape[0], s.fixed.q, prob['W'].shape[0]
    for _ in range(30):
        var = dict(u_ob=rng.random(n), n_eps=rng.standard_normal(n), gamma=rng.standard_gamma(prob['tau_shape']),
                   xi=rng.standard_normal(m), n_beta=rng.standard_normal(3), u_oa=rng.random(R),
                   n_alpha=rng.standard_normal(2), u_z=rng.random(n))
        st = pr.step(prob, st, var)['state']
        for k, v in st.items():
            assert np.all(np.isfinite(v)), k


def restatement_problem(s):
    """The dict tests/_probit_reference.step takes, from a ProbitRSRGibbs."""
    P = s._problem
    pb = P.probit
    return dict(X=P.X, W=P.W, y=P.y, site_ptr=P.site_ptr, site_id=P.site_id, obs_site=P.obs_site, a_mu=P.a_mu,
                a_prec=P.a_prec, b_mu=P.b_mu, b_prec=P.b_prec, tau_rate=P.tau_rate, tau_shape=P.tau_shape,
                K=pb['K'], KTK=pb['KTK'], Qr=pb['Q'], Phi=pb['Phi'], G=pb['G'], lam=pb['lam'])


@pytest.mark.parametrize('case', ['ref_probit_r05', 'ref_probit_q10'])
def test_basis_and_default_start_match_the_reference(case):
    """K, Qr, KTK, m and tau_shape of the reference's _configure, and its default start bit for bit
    (tests/golden/make_golden_probit.py ran the reference's own code)."""
    from occuspytial_amd import ProbitRSRGibbs
    from .conftest import load_golden
    from .test_api_cpu import _inputs
    g = load_golden(case)
    Q, W, X, y, _ = _inputs(g)
    kw = {'q': int(g['basis_q'])} if int(g['basis_q']) else {'r': float(g['basis_r'])}
    s = ProbitRSRGibbs(Q, W, X, y, random_state=int(g['seed']), **kw)
    assert s.fixed.q == int(g['m'])
    assert s.fixed.tau_shape == float(g['tau_shape'])
    sign = np.sign(np.sum(s.fixed.K * g['K'], axis=0))   # (an eigenvector's sign is arbitrary)
    np.testing.assert_allclose(s.fixed.K * sign, g['K'], atol=1e-10)
    np.testing.assert_allclose(s.fixed.Q * np.outer(sign, sign), g['Qr'], atol=1e-10)
    np.testing.assert_allclose(s.fixed.KTK * np.outer(sign, sign), g['KTK'], atol=1e-12)
    np.testing.assert_array_equal(s.fixed.XTX_plus_bprec, g['XTX_plus_bprec'])
    s._initialize_posterior_state(None)
    assert s.state.tau == float(g['start_tau'])
    for name in ('alpha', 'beta', 'eta', 'eps'):
        assert np.array_equal(getattr(s.state, name), g['start_' + name]), name
