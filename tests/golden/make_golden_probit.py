#!/usr/bin/env python
"""Generate the ProbitRSRGibbs fixtures ``tests/golden/ref_probit_*.npz`` by RUNNING THE REFERENCE's own probit code.

Run in the build container only (needs ``/root/reference``; the GPU box never has it)::

    python tests/golden/make_golden_probit.py

The reference is built as ``make_golden.py`` builds it (its ``build_reference``: the Cython modules cythonized from a
scratch copy under ``/tmp``, import shims for ``polyagamma`` and ``arviz``, which the probit sampler does not call).
``gibbs/probit.py`` runs unmodified.  The inputs come from ``occuspytial_amd.utils.make_data`` (the reference's
``make_data`` needs libpysal), with the shape of the reference's ``test_samplers.py``: 150 sites, p = 3, q = 2.

Each fixture holds, for one basis rule (``r = 0.5`` and ``q = 10``):
  * the inputs, the basis ``K``, ``Qr = K'QK``, ``KTK``, ``m`` and ``tau_shape`` of the reference's ``_configure``;
  * the default start of ``random_state = seed`` (tau, alpha, beta, eta = theta, eps, spatial);
  * the inputs, the variates and the outputs of the FIRST call of every ``_update_*``, in the reference's order, from a
    moderate state.  The first call is correct in the reference: beta is drawn from a corrupted precision only from its
    second call on (``precision_mvnorm`` overwrites ``XTX_plus_bprec`` with its factor).
Every variate is recovered by replaying a clone of the SFC64 state taken just before the call.
"""
import os
import sys

import numpy as np
from scipy import sparse

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from make_golden import build_reference, clone_rng, flatten  # noqa: E402


def probit_data():
    from occuspytial_amd.utils import make_data
    return make_data(150, min_v=2, max_v=4, ns=75, p=3, q=2, random_state=10)[:4]


def capture_probit_case(name, Q, W, X, y, seed, **basis):
    from occuspytial.gibbs.probit import ProbitRSRGibbs

    out = {}
    Qc = sparse.csr_matrix(Q).astype(float)
    Qc.sort_indices()
    n, p = X.shape
    q = next(iter(W.values())).shape[1]
    sites, visits, Wf, yf = flatten(W, y, q)
    out.update(Q_indptr=Qc.indptr.astype(np.int64), Q_indices=Qc.indices.astype(np.int64), Q_data=Qc.data,
               X=X, sites=sites, visits=visits, W_flat=Wf, y_flat=yf, seed=np.int64(seed),
               basis_r=np.float64(basis.get('r', 0.5)), basis_q=np.int64(basis.get('q') or 0))
    s = ProbitRSRGibbs(Q, W, X, y, random_state=seed, **basis)
    f = s.fixed
    m = int(f.q)
    out.update(m=np.int64(m), K=np.asarray(f.K), Qr=np.asarray(f.Q), KTK=np.asarray(f.KTK),
               tau_shape=np.float64(f.tau_shape), tau_rate=np.float64(f.tau_rate), a_mu=f.a_mu, a_prec=f.a_prec,
               b_mu=f.b_mu, b_prec=f.b_prec, XTX_plus_bprec=np.asarray(f.XTX_plus_bprec).copy())
    s._initialize_posterior_state(None)
    st = s.state
    out.update(start_tau=np.float64(st.tau), start_alpha=st.alpha.copy(), start_beta=st.beta.copy(),
               start_eta=st.eta.copy(), start_eps=st.eps.copy(), start_spatial=st.spatial.copy())

    # a moderate state (the default start puts theta ~ N(0, 25): linear predictors far beyond the reference's accurate range)
    g = np.random.default_rng(1234)
    st.alpha = np.array([0.4, -0.3])[:q].copy()
    st.beta = np.array([0.2, -0.3, 0.1])[:p].copy()
    st.tau = 1.5
    st.eta = 0.3 * g.standard_normal(m)
    st.spatial = f.K @ st.eta
    st.eps = 0.5 * g.standard_normal(n)
    st.z = st.z.copy()
    out.update(in_alpha=st.alpha.copy(), in_beta=st.beta.copy(), in_tau=np.float64(st.tau), in_theta=st.eta.copy(),
               in_spatial=st.spatial.copy(), in_eps=st.eps.copy(), in_z=st.z.copy())

    # omega_b: uniforms of the sites with z = 1 first, then of the others (probit.py _update_omega_b)
    c = clone_rng(s.rng)
    s._update_omega_b()
    mask = st.z == 1
    u = np.empty(n)
    u[mask] = c.random(int(mask.sum()))
    u[~mask] = c.random(int((~mask).sum()))
    out.update(ob_u=u, omega_b=st.omega_b.copy())
    # tau
    c = clone_rng(s.rng)
    s._update_tau()
    out.update(tau_g=np.float64(c.standard_gamma(f.tau_shape)), tau=np.float64(st.tau))
    # eps
    c = clone_rng(s.rng)
    s._update_eps()
    out.update(eps_n=c.standard_normal(n), eps=st.eps.copy())
    # theta (precision_mvnorm draws its n standard normals first)
    c = clone_rng(s.rng)
    s._update_eta()
    out.update(theta_n=c.standard_normal(m), theta=st.eta.copy(), spatial=st.spatial.copy())
    # beta: its FIRST call, from the intact precision
    assert np.array_equal(f.XTX_plus_bprec, out['XTX_plus_bprec'])
    c = clone_rng(s.rng)
    s._update_beta()
    out.update(beta_n=c.standard_normal(p), beta=st.beta.copy())
    # omega_a: rows of state.W (existing sites, reference order), uniforms of the y = 1 rows first, then of the others
    c = clone_rng(s.rng)
    s._update_omega_a()
    yrows = np.asarray(s.y[st.exists]) == 1
    ua = np.empty(yrows.size)
    ua[yrows] = c.random(int(yrows.sum()))
    ua[~yrows] = c.random(int((~yrows).sum()))
    out.update(oa_exists=np.asarray(st.exists, dtype=np.int64), oa_W=np.asarray(st.W).copy(), oa_y=yrows.astype(np.int64),
               oa_u=ua, omega_a=st.omega_a.copy())
    # alpha
    c = clone_rng(s.rng)
    s._update_alpha()
    out.update(alpha_n=c.standard_normal(q), alpha=st.alpha.copy())
    # z: uniforms of the surveyed sites without a detection, then of the unsurveyed sites
    c = clone_rng(s.rng)
    s._update_z()
    out.update(z_no=np.asarray(f.not_obs, dtype=np.int64), z_ns=np.asarray(f.not_surveyed, dtype=np.int64),
               z_u_no=c.uniform(size=f.n_no), z_u_ns=c.uniform(size=f.n_ns) if f.n_ns else np.zeros(0), z=st.z.copy())
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **out)
    print(name, 'n =', n, 'basis columns =', m, 'bytes =', os.path.getsize(os.path.join(HERE, name + '.npz')))


def main():
    build_reference()
    Q, W, X, y = probit_data()
    capture_probit_case('ref_probit_r05', Q, W, X, y, seed=10)
    capture_probit_case('ref_probit_q10', Q, W, X, y, seed=11, q=10)


if __name__ == '__main__':
    main()
