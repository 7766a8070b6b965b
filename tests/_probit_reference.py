"""A numpy restatement of one iteration of ``ProbitRSRGibbs`` with injected variates.

Written from the model (DESIGN.md "ProbitRSRGibbs"), not from the reference's code: the reference's ``step`` loses the beta
precision after its first call and draws its truncated normals with a formula that overflows past |loc| ~ 38.  Here the
beta precision ``M = X'X + b_prec`` is never touched, and the truncated normal is the stable inverse CDF the engine uses
(``occ_probit.hpp``), statement for statement, so that a device draw and this one agree to rounding.

Truncated normal.  ``tn_pos(loc, U)`` is N(loc, 1) truncated to (0, inf) at the uniform U, i.e. the reference's
``loc - ndtri(ndtr(loc) (1 - U))``; ``tn_neg(loc, U)`` truncates to (-inf, 0): ``loc + ndtri(ndtr(-loc) U)``.  Both are
``+-excess(a, v, w, E)``: the x >= 0 with ``Q(a + x) = Q(a) v`` (Q the upper normal tail), given ``v``, ``w = 1 - v`` and
``E = -log v`` each to full accuracy.
  * a <= 0 (the truncation point lies below the mode): the inverse CDF directly, on whichever of ``q = Q(a) v`` and
    ``1 - q = Phi(a) + Q(a) w`` is below 1/2, so no probability near 1 is ever formed; x = N - a.  Where x < |a| / 32 the
    subtraction has cost more than 64 ulp and x is refined as below (max(|a|, 1): near a = 0, q lies near 1/2).
  * a > 0 (the draw lies in the tail beyond the truncation point), and refinement: Newton's method on
    ``h(x) = -log(Q(a + x) / Q(a)) = int_a^{a+x} H(y) dy = E``, H the normal hazard ``phi / Q = sqrt(2/pi) / erfcx(y/sqrt 2)``,
    h by 16-point Gauss-Legendre quadrature, ``h' = H(a + x)``.  h is increasing and convex, so Newton's method converges
    monotonically once it is above the root; the start ``2E / (a + sqrt(a^2 + 2E))`` (the root for H(y) = y < H(y)) is.
    Every term is a product or a sum of positive terms: x has a relative error of a few ulp for any a, and is finite for
    every finite loc and U in (0, 1).
"""
import numpy as np
from scipy.special import erfc, erfcx, ndtr

SQRT_HALF = 0.70710678118654752440
SQRT_2_OVER_PI = 0.79788456080286535588
_GL_X, _GL_W = np.polynomial.legendre.leggauss(16)
GL_T = (_GL_X + 1.0) / 2.0   # nodes on [0, 1]
GL_W = _GL_W / 2.0           # weights summing to 1

# AS 241 (Wichura 1988), PPND16
_A = (3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
      4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3)
_B = (1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
      3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3)
_C = (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
      1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
_D = (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
      1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
_E = (6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
      2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
_F = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
      1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def _poly(c, r):
    out = np.full_like(r, c[7])
    for k in range(6, -1, -1):
        out = out * r + c[k]
    return out


def ndtri_as241(p):
    """Phi^-1(p), p in (0, 1): AS 241 plus one Newton step on Phi (both tails to about an ulp)."""
    p = np.asarray(p, dtype=np.float64)
    q = p - 0.5
    central = np.abs(q) <= 0.425
    rc = 0.180625 - q * q
    xc = q * _poly(_A, rc) / _poly(_B, rc)
    r = np.sqrt(-np.log(np.where(q < 0, p, 1.0 - p)))
    r1, r2 = r - 1.6, r - 5.0
    xt = np.where(r <= 5.0, _poly(_C, r1) / _poly(_D, r1), _poly(_E, r2) / _poly(_F, r2))
    xt = np.where(q < 0, -xt, xt)
    # one Newton step, on the tail that holds p (Phi(x) - p, formed as a difference of two small numbers)
    lo = q < 0
    cdf = np.where(lo, 0.5 * erfc(-xt * SQRT_HALF), 0.5 * erfc(xt * SQRT_HALF))
    tgt = np.where(lo, p, 1.0 - p)
    pdf = np.exp(-0.5 * xt * xt) * (SQRT_2_OVER_PI / 2.0)
    step = np.where(lo, cdf - tgt, tgt - cdf) / pdf
    xt = np.where(np.isfinite(step), xt - step, xt)
    return np.where(central, xc, xt)


def hazard(y):
    """phi(y) / Q(y)."""
    return SQRT_2_OVER_PI / erfcx(np.asarray(y) * SQRT_HALF)


def _newton(a, E, x):
    x = np.array(x, dtype=np.float64, copy=True)
    active = np.ones(x.shape, dtype=bool)
    for _ in range(40):
        s = np.zeros_like(x)
        for t, w in zip(GL_T, GL_W):
            s = w * hazard(x * t + a) + s
        dx = (x * s - E) / hazard(a + x)
        x = np.where(active, x - dx, x)
        active &= np.abs(dx) > 1e-14 * np.abs(x)
        if not active.any():
            break
    return x


def excess(a, v, w, E):
    """x >= 0 with Q(a + x) = Q(a) v, given v, w = 1 - v and E = -log v (see the module docstring)."""
    a, v, w, E = np.broadcast_arrays(*(np.asarray(t, dtype=np.float64) for t in (a, v, w, E)))
    out = np.empty(a.shape)
    tail = a > 0
    if tail.any():
        at, Et = a[tail], E[tail]
        x0 = 2.0 * Et / (at + np.sqrt(at * at + 2.0 * Et))
        out[tail] = _newton(at, Et, x0)
    body = ~tail
    if body.any():
        ab, vb, wb, Eb = a[body], v[body], w[body], E[body]
        Qa = 0.5 * erfc(ab * SQRT_HALF)
        Pa = 0.5 * erfc(-ab * SQRT_HALF)
        q = Qa * vb
        with np.errstate(invalid='ignore', divide='ignore'):
            N = np.where(q <= 0.5, -ndtri_as241(np.minimum(q, 0.5)), ndtri_as241(np.minimum(Qa * wb + Pa, 0.5)))
        x = N - ab
        bad = x < np.maximum(-ab, 1.0) / 32.0
        if bad.any():
            x[bad] = _newton(ab[bad], Eb[bad], np.maximum(x[bad], 0.0))
        out[body] = x
    return out


def tn_pos(loc, U):
    """N(loc, 1) truncated to (0, inf) at uniform U: the reference's loc - ndtri(ndtr(loc) (1 - U)), stably."""
    loc, U = np.broadcast_arrays(np.asarray(loc, dtype=np.float64), np.asarray(U, dtype=np.float64))
    return excess(-loc, 1.0 - U, U, -np.log1p(-U))


def tn_neg(loc, U):
    """N(loc, 1) truncated to (-inf, 0) at uniform U: the reference's loc + ndtri(ndtr(-loc) U), stably."""
    loc, U = np.broadcast_arrays(np.asarray(loc, dtype=np.float64), np.asarray(U, dtype=np.float64))
    return -excess(loc, U, 1.0 - U, -np.log(U))


def tn_reference_formula(loc, U, positive):
    """The reference's own inverse CDF (probit.py truncnorm_*_ppf), accurate only for small |loc|."""
    from scipy.special import ndtri
    loc = np.asarray(loc, dtype=np.float64)
    if positive:
        return -ndtri(ndtr(loc) * (1.0 - U)) + loc
    return ndtri(ndtr(-loc) * U) + loc


# ---- the fixed quantities ---------------------------------------------------------------------------------------
def eigen_basis(KTK, Qr):
    """G, lam of the generalized problem Qr G = KTK G diag(lam), G' KTK G = I (lam < 0 from rounding clamped to 0)."""
    from scipy.linalg import eigh
    lam, G = eigh(Qr, KTK)
    return np.ascontiguousarray(G), np.clip(lam, 0.0, None)


def cholesky_upper(M):
    return np.linalg.cholesky(M).T


def precision_draw(A, b, eps):
    """x ~ N(A^-1 b, A^-1) with the upper Cholesky factor U of A (A = U'U): A^-1 b + U^-1 eps -- the reference's
    precision_mvnorm, and the engine's precision_mvnorm_dev."""
    from scipy.linalg import solve_triangular
    U = cholesky_upper(A)
    o = U.T @ eps + b
    v = solve_triangular(U, o, trans='T', lower=False)
    return solve_triangular(U, v, lower=False)


# ---- one iteration ------------------------------------------------------------------------------------------------
def step(prob, st, var, theta_form='c'):
    """One iteration of one chain in the reference's order: omega_b, tau, eps, theta, beta, omega_a, alpha, z.

    ``prob``: dict with X (n x p), W (R x q), y (R), site_ptr (S + 1), site_id (S), obs_site (S), a_mu, a_prec, b_mu,
    b_prec, tau_rate, tau_shape, and the basis: K, KTK, Qr; Phi = K G, G, lam.
    ``st``: dict with alpha, beta, tau, c (the engine's coordinates; theta = G c), eta (= K theta), eps, z.
    ``var``: the variates -- u_ob (n), n_eps (n), gamma (the standard gamma variate of tau), xi (m), n_beta (p),
    u_oa (R), n_alpha (q), u_z (n).
    theta_form 'c': c = D u + D^1/2 xi (the engine's form); 'chol': theta = A^-1 b + U^-1 xi with A = KTK + tau Qr
    (the reference's form; then ``var['xi']`` are the normals of the Cholesky form and c = G^-1 theta).
    Returns the new state and the intermediate quantities."""
    X, W, y = prob['X'], prob['W'], prob['y']
    n, p = X.shape
    q = W.shape[1]
    site_ptr, site_id, obs_site = prob['site_ptr'], prob['site_id'], prob['obs_site']
    alpha, beta, tau = np.asarray(st['alpha'], float), np.asarray(st['beta'], float), float(st['tau'])
    c, eta, eps, z = (np.asarray(st[k], float) for k in ('c', 'eta', 'eps', 'z'))
    lam, Phi, G = prob['lam'], prob['Phi'], prob['G']
    out = {}
    # omega_b
    xb = X @ beta
    loc = xb + eta + eps
    ob = np.where(z == 1, tn_pos(loc, var['u_ob']), tn_neg(loc, var['u_ob']))
    out['omega_b'] = ob
    # tau (from the current theta: theta' Qr theta = c' diag(lam) c)
    rate = 0.5 * np.sum(lam * c * c) + prob['tau_rate']
    tau = var['gamma'] / rate
    out['tau'] = tau
    # eps
    eps = 0.5 * (ob - xb - eta) + SQRT_HALF * var['n_eps']
    out['eps'] = eps
    # theta
    s = ob - xb - eps
    if theta_form == 'c':
        u = Phi.T @ s
        D = 1.0 / (1.0 + tau * lam)
        c = D * u + np.sqrt(D) * var['xi']
        theta = G @ c
        eta = Phi @ c
    else:
        A = prob['KTK'] + tau * prob['Qr']
        theta = precision_draw(A, prob['K'].T @ s, var['xi'])
        c = np.linalg.solve(G, theta)
        eta = prob['K'] @ theta
    out['c'], out['theta'], out['eta'] = c, theta, eta
    # beta, from the fixed precision X'X + b_prec
    M = X.T @ X + prob['b_prec']
    bb = prob['b_prec'] @ prob['b_mu'] + X.T @ (ob - eta - eps)
    beta = precision_draw(M, bb, var['n_beta'])
    out['beta'] = beta
    # omega_a over the rows of existing sites (a detection, or z = 1), then alpha
    S = len(site_id)
    exists = np.array([bool(obs_site[t]) or z[site_id[t]] == 1 for t in range(S)], dtype=bool)
    rows = np.concatenate([np.arange(site_ptr[t], site_ptr[t + 1]) for t in range(S) if exists[t]] or [np.zeros(0, int)])
    la = W[rows] @ alpha
    ua = var['u_oa'][rows]
    oa_rows = np.where(y[rows] == 1, tn_pos(la, ua), tn_neg(la, ua))
    oa = np.zeros(W.shape[0])
    oa[rows] = oa_rows
    out['omega_a'], out['exists'] = oa, exists
    We = W[rows]
    A = We.T @ We + prob['a_prec']
    ba = prob['a_prec'] @ prob['a_mu'] + We.T @ oa_rows
    alpha = precision_draw(A, ba, var['n_alpha'])
    out['alpha'] = alpha
    # z
    loc = X @ beta + eta + eps
    pz = ndtr(loc)
    qz = ndtr(-loc)
    znew = z.copy()
    surveyed = np.zeros(n, dtype=bool)
    surveyed[site_id] = True
    for t in range(S):
        i = site_id[t]
        if obs_site[t]:
            continue
        r = np.arange(site_ptr[t], site_ptr[t + 1])
        prod = np.prod(ndtr(-(W[r] @ alpha))) if r.size else 1.0
        num = pz[i] * prod
        pr = num / (qz[i] + num)
        znew[i] = 1.0 if var['u_z'][i] < pr else 0.0
    ns = np.flatnonzero(~surveyed)
    znew[ns] = (var['u_z'][ns] < pz[ns]).astype(float)
    out['z'] = znew
    out['state'] = dict(alpha=alpha, beta=beta, tau=tau, c=c, eta=eta, eps=eps, z=znew)
    return out
