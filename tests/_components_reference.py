"""A dense numpy restatement of ``LogitICARGibbs`` under either sum-to-zero constraint, for small graphs.

Written from the model, in the order of the reference's seven conditionals (omega_b, tau, eta, beta, omega_a, alpha, z;
``gibbs/logit.py:254-266``).  What differs from the engine on purpose: eta is drawn by a dense Cholesky factor of
``Lambda = tau Q + diag(omega_b)`` and conditioned on ``A eta = 0`` by kriging (Rue & Held 2005, algorithm 2.6),
``eta = x - Lambda^-1 A' (A Lambda^-1 A')^-1 A x`` -- A the k x n indicator matrix of the components under
``'component'``, the row of ones under ``'global'`` -- and a site alone in its component gets exactly 0.  No MINRES, no
projection through ``Lambda^-1 1``, no edge form of the prior.  PG(1, c) comes from the oracle library where it loads
(``oracle.occ_oracle.pg1``), else from the sampler of Polson, Scott & Windle (2013, after Devroye) below.

``tests/golden/make_components_golden.py`` runs it once and stores the draws in ``tests/golden/components34.npz``.
"""
import math

import numpy as np
from scipy.linalg import cho_factor, cho_solve, solve_triangular
from scipy.special import expit, ndtr

T_PG = 0.64


def _a_coef(n, x):
    k = (n + 0.5) * math.pi
    if x > T_PG:
        return k * math.exp(-0.5 * k * k * x)
    return k * (2.0 / (math.pi * x)) ** 1.5 * math.exp(-2.0 * (n + 0.5) ** 2 / x)


def _trunc_inv_gauss(z, rng):
    """IG(mu = 1 / z, lambda = 1) truncated to (0, T_PG)."""
    if z < 1.0 / T_PG:
        while True:
            while True:
                e1, e2 = rng.standard_exponential(2)
                if e1 * e1 <= 2.0 * e2 / T_PG:
                    break
            x = T_PG / (1.0 + T_PG * e1) ** 2
            if rng.random() <= math.exp(-0.5 * z * z * x):
                return x
    mu = 1.0 / z
    while True:
        y = rng.standard_normal() ** 2
        x = mu + 0.5 * mu * mu * y - 0.5 * mu * math.sqrt(4.0 * mu * y + (mu * y) ** 2)
        if rng.random() > mu / (mu + x):
            x = mu * mu / x
        if x <= T_PG:
            return x


def pg1_devroye(c, rng):
    """One PG(1, c) draw: J*(1, |c| / 2) / 4 by the alternating-series method."""
    z = 0.5 * abs(float(c))
    K = math.pi ** 2 / 8.0 + 0.5 * z * z
    p = math.pi / (2.0 * K) * math.exp(-K * T_PG)
    if z > 0:
        q = 2.0 * math.exp(-z) * (ndtr(math.sqrt(1.0 / T_PG) * (T_PG * z - 1.0))
                                  + math.exp(2.0 * z) * ndtr(-math.sqrt(1.0 / T_PG) * (T_PG * z + 1.0)))
    else:
        q = 2.0 * 2.0 * ndtr(-math.sqrt(1.0 / T_PG))
    while True:
        if rng.random() < p / (p + q):
            x = T_PG + rng.standard_exponential() / K
        elif z > 0:
            x = _trunc_inv_gauss(z, rng)
        else:   # IG with infinite mean, truncated: the first branch of _trunc_inv_gauss without its acceptance step
            while True:
                e1, e2 = rng.standard_exponential(2)
                if e1 * e1 <= 2.0 * e2 / T_PG:
                    break
            x = T_PG / (1.0 + T_PG * e1) ** 2
        s = _a_coef(0, x)
        y = rng.random() * s
        n = 0
        while True:
            n += 1
            if n % 2 == 1:
                s -= _a_coef(n, x)
                if y <= s:
                    return 0.25 * x
            else:
                s += _a_coef(n, x)
                if y > s:
                    break


class PG:
    """PG(1, c) for arrays: the oracle library's keyed draws where it loads, else pg1_devroye from `rng`."""

    def __init__(self, rng, key):
        self.rng, self.key, self.calls = rng, int(key), 0
        try:
            from oracle import occ_oracle
            occ_oracle.lib()
            self.oracle = occ_oracle
        except Exception:
            self.oracle = None

    def __call__(self, c):
        c = np.ascontiguousarray(c, dtype=np.float64)
        self.calls += 1
        if self.oracle is not None:
            return self.oracle.pg1(c, key=self.key, it=self.calls, stream=1)
        return np.array([pg1_devroye(v, self.rng) for v in c])


def constraint_rows(labels, constraint):
    """A (rows x n): one row of ones (global), or the indicator of every component of more than one site."""
    n = labels.size
    if constraint == 'global':
        return np.ones((1, n)), np.zeros(n, dtype=bool)
    size = np.bincount(labels)
    rows = [(labels == c).astype(np.float64) for c in range(size.size) if size[c] > 1]
    return np.array(rows), size[labels] == 1


def mvn_from_precision(b, prec, rng):
    """N(prec^-1 b, prec^-1)."""
    cf = cho_factor(prec, lower=True)
    return cho_solve(cf, b) + solve_triangular(cf[0], rng.standard_normal(b.size), lower=True, trans='T')


def run_chain(g, constraint, size, seed, tau_shape=None, tau_rate=0.005, prec0=0.1, with_eta=False):
    """`size` iterations of one chain on the graph dict `g` (tests/_components_graphs.py).  -> (alpha, beta, tau) draws, and
    the last eta if asked."""
    rng = np.random.default_rng(seed)
    pg = PG(rng, key=0x5EED0000 + seed)
    Q = np.asarray(g['Q'].todense())
    X, n, labels = g['X'], g['n'], np.asarray(g['labels'])
    k = int(labels.max()) + 1
    if tau_shape is None:
        tau_shape = 0.5 + 0.5 * (n - (k if constraint == 'component' else 1))
    A, single = constraint_rows(labels, constraint)
    sites = sorted(g['W'])
    W = np.concatenate([g['W'][s] for s in sites])
    y = np.concatenate([g['y'][s] for s in sites])
    row_site = np.concatenate([np.full(len(g['y'][s]), s) for s in sites])
    detected = np.zeros(n, dtype=bool)
    for s in sites:
        detected[s] = g['y'][s].any()
    surveyed = np.zeros(n, dtype=bool)
    surveyed[sites] = True
    p, q = X.shape[1], W.shape[1]
    a_prec, b_prec = prec0 * np.eye(q), prec0 * np.eye(p)
    # start: the package's defaults in spirit -- z = 1 unless surveyed without a detection, everything else from the prior's scale
    z = np.where(surveyed & ~detected, 0.0, 1.0)
    alpha, beta, tau = rng.standard_normal(q), rng.standard_normal(p), 1.0
    eta = np.zeros(n)
    out_a, out_b, out_t = np.empty((size, q)), np.empty((size, p)), np.empty(size)
    for it in range(size):
        omega_b = pg(X @ beta + eta)
        tau = rng.gamma(tau_shape, 1.0 / (0.5 * eta @ Q @ eta + tau_rate))
        # eta | rest, A eta = 0
        lam = tau * Q + np.diag(omega_b)
        cf = cho_factor(lam, lower=True)
        kk = z - 0.5
        x = cho_solve(cf, kk - omega_b * (X @ beta)) + solve_triangular(cf[0], rng.standard_normal(n), lower=True, trans='T')
        V = cho_solve(cf, A.T)
        eta = x - V @ np.linalg.solve(A @ V, A @ x)
        eta[single] = 0.0
        # beta | rest
        beta = mvn_from_precision(X.T @ (kk - omega_b * eta), (X.T * omega_b) @ X + b_prec, rng)
        # omega_a, alpha | rest: the visits of the sites that exist (z = 1)
        live = z[row_site] == 1.0
        Wl = W[live]
        omega_a = pg(Wl @ alpha)
        alpha = mvn_from_precision(Wl.T @ (y[live] - 0.5), (Wl.T * omega_a) @ Wl + a_prec, rng)
        # z | rest
        psi = expit(X @ beta + eta)
        miss = np.ones(n)
        np.multiply.at(miss, row_site, expit(-(W @ alpha)))
        pz = np.where(surveyed, psi * miss / ((1.0 - psi) + psi * miss), psi)
        z = np.where(detected, 1.0, (rng.random(n) < pz).astype(np.float64))
        out_a[it], out_b[it], out_t[it] = alpha, beta, tau
    return (out_a, out_b, out_t, eta) if with_eta else (out_a, out_b, out_t)


def batch_means_mcse(x):
    """Monte-Carlo standard error of the mean of `x` (chains, draws) by batch means: batches of floor(sqrt(draws)) within a
    chain, the chains' variance estimates averaged."""
    x = np.asarray(x, dtype=np.float64)
    C, N = x.shape
    L = int(math.floor(math.sqrt(N)))
    nb = N // L
    var = []
    for c in range(C):
        means = x[c, :nb * L].reshape(nb, L).mean(axis=1)
        var.append(L * means.var(ddof=1))
    return math.sqrt(np.mean(var) / (C * N))
