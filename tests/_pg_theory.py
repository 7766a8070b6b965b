"""Closed forms of the Polya-Gamma law PG(1, z) for the tests, finite and accurate at every finite z.

Plain numpy / scipy (no mpmath at run time); tests/test_oracle_rng.py checks these forms against mpmath quadrature of the
density and against high-precision evaluation.  Polson, Scott & Windle (2013), "Bayesian inference for logistic models
using Polya-Gamma latent variables", JASA 108: PG(1, z) has the Laplace transform cosh(z/2) / cosh(sqrt((z^2/2 + t)/2)),
hence the mean and variance below.

The CDF: with b = |z|, 4 X ~ PG(1, z) scaled by 4 has the Laplace transform cosh(b/2) / cosh(sqrt(b^2/4 + 2 s)) of the
time Brownian motion with drift b/2 takes to leave (-1, 1) from 0; rescaling time by 4 and space by 2, X itself is the
time Brownian motion with drift b takes to leave (-1/2, 1/2).  The method of images for two absorbing barriers (Cox &
Miller 1965, "The Theory of Stochastic Processes", ch. 5) gives, with a_n = n + 1/2 and Phi the standard normal CDF,

    F(x) = sum_n (-1)^n 2 cosh(b/2) [exp(-a_n b) Phi((b x - a_n) / sqrt x) + exp(a_n b) Phi(-(b x + a_n) / sqrt x)].

Both products are formed without overflow or cancellation: 2 cosh(b/2) exp(-a_n b) = (1 + e^-b) e^(-n b), and with
w = (b x - a_n) / sqrt x, y = (b x + a_n) / sqrt x the second product is (1 + e^-b) e^(-n b) e^(-w^2/2) erfcx(y / sqrt 2) / 2
(Phi(-y) = erfcx(y / sqrt 2) e^(-y^2/2) / 2 and y^2 - w^2 = 4 a_n b).  For b > 0 the terms fall as e^(-n b); at b = 0 the
sum converges once a_n >> sqrt x, so the default 400 terms serve every x < ~2 000.
"""
import numpy as np
from scipy import special

# The sampler's branch on Z = |z| / 2 against 1 / t (t = 0.64) sits at |z| = 3.125.  From |z| = PG_OVERFLOW on, the
# probability of the right piece of its envelope, 1 / (1 + k f exp(f t - Z)), has an infinite denominator; from
# PG_SUBNORMAL on the denominator is at least 2^1022 and its reciprocal subnormal.  Both bisected on the oracle's
# arithmetic (tests/test_oracle_rng.py checks them).
PG_BRANCH = 3.125
PG_OVERFLOW = 96.83100867754516
PG_SUBNORMAL = 96.73862732109177


def pg_mean(z):
    """E PG(1, z) = tanh(z/2) / (2 z); its Taylor series near 0."""
    z = np.abs(np.asarray(z, dtype=float))
    small = z < 1e-2
    zs = np.where(small, 1.0, z)
    zz = np.where(small, z, 0.0) ** 2
    series = 0.25 - zz / 48 + zz * zz / 480 - 17 * zz ** 3 / 80640
    out = np.where(small, series, np.tanh(zs / 2) / (2 * zs))
    return out if out.ndim else float(out)


def pg_var(z):
    """Var PG(1, z) = (2 tanh(z/2) - z sech^2(z/2)) / (4 z^3), sech^2 formed as 4 e^-|z| / (1 + e^-|z|)^2 (finite for any
    z); its Taylor series where the numerator cancels."""
    z = np.abs(np.asarray(z, dtype=float))
    small = z < 5e-2
    zs = np.where(small, 1.0, z)
    zz = np.where(small, z, 0.0) ** 2
    e = np.exp(-zs)
    sech2 = 4 * e / (1 + e) ** 2
    series = 1 / 24 - zz / 120 + 17 * zz * zz / 13440 - 31 * zz ** 3 / 181440
    out = np.where(small, series, (2 * np.tanh(zs / 2) - zs * sech2) / (4 * zs ** 3))
    return out if out.ndim else float(out)


def pg_laplace(z, t):
    """E exp(-t X), X ~ PG(1, z): cosh(z/2) / cosh(s), s = sqrt((z^2/2 + t)/2), as exp(|z|/2 - s) (1 + e^-|z|) / (1 + e^-2s)
    with |z|/2 - s = -t / (|z| + 2 s) (s^2 = z^2/4 + t/2: no cancellation at large |z|)."""
    b = np.abs(np.asarray(z, dtype=float))
    s = np.sqrt((b * b / 2 + t) / 2)
    out = np.exp(-t / (b + 2 * s)) * (1 + np.exp(-b)) / (1 + np.exp(-2 * s))
    return out if out.ndim else float(out)


def pg_cdf(x, z, terms=400):
    """P(X <= x), X ~ PG(1, z): the image series of the module docstring, vectorised over x (z a scalar).  For b > 0 the
    series stops once e^(-n b) < e^-40."""
    x = np.asarray(x, dtype=float)
    b = abs(float(z))
    if b > 0:
        terms = min(terms, 2 + int(40.0 / b))
    n = np.arange(terms, dtype=float)
    a = n + 0.5
    scale = (1 + np.exp(-b)) * np.exp(-n * b) * np.where(n % 2 == 0, 1.0, -1.0)
    flat = x.ravel()
    F = np.zeros(flat.size)
    step = max(1, 2_000_000 // terms)
    for i in range(0, flat.size, step):
        xs = flat[i:i + step]
        xs = np.where(xs > 0, xs, 1.0)[:, None]
        rx = np.sqrt(xs)
        w = (b * xs - a) / rx
        y = (b * xs + a) / rx
        with np.errstate(under='ignore', over='ignore'):
            t = special.ndtr(w) + 0.5 * np.exp(-0.5 * w * w) * special.erfcx(y / np.sqrt(2.0))
        F[i:i + step] = t @ scale
    out = np.where(flat > 0, np.clip(F, 0.0, 1.0), 0.0).reshape(x.shape)
    return out if out.ndim else float(out)
