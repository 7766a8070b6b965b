"""The high-precision reference of the reduced-rank theta conditional (tests/_rsr_reference.py) against exact rational
arithmetic and mpmath, and the CPU oracle's theta (what every GPU lock-step test of the reduced-rank model compares with)
against that reference: an accuracy statement for the lock-step yardstick of its own."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from . import _rsr_reference as R


def _frac(x):
    """Exact rational value of a float64 or long-double number."""
    return Fraction(*x.as_integer_ratio())


def test_gram_hp_is_exact_to_long_double():
    """K' diag(omega) K of a 37 x 6 K with mixed signs and magnitudes over four decades, omega spread over 1e-5 ... 0.25:
    every entry within 2^-62 of |K|' diag(omega) |K| (~1e-19) of the exact rational sum."""
    rng = np.random.default_rng(3)
    n, m = 37, 6
    K = rng.standard_normal((n, m)) * 10.0 ** rng.uniform(-2, 2, (n, m))
    omega = np.exp(rng.uniform(np.log(1e-5), np.log(0.25), n))
    G = R.gram_hp(K, omega)
    A = np.abs(K).T @ (omega[:, None] * np.abs(K))
    worst = 0.0
    for a in range(m):
        for c in range(m):
            exact = sum(_frac(K[i, a]) * _frac(omega[i]) * _frac(K[i, c]) for i in range(n))
            worst = max(worst, abs(float(_frac(G[a, c]) - exact)) / A[a, c])
    assert worst < 2.0 ** -62, worst
    # and plain float64 is not: the test can tell the two apart
    G64 = K.T @ (omega[:, None] * K)
    assert np.max(np.abs((G64 - G).astype(float)) / A) > 2.0 ** -56


def test_gram_hp_is_exact_at_the_cap_sites_count():
    """n = 4 160 sites (the largest GPU test's lattice; slices of s = 20 bits, where n 2^(2 s) is just below 2^53), an
    orthonormal K of 24 columns: a dozen entries within 2^-62 of |K|' diag(omega) |K| of the exact rational sum."""
    rng = np.random.default_rng(4160)
    n, m = 4160, 24
    K = np.linalg.qr(rng.standard_normal((n, m)))[0]
    omega = np.exp(rng.uniform(np.log(1e-5), np.log(0.25), n))
    G = R.gram_hp(K, omega)
    A = np.abs(K).T @ (omega[:, None] * np.abs(K))
    fk = [[_frac(v) for v in K[:, a]] for a in range(m)]
    fo = [_frac(v) for v in omega]
    worst = 0.0
    for a, c in [(0, 0), (0, 23), (3, 7), (5, 5), (11, 12), (23, 23), (17, 2), (8, 19), (1, 22), (14, 14), (20, 9), (6, 16)]:
        exact = sum(x * w * y for x, w, y in zip(fk[a], fo, fk[c]))
        worst = max(worst, abs(float(_frac(G[a, c]) - exact)) / A[a, c])
    assert worst < 2.0 ** -62, worst


def _spd(m, kap, rng):
    Q1 = np.linalg.qr(rng.standard_normal((m, m)))[0]
    return (Q1 * np.logspace(0.0, -np.log10(kap), m)) @ Q1.T


@pytest.mark.parametrize('kap', [1e2, 1e6, 1e10])
def test_theta_hp_against_mpmath(kap):
    """Lam^-1 r for a 40 x 40 Lam of condition number kap, Lam held in long double (the sum of a float64 matrix and a small
    perturbation, as a Gram matrix plus tau Qr is): within 1e-3 of 2 m u kappa (what a float64 solve may be held to) of
    mpmath.lu_solve at 50 digits."""
    rng = np.random.default_rng(int(np.log10(kap)))
    m = 40
    Lam = _spd(m, kap, rng).astype(R.LD)
    Lam = Lam + R.LD(2.0 ** -60) * np.asarray(Lam.astype(np.float64) * rng.uniform(-1, 1, (m, m)), dtype=R.LD)
    Lam = (Lam + Lam.T) / 2
    r = rng.standard_normal(m).astype(R.LD) * (1 + R.LD(2.0 ** -58))
    th = R.theta_hp(Lam, r)
    with mpmath.workdps(50):
        A = mpmath.matrix([[mpmath.mpf(_frac(Lam[i, j]).numerator) / _frac(Lam[i, j]).denominator for j in range(m)] for i in range(m)])
        b = mpmath.matrix([mpmath.mpf(_frac(v).numerator) / _frac(v).denominator for v in r])
        x = mpmath.lu_solve(A, b)
        err = float(mpmath.norm(mpmath.matrix([mpmath.mpf(_frac(th[i]).numerator) / _frac(th[i]).denominator - x[i] for i in range(m)]))
                    / mpmath.norm(x))
    k = R.kappa(Lam)
    bound = 2 * m * R.U * k
    print(f'theta_hp m={m} kappa={k:.2e} err={err:.2e} (1e-3 of 2 m u kappa: {1e-3 * bound:.2e})')
    assert 0.3 * kap < k < 3 * kap
    assert err <= 1e-3 * bound, (err, bound)


def _rsr_case(m, kap, seed):
    """A reduced-rank system of m columns on n = m + 64 sites: K orthonormal, Qr = K'(D - A)K of a path graph's ICAR
    precision, E from eigh(Qr), then reparameterised (tests/_rsr_reference.reparam) to kappa(Lam) ~ kap."""
    rng = np.random.default_rng(seed)
    n = m + 64
    K = np.linalg.qr(rng.standard_normal((n, m)))[0]
    Qn = np.diag(np.r_[1.0, 2.0 * np.ones(n - 2), 1.0]) - np.eye(n, k=1) - np.eye(n, k=-1)
    Qr = K.T @ Qn @ K
    Qr = 0.5 * (Qr + Qr.T)
    s, u = np.linalg.eigh(Qr)
    E = u * np.sqrt(np.clip(s, 0.0, None))
    omega = np.exp(rng.uniform(np.log(1e-3), np.log(0.25), n))
    tau = 1.5
    _, M = R.spread_for(K, Qr, omega, tau, kap, rng)
    K, Qr, E = R.reparam(K, Qr, E, M)
    b = rng.integers(0, 2, n) - 0.5 - omega * rng.normal(0, 2, n)
    return K, Qr, E, b, omega, tau, rng.standard_normal(n), rng.standard_normal(m)


@pytest.mark.parametrize('kap', [1e2, 1e6, 1e10])
@pytest.mark.parametrize('m', [17, 129, 333])
def test_oracle_rsr_theta_is_as_accurate_as_numpy(oracle, m, kap):
    """orc_rsr_theta (the oracle's float64 Gram matrix, Cholesky and substitutions) from injected normals: its error
    against theta_hp is within 10 x that of the reference's own float64 arithmetic (numpy_theta) + 64 u."""
    K, Qr, E, b, omega, tau, e1, e2 = _rsr_case(m, kap, m)
    Lam = R.lam_hp(K, Qr, omega, tau)
    th_hp = R.theta_hp(Lam, R.rhs_hp(K, b, omega, e1, E, e2, tau))
    th_orc, code = oracle.rsr_theta(K, Qr, E, b, omega, tau, e1, e2)
    assert code == 0
    err_orc = R.rel_err(th_orc, th_hp)
    err_np = R.rel_err(R.numpy_theta(K, Qr, E, b, omega, tau, e1, e2), th_hp)
    k = R.kappa(Lam)
    print(f'oracle m={m} kappa={k:.2e} err_orc={err_orc:.2e} err_np={err_np:.2e}')
    assert 0.1 * kap < k < 10 * kap
    assert err_orc <= 10 * err_np + 64 * R.U, (err_orc, err_np)
