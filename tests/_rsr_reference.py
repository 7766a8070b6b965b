"""High-precision reference of the reduced-rank model's theta conditional (LogitRSRGibbs) for the tests.

theta ~ N(Lam^-1 r, Lam^-1) with Lam = K' diag(omega) K + tau Qr and r = K'(b + sqrt(omega) eps1) + sqrt(tau) E eps2
(occ_rsr.hpp).  Plain numpy / scipy; tests/test_rsr_reference_cpu.py checks these forms against exact rational arithmetic
and mpmath.

The Gram matrix K' diag(omega) K is what costs at the basis cap (n = 4 160 sites, m = 4 096 columns): a long-double matmul
runs at ~0.15 GMAC/s, so it is formed by an error-free splitting on float64 BLAS instead (Ozaki, Ogita, Oishi & Rump 2012,
"Error-free transformations of matrix multiplication by using fast routines of matrix multiplication and its
applications", Numer. Algorithms 59): B = diag(omega) K is formed with its exact rounding error (Dekker's TwoProduct), K
and B are cut column by column into slices of s bits, s = floor((53 - ceil(log2 n)) / 2), so that every product of two
slices summed over the n sites is an exact float64, and the slice products are added in long double (64-bit significand).
"""
import numpy as np
from scipy import linalg

LD = np.longdouble
U = 2.0 ** -53          # unit roundoff of float64
SLICES = 4              # slices per operand: what is dropped is below 2^(-s SLICES) of a column's largest entry


def _split(a):
    """Dekker's split: a = hi + lo exactly, hi and lo of 26 significant bits each."""
    c = 134217729.0 * a  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_product(a, b):
    """p = fl(a b) and its exact rounding error e: a b = p + e (Dekker 1971; no fma needed)."""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _slices(A, s, count):
    """A = S_1 + ... + S_count + rest, S_k an integer of at most s bits times 2^(e_j - s k) in column j (|A[:, j]| <= 2^e_j)."""
    amax = np.abs(A).max(axis=0)
    e = np.ceil(np.log2(np.where(amax > 0, amax, 1.0))).astype(int)
    R = np.array(A, dtype=np.float64)
    out = []
    for k in range(1, count + 1):
        q = np.ldexp(1.0, e - s * k)[None, :]
        S = np.round(R / q) * q      # exact: power-of-two scaling, rounding to the grid of q
        R = R - S                    # exact: |R - S| <= q / 2 on the same grid
        out.append(S)
    return out


def _exact_gemm_tn(A, B):
    """A'B (A: n x a, B: n x b, float64) as a long-double array, error below ~n 2^(-s SLICES) of the columns' largest
    entries' products plus the long-double sum's own rounding."""
    n = A.shape[0]
    s = (53 - int(np.ceil(np.log2(max(n, 2))))) // 2
    SA, SB = _slices(A, s, SLICES), _slices(B, s, SLICES)
    out = np.zeros((A.shape[1], B.shape[1]), dtype=LD)
    terms = [(k, l) for k in range(SLICES) for l in range(SLICES) if k + l < SLICES]
    for k, l in sorted(terms, key=lambda t: -(t[0] + t[1])):    # smallest first
        out += (SA[k].T @ SB[l]).astype(LD)
    return out


def gram_hp(K, omega):
    """K' diag(omega) K in long double.  The slices are scaled per column, so what is dropped is bounded by the columns'
    largest entries: |error_ac| <~ 2^-64 |K|'diag(omega)|K|_ac + n 2^(-s SLICES) max|K[:, a]| max|B[:, c]| (s = 20 at
    n = 4 160: 2^-80 of the maxima).  For bases whose columns are not dominated by a few entries (Moran eigenvectors,
    orthonormal K) that is ~1e-19 of |K|'diag(omega)|K| entry by entry; a column of a few huge and many tiny entries
    can do worse."""
    K = np.ascontiguousarray(K, dtype=np.float64)
    B, Be = _two_product(K, np.asarray(omega, dtype=np.float64)[:, None])
    # K'Be is below 2^-53 of K'B: plain float64 gives it to ~n 2^-106 relative
    return _exact_gemm_tn(K, B) + (K.T @ Be).astype(LD)


def _ld_matvec(A, x, rows=512):
    """A x with A float64 or long double and x long double, products and sums in long double (row blocks: bounded memory)."""
    x = np.asarray(x, dtype=LD)
    out = np.empty(A.shape[0], dtype=LD)
    for i in range(0, A.shape[0], rows):
        out[i:i + rows] = np.asarray(A[i:i + rows], dtype=LD) @ x
    return out


def _ld_tmatvec(A, x, rows=512):
    """A' x in long double."""
    x = np.asarray(x, dtype=LD)
    out = np.zeros(A.shape[1], dtype=LD)
    for i in range(0, A.shape[0], rows):
        out += np.asarray(A[i:i + rows], dtype=LD).T @ x[i:i + rows]
    return out


def b_hp(z, omega, X, beta):
    """b = (z - 1/2) - omega X beta in long double (the sites' part of the right-hand side before the noise)."""
    return (np.asarray(z, dtype=LD) - LD(0.5)) - np.asarray(omega, dtype=LD) * _ld_matvec(X, beta)


def rhs_hp(K, b, omega, eps1, E, eps2, tau):
    """r = K'(b + sqrt(omega) eps1) + sqrt(tau) E eps2 in long double (b may already be long double: :func:`b_hp`)."""
    u = np.asarray(b, dtype=LD) + np.sqrt(np.asarray(omega, dtype=LD)) * np.asarray(eps1, dtype=LD)
    return _ld_tmatvec(K, u) + np.sqrt(LD(tau)) * _ld_matvec(E, eps2)


def lam_hp(K, Qr, omega, tau):
    """Lam = K' diag(omega) K + tau Qr in long double."""
    return gram_hp(K, omega) + LD(tau) * np.asarray(Qr, dtype=LD)


def theta_hp(Lam, r, min_steps=3, max_steps=12):
    """Lam^-1 r in long double: a float64 Cholesky of Lam and iterative refinement with the residual r - Lam theta taken in
    long double (Lam in long double, i.e. its float64 part and the rest).  At least ``min_steps`` corrections; stops once a
    correction is below 1e-3 of the first one (the float64 solve's error) or no longer shrinks (the long-double floor).
    The result is NOT long-double accurate for an ill-conditioned Lam: its relative error is ~kappa 2^-64 at best
    (tests/test_rsr_reference_cpu.py measures 2e-15 at kappa 1e6 and 8e-12 at 1e10), i.e. ~1e-4 of kappa u -- enough
    for bounds of the form c m u kappa, not for anything tighter."""
    Lam = np.asarray(Lam, dtype=LD)
    r = np.asarray(r, dtype=LD)
    cf = linalg.cho_factor(Lam.astype(np.float64), lower=False, check_finite=False)
    th = linalg.cho_solve(cf, r.astype(np.float64), check_finite=False).astype(LD)
    first = prev = None
    for step in range(max_steps):
        d = linalg.cho_solve(cf, (r - _ld_matvec(Lam, th)).astype(np.float64), check_finite=False)
        th = th + d.astype(LD)
        dn = np.linalg.norm(d) / max(np.linalg.norm(th.astype(np.float64)), 1e-300)
        first = dn if first is None else first
        if step + 1 >= min_steps and (dn <= 1e-3 * first or dn >= 0.5 * prev):
            break
        prev = dn
    return th


def kappa(Lam):
    """2-norm condition number of the symmetric positive definite Lam (eigvalsh in float64)."""
    w = linalg.eigvalsh(np.asarray(Lam, dtype=np.float64), check_finite=False)
    return float(w[-1] / w[0])


def numpy_theta(K, Qr, E, b, omega, tau, eps1, eps2):
    """theta as the reference computes it, all in float64: prec = K'(omega K) + tau Qr, then np.linalg.solve."""
    prec = K.T @ (omega[:, None] * K) + tau * Qr
    rhs = K.T @ (np.asarray(b, dtype=np.float64) + np.sqrt(omega) * eps1) + np.sqrt(tau) * (E @ eps2)
    return np.linalg.solve(prec, rhs)


def cholesky_hp(Lam):
    """Upper Cholesky factor U (Lam = U'U) in long double, right-looking, one row per step."""
    A = np.array(Lam, dtype=LD)
    m = A.shape[0]
    Uf = np.zeros_like(A)
    for j in range(m):
        d = np.sqrt(A[j, j])
        Uf[j, j] = d
        row = A[j, j + 1:] / d
        Uf[j, j + 1:] = row
        A[j + 1:, j + 1:] -= np.outer(row, row)
    return Uf


def rel_err(x, ref):
    """||x - ref|| / ||ref|| (2-norms) with the difference taken in long double."""
    ref = np.asarray(ref, dtype=LD)
    return float(np.linalg.norm((np.asarray(x, dtype=LD) - ref).astype(np.float64)) / np.linalg.norm(ref.astype(np.float64)))


def conditioning_matrix(m, spread, rng):
    """M = Q1 diag(logspace(0, -spread)) Q2' with Q1, Q2 random orthogonal: singular values 1 ... 10^-spread."""
    Q1 = np.linalg.qr(rng.standard_normal((m, m)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((m, m)))[0]
    return (Q1 * np.logspace(0.0, -spread, m)) @ Q2.T


def reparam(K, Qr, E, M):
    """The same model in the basis K M: Qr' = M'Qr M, E' = M'E (E'E'' = Qr'), theta' = M^-1 theta.  eta = K theta, the rate
    theta'Qr theta and the law of eta are unchanged; Lam' = M'Lam M, so only kappa(Lam) moves."""
    Qn = M.T @ Qr @ M
    return np.ascontiguousarray(K @ M), np.ascontiguousarray(0.5 * (Qn + Qn.T)), np.ascontiguousarray(M.T @ E)


def spread_for(K, Qr, omega, tau, target, rng):
    """The spread s of :func:`conditioning_matrix` that brings kappa(M'Lam M) near ``target`` for Lam at (omega, tau)
    (kappa grows about as 10^(2 s) times kappa(Lam)); returns (s, M)."""
    Lam = K.T @ (omega[:, None] * K) + tau * Qr
    s = max(0.0, 0.5 * np.log10(target / kappa(Lam)))
    for _ in range(4):
        M = conditioning_matrix(K.shape[1], s, np.random.default_rng(rng.integers(2 ** 32)))
        k = kappa(M.T @ Lam @ M)
        if abs(np.log10(k / target)) < 0.3:
            break
        s = max(0.0, s + 0.5 * np.log10(target / k))
    return s, M
