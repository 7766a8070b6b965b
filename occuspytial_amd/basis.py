"""The reduced-rank Moran basis without any n x n array: a Chebyshev-filtered block subspace iteration.

``FlatProblem.enable_rsr`` builds the basis ``K`` the reference's way: the dense projector ``P = I - X (X'X)^-1 X'``, the dense
Moran operator ``Omega = n P A P / sum(A)`` (``A = -offdiag(Q)``) and a full ``eigh`` -- O(n^2) memory, O(n^3) time.  Only the
``m << n`` leading eigenpairs are wanted, ``A`` is sparse and ``P`` a rank-p correction, so :func:`moran_basis` iterates on a
block of ``b = m + guard`` columns instead:

    filter          V <- T_d((Omega - c) / e) V, the Chebyshev polynomial that damps [-rho, smallest Ritz value], scaled to
                    1 at (a bound of) the largest eigenvalue
    orthonormalise  CholQR twice: G = V'V, R = chol(G)', V <- V R^-1
    Rayleigh-Ritz   H = V' Omega V, H Y = Y diag(theta), V <- V Y
    residuals       || Omega v_j - theta_j v_j ||

The O(nnz b) and O(n b^2) parts are the ``ops`` object's -- by default a handle of ``libocc_basis.so`` (HIP kernels for
gfx950, ``csrc/occ_basis.hip``) -- the O(b^3) parts (a b x b Cholesky factor and ``scipy.linalg.eigh``) are the host's.

``ops`` is any object with ``rho`` (a bound of ``||Omega||``), ``set_block(V)``, ``get_block()``, ``project()`` (V <- P V),
``filter(degree, lo, hi, top)``, ``gram(which)`` (``V'V`` for 0, ``V' Omega V`` for 1), ``rotate(Y)`` (V <- V Y) and
``residual(theta)``; ``tests/test_basis_cpu.py`` runs the driver against one made of numpy matrix products.
"""
import math
import time

import numpy as np
from scipy.linalg import cholesky, eigh, solve_triangular

GUARD = 32              # extra columns of the block beyond the wanted ones (at least; b is then rounded up to 16)
SEED = 0x6d6f72616e     # of the starting block: the result is a function of (Q, X, r, q) alone
AMPLIFICATION = 1e6     # a filter may stretch the block's condition number to this (CholQR twice needs it below 1 / sqrt(eps))
MAX_START_BLOCK = 1024  # threshold mode: the first block is n / 16 + GUARD columns, at most this many
MAX_BASIS = 4096        # what the samplers take (gibbs/logit.py, gibbs/probit.py); a block never grows past this plus two guards
MAX_BLOCK = 4096 + 2 * GUARD


def _too_many(count):
    # (the samplers' own text; Ritz values >= r never outnumber eigenvalues >= r, so `count` is a lower bound)
    return ValueError(f'{count} basis columns selected; the device path supports at most {MAX_BASIS} '
                      '(raise the threshold `r` or pass `q`)')


def _round16(v):
    return (int(v) + 15) // 16 * 16


class _Clock:
    def __init__(self):
        self.ops = self.dense = 0.0
        self.applies = 0


def _timed(clock, field, fn, *args):
    t0 = time.perf_counter()
    out = fn(*args)
    setattr(clock, field, getattr(clock, field) + time.perf_counter() - t0)
    return out


def _orthonormalise(ops, clock):
    """CholQR twice (a third pass when the first factorisation needed a shift)."""
    passes, done = 2, 0
    while done < passes:
        G = _timed(clock, 'ops', ops.gram, 0)
        t0 = time.perf_counter()
        try:
            R = cholesky(G, lower=False)
        except np.linalg.LinAlgError:
            # shifted CholQR: the block's condition number is beyond 1 / sqrt(eps); one more pass restores orthogonality
            b = G.shape[0]
            shift = 100.0 * b * np.finfo(float).eps * np.abs(np.diag(G)).max()
            try:
                R = cholesky(G + shift * np.eye(b), lower=False)
            except np.linalg.LinAlgError:
                raise RuntimeError('moran_basis: the block lost rank (its Gram matrix is not positive definite)') from None
            passes = min(passes + 1, 4)
        Rinv = solve_triangular(R, np.eye(R.shape[0]), lower=False)
        clock.dense += time.perf_counter() - t0
        _timed(clock, 'ops', ops.rotate, Rinv)
        done += 1


def _ritz(ops, clock):
    H = _timed(clock, 'ops', ops.gram, 1)
    theta, Y = _timed(clock, 'dense', eigh, H)
    _timed(clock, 'ops', ops.rotate, np.ascontiguousarray(Y))
    return theta


def _degree(degree, lo, hi, top):
    """The largest degree <= ``degree`` whose polynomial grows by at most AMPLIFICATION between ``hi`` and ``top``."""
    c, e = 0.5 * (lo + hi), 0.5 * (hi - lo)
    x = max((top - c) / e, 1.0 + 1e-12)
    return int(min(degree, max(1, math.floor(math.acosh(AMPLIFICATION) / math.acosh(x)))))


def moran_basis(Q, X, r=0.5, q=None, *, ops=None, tol=1e-9, degree=200, max_outer=100, device=0, return_info=False):
    """The ``m`` leading eigenvectors of the Moran operator ``Omega = n P A P / sum(A)``, as an ``n x m`` array whose columns
    are ordered by ascending eigenvalue (what ``np.linalg.eigh(Omega)[1][:, -m:]`` is in ``enable_rsr``).  ``q`` fixes ``m``;
    otherwise ``m`` is the number of eigenvalues ``>= r``.

    The columns are orthonormal and orthogonal to ``X``.  They are defined up to sign, and up to a rotation inside a cluster of
    near-equal eigenvalues; the model depends on ``span(K)`` alone, and that is what converges: the iteration stops when the
    kept columns' residuals ``||Omega k - theta k||`` have a root sum of squares ``<= tol * rho`` (so each of them is, and so
    is ``||Omega K - K diag(theta)||``, which Davis-Kahan's bound asks for; ``rho >= ||Omega||`` is Gershgorin's bound) and raises
    ``RuntimeError`` after ``max_outer`` rounds -- an unconverged basis is never returned.  ``degree`` bounds the filter's
    degree (it is lowered where the polynomial would stretch the block's condition number beyond 1e6).

    The same inputs give the same bits: the starting block comes from a fixed seed and no kernel's sums depend on scheduling.
    With ``return_info`` the result is ``(K, info)``: eigenvalues, residuals, rho, outer rounds, Omega applications and the
    seconds spent in ``ops`` and in the host's b x b factorisations.
    """
    t_start = time.perf_counter()
    X = np.ascontiguousarray(X, dtype=np.float64)
    n, p = X.shape
    fixed = bool(q)
    if fixed:
        m = int(q)
        if m < 1 or m > n - p:
            raise ValueError(f"q must lie in [1, n - p] = [1, {n - p}] for basis='device'")
        if m > MAX_BASIS:
            raise _too_many(m)
        b = min(_round16(m + GUARD), n - p)
    else:
        if not 0 <= r <= 1:
            raise ValueError('Threshold value needs to be in [0, 1]')
        m = 0
        b = min(_round16(min(n // 16 + GUARD, MAX_START_BLOCK)), n - p)
    own = ops is None
    if own:
        from ._basis_lib import DeviceBasisOps
        ops = DeviceBasisOps(Q, X, b if fixed else min(n - p, 4 * b, MAX_BLOCK), device=device)
    clock = _Clock()
    rng = np.random.Generator(np.random.PCG64(SEED))
    try:
        rho = float(ops.rho)
        goal = tol * rho
        ops.set_block(rng.standard_normal((n, b)))
        _timed(clock, 'ops', ops.project)
        _orthonormalise(ops, clock)
        theta = _ritz(ops, clock)
        res = np.full(b, np.inf)
        for outer in range(1, int(max_outer) + 1):
            # where the polynomial is 1: rho at first, then just above the largest Ritz value (which converges first)
            top = min(rho, theta[-1] + max(res[-1], 1e-3 * rho))
            d = _degree(degree, -rho, theta[0], top)
            _timed(clock, 'ops', ops.filter, d, -rho, theta[0], top)
            clock.applies += d
            _orthonormalise(ops, clock)
            theta = _ritz(ops, clock)
            res = _timed(clock, 'ops', ops.residual, theta)
            clock.applies += 1
            if fixed:
                if np.linalg.norm(res[-m:]) <= goal:
                    break
                continue
            # threshold mode (ascending theta): the columns before `keep` are the guard
            keep = b - min(GUARD, b // 2)
            count = int((theta >= r).sum())
            if count < b and np.linalg.norm(res[b - count - 1:]) <= goal:
                m = count   # every eigenvalue >= r has converged, and so has the first one below r
                break
            if count > MAX_BASIS:
                raise _too_many(count)
            first = b - keep  # the smallest Ritz value outside the guard
            if b < min(n - p, MAX_BLOCK) and (count == b or theta[first] - res[first] >= r):
                # the block does not reach down to r yet: half as many columns again, random, projected, orthogonalised
                b_new = min(_round16(b + b // 2), n - p, MAX_BLOCK)
                V = ops.get_block()
                V = np.concatenate([rng.standard_normal((n, b_new - b)), V], axis=1)
                if own and b_new > ops.b_max:
                    ops.close()
                    ops = DeviceBasisOps(Q, X, min(n - p, 2 * b_new, MAX_BLOCK), device=device)
                ops.set_block(V)
                del V
                b = b_new
                _timed(clock, 'ops', ops.project)
                _orthonormalise(ops, clock)
                theta = _ritz(ops, clock)
                res = np.full(b, np.inf)   # (of the grown block: not known until the next round)
        else:
            worst = float(np.linalg.norm(res[-m:] if fixed else res[b - min(b, int((theta >= r).sum()) + 1):]))
            raise RuntimeError(f'moran_basis did not converge in {int(max_outer)} outer iterations: residual {worst:.3e}, '
                               f'needed {goal:.3e} (tol * rho); raise max_outer or degree')
        if not m:
            raise ValueError('The Moran Operator Matrix of the data has no positive '
                             'eigenvalues. Set threshold to a lower value')
        K = np.ascontiguousarray(ops.get_block()[:, b - m:])
    finally:
        if own:
            ops.close()
    if not return_info:
        return K
    info = {'eigenvalues': theta[b - m:].copy(), 'residuals': res[b - m:].copy(), 'rho': rho, 'outer': outer, 'block': b,
            'applies': clock.applies, 'seconds_ops': clock.ops, 'seconds_dense': clock.dense,
            'seconds': time.perf_counter() - t_start}
    return K, info
