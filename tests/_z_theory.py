"""The logit z update at a surveyed site without a detection, as a reference in log space (numpy float64): no probability near
1 is formed and nothing is subtracted, so it holds where psi = expit(a0) rounds to 1 and 1 - psi has no digit left.

    a0 = x_i beta + eta_i,   t_r = -w_r alpha,   lsig(t) = log expit(t) = min(t, 0) - log1p(exp(-|t|))
    s = sum_r lsig(t_r)                                   log P, P = prod_r expit(t_r)
    L = a0 + s                                            the logit of pr
    pr = exp(lsig(L)),   q = 1 - pr = exp(lsig(-L))       P(z = 1 | rest) = psi P / ((1 - psi) + psi P)
    l = logaddexp(lsig(-a0), lsig(a0) + s),  D = exp(l)   the site's marginal likelihood D = (1 - psi) + psi P
    b = 1 + |a0| + sum_r (1 + |t_r|)                      the size the bounds are proportional to; where a0 and t_r come
                                                          from dot products, the sums of the |products| stand for |a0|, |t_r|

tests/test_z_theory_cpu.py holds it to mpmath at 50 digits.  The tolerances of every comparison of a kernel (or the oracle)
with it, u = 2^-53 -- derived, not measured:

    pr:  1e-12 b min(pr, q) + 4 u        l:  1e-12 (b + |l|)        D:  the tolerance of l, times D

A dot product differs between host and device by at most 2 (p + 1) u sum |products| (2.2e-15 sum |products| for p <= 9);
that shifts L by as much (a0 directly, s through lsig, whose slope is <= 1) and pr by min(pr, q) times that (d pr / d L =
pr q); an expit costs a few u relative, forty factors 160 u = 1.8e-14, the division and the logarithm a few u more.  So 1e-12
leaves a margin of more than fifty.  No 1 / (1 - psi) appears: a form that subtracts psi from 1 cannot meet them.

Also here: the grid of points the tests share, the two float64 forms of the update (the reference implementation's, which
subtracts, and the device's) restated in numpy, and the terms of a whole problem for the accumulating outputs."""
import numpy as np

U = 2.0 ** -53
A0_GRID = (-700.0, -100.0, -36.75, -20.0, -5.0, 0.0, 5.0, 10.0, 20.0, 25.0, 30.0, 34.0, 36.0, 36.7, 36.8, 37.5, 40.0, 60.0, 100.0,
           300.0, 700.0)
V_GRID = (1, 2, 7, 40)
REPS = 8


def lsig(t):
    """log expit(t), stable on both sides."""
    t = np.asarray(t, dtype=np.float64)
    return np.minimum(t, 0.0) - np.log1p(np.exp(-np.abs(t)))


def reference(a0, s, b):
    """-> dict(pr, q, l, D, b) from a0, s = sum_r lsig(t_r) and b (scalars or arrays of one shape)."""
    a0, s = np.asarray(a0, dtype=np.float64), np.asarray(s, dtype=np.float64)
    L = a0 + s
    l = np.logaddexp(lsig(-a0), lsig(a0) + s)
    return dict(pr=np.exp(lsig(L)), q=np.exp(lsig(-L)), l=l, D=np.exp(l), b=np.asarray(b, dtype=np.float64))


def site(a0, t):
    """The reference at one site: a0 and the site's t_r."""
    t = np.asarray(t, dtype=np.float64)
    return reference(a0, lsig(t).sum(), 1.0 + abs(a0) + np.sum(1.0 + np.abs(t)))


def tol_pr(ref, rel=1e-12, ulps=4.0):
    return rel * ref['b'] * np.minimum(ref['pr'], ref['q']) + ulps * U


def tol_l(ref, rel=1e-12):
    return rel * (ref['b'] + np.abs(ref['l']))


def tol_D(ref):
    return tol_l(ref) * ref['D']


def grid(seed=20):
    """The 21 x 4 x 8 = 672 points (a0, t): a0 of A0_GRID, V of V_GRID rows with -t_r uniform in (-3, 6), REPS repetitions.
    The order is fixed: a0 slowest, the repetition fastest."""
    rng = np.random.default_rng(seed)
    return [(a0, -rng.uniform(-3.0, 6.0, V)) for a0 in A0_GRID for V in V_GRID for _ in range(REPS)]


def _expit_e(t, e):
    return e / (1.0 + e) if t < 0.0 else 1.0 / (1.0 + e)


def _product(t):
    prod = 1.0
    for k, tr in enumerate(np.asarray(t, dtype=np.float64)):             # rows in row order
        ex = _expit_e(tr, np.exp(-abs(tr)))
        prod = ex if k == 0 else prod * ex
    return prod


def subtracting_form(a0, t):
    """(pr, D) as the reference implementation writes them in float64: num / ((1 - psi) + num)."""
    psi = _expit_e(a0, np.exp(-abs(a0)))
    num = psi * _product(t)
    D = (1.0 - psi) + num
    return num / D, D


def device_form(a0, t):
    """(pr, D) by the operations of the device and of the oracle, restated: 1 - psi is 1 - psi for a0 < 0 and exp(-a0) psi
    otherwise (expit_c of csrc/occ_state.hpp), and D is held to 1 (z_den: with P = 1 the rounded sum can be 1 + 2^-52)."""
    e0 = np.exp(-abs(a0))
    psi = _expit_e(a0, e0)
    num = psi * _product(t)
    D = min(((1.0 - psi) if a0 < 0.0 else e0 * psi) + num, 1.0)
    return num / D, D


def misses(pr, D, ref):
    """-> (pr misses its tolerance, l = log D misses its) for one form's (pr, D) at one point."""
    with np.errstate(divide='ignore'):
        l = np.log(D)
    return bool(not abs(pr - ref['pr']) <= tol_pr(ref)), bool(not abs(l - ref['l']) <= tol_l(ref))


def problem_terms(X, eta, beta, W, alpha, ptr, sites):
    """The reference at the entries of a problem: entry k is site ``sites[k]`` with the rows ``ptr[k]:ptr[k + 1]`` of ``W``, taken
    as a site WITHOUT a detection.  -> dict(psi, pr, q, l, D, b, a0, s, P), arrays over the entries; psi = expit(a0) and
    P = exp(s) beside the reference's own.  b is formed from the sums of the |products| of the dot products."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    sites, ptr = np.asarray(sites, dtype=np.int64), np.asarray(ptr, dtype=np.int64)
    a0 = X[sites] @ beta + eta[sites]
    a0_abs = np.abs(X[sites] * beta).sum(axis=1) + np.abs(eta[sites])
    t = -(W @ alpha)
    t_abs = np.abs(W * alpha).sum(axis=1)
    seg = lambda v: np.array([v[ptr[k]:ptr[k + 1]].sum() for k in range(sites.size)])
    s = seg(lsig(t))
    out = reference(a0, s, 1.0 + a0_abs + seg(1.0 + t_abs))
    out.update(psi=np.exp(lsig(a0)), a0=a0, s=s, P=np.exp(s))
    return out


def subtracting_terms(X, eta, beta, W, alpha, ptr, sites):
    """(pr, D) of ``subtracting_form`` at the entries of a problem (``problem_terms``): what a test's inputs are judged by --
    where this form misses the tolerances the inputs have power."""
    X, W = np.asarray(X, dtype=np.float64), np.asarray(W, dtype=np.float64)
    a0 = X[np.asarray(sites)] @ beta + eta[np.asarray(sites)]
    t = -(W @ alpha)
    out = [subtracting_form(a0[k], t[ptr[k]:ptr[k + 1]]) for k in range(len(sites))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])
