"""The reference of the z update (tests/_z_theory.py) against mpmath at 50 digits; the power of its grid against the form that
subtracts psi from 1; and the oracle's orc_z_prob against it.  The tolerances are those of _z_theory's docstring."""
import numpy as np
import pytest

from . import _z_theory as zt


@pytest.fixture(scope='module')
def points():
    """The grid with the reference at every point: computed once, never changed."""
    return [(a0, t, zt.site(a0, t)) for a0, t in zt.grid()]


def _exact(a0, t):
    """(pr, l) to 50 digits."""
    mp = pytest.importorskip('mpmath')
    mp.mp.dps = 50
    a = mp.mpf(float(a0))
    psi = 1 / (1 + mp.exp(-a))
    P = mp.mpf(1)
    for tr in t:
        P *= 1 / (1 + mp.exp(-mp.mpf(float(tr))))
    D = 1 / (1 + mp.exp(a)) + psi * P
    return psi * P / D, mp.log(D)


def test_the_reference_equals_mpmath_at_50_digits(points):
    """|pr - exact| <= 1e-13 b min(pr, q) + 2^-52 and |l - exact| <= 1e-14 (1 + |l|) at every point whose exact pr is at least
    1e-300 (a0 = -700 falls out: 640 of the 672 points are left)."""
    mp = pytest.importorskip('mpmath')
    kept, worst_pr, worst_l, worst_gpu = 0, 0.0, 0.0, 0.0
    for a0, t, ref in points:
        pr, l = _exact(a0, t)
        if pr < mp.mpf('1e-300'):
            continue
        kept += 1
        d_pr, d_l = float(abs(mp.mpf(float(ref['pr'])) - pr)), float(abs(mp.mpf(float(ref['l'])) - l))
        d_q = float(abs(mp.mpf(float(ref['q'])) - (1 - pr)))
        worst_pr = max(worst_pr, d_pr / float(zt.tol_pr(ref, 1e-13, 2.0)))
        worst_l = max(worst_l, d_l / (1.0 + abs(float(l))))
        worst_gpu = max(worst_gpu, d_pr / float(zt.tol_pr(ref)))
        assert d_pr <= zt.tol_pr(ref, 1e-13, 2.0), (a0, t.size, float(pr), d_pr)
        assert d_q <= zt.tol_pr(ref, 1e-13, 2.0), (a0, t.size, float(pr), d_q)
        assert d_l <= 1e-14 * (1.0 + abs(float(l))), (a0, t.size, float(l), d_l)
    print('reference against mpmath: %d points, pr worst found / bound %.3g (%.3g of the tolerance held against it), l worst %.3g (1 + |l|)'
          % (kept, worst_pr, worst_gpu, worst_l))
    assert kept == 640


def _kept(points):
    return [(a0, t, ref) for a0, t, ref in points if a0 != -700.0]


def test_the_grid_has_power_against_the_subtraction(points):
    """The form num / ((1 - psi) + num) in float64 misses the tolerance of pr at 20 % of the points or more and that of l at
    15 % or more; the device's form, restated in numpy, misses neither anywhere."""
    pts = _kept(points)
    old = np.array([zt.misses(*zt.subtracting_form(a0, t), ref) for a0, t, ref in pts])
    new = np.array([zt.misses(*zt.device_form(a0, t), ref) for a0, t, ref in pts])
    worst = max(max(abs(pr - ref['pr']) / zt.tol_pr(ref), abs(np.log(D) - ref['l']) / zt.tol_l(ref))
                for (a0, t, ref) in pts for pr, D in [zt.device_form(a0, t)])
    print('the subtracting form misses pr at %d and l at %d of %d points; the device form: worst found / bound %.3g'
          % (old[:, 0].sum(), old[:, 1].sum(), len(pts), worst))
    assert len(pts) == 640
    assert old[:, 0].sum() >= 0.20 * len(pts)
    assert old[:, 1].sum() >= 0.15 * len(pts)
    assert not new.any()


def test_a_likelihood_never_exceeds_one_where_the_product_is_one(oracle):
    """t_r = 800: expit(t_r) = 1 and P = 1, so D = (1 - psi) + psi = 1 and pr = psi.  The rounded exp(-a0) psi + psi exceeds 1
    by 2^-52 at about a tenth of the a0 in (0, 40) (the first assertion: the inputs find it); the device's form, restated, gives
    D <= 1 and pr <= 1 at every one, and the oracle's probability is psi to two ulp."""
    a0 = np.linspace(0.0, 40.0, 4001)
    e0 = np.exp(-a0)
    psi = 1.0 / (1.0 + e0)
    assert np.count_nonzero(e0 * psi + psi > 1.0) >= 100
    t = np.array([800.0, 800.0])
    beta, alpha, W = np.array([0.0, 1.0]), np.array([0.0, 1.0]), np.column_stack([np.ones(2), -t])
    for a, ps in zip(a0, psi):
        pr, D = zt.device_form(a, t)
        assert D <= 1.0 and pr <= 1.0 and abs(D - 1.0) <= 2.0 * zt.U and abs(pr - ps) <= 4.0 * zt.U, (a, pr, D)
        assert abs(oracle.z_prob(np.array([1.0, a]), beta, 0.0, W, alpha) - ps) <= 4.0 * zt.U, a


def test_the_oracles_z_probability_equals_the_reference(oracle, points):
    """orc_z_prob at every point of the grid, with the inputs exact: X = [1, a0], beta = (0, 1), eta = 0; W = [1, -t_r],
    alpha = (0, 1)."""
    beta, alpha = np.array([0.0, 1.0]), np.array([0.0, 1.0])
    worst = 0.0
    for a0, t, ref in points:
        W = np.column_stack([np.ones(t.size), -t])
        pr = oracle.z_prob(np.array([1.0, a0]), beta, 0.0, W, alpha)
        worst = max(worst, abs(pr - ref['pr']) / zt.tol_pr(ref))
        assert abs(pr - ref['pr']) <= zt.tol_pr(ref), (a0, t.size, pr, float(ref['pr']))
    print('orc_z_prob against the reference: worst found / bound %.3g' % worst)
