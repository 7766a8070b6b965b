"""Known-answer and distributional tests of the oracle's variate generators.

PG(1, z) is NOT pinned by the reference (third-party `polyagamma`, absent): closed-form moments and
Laplace transform of the Polya-Gamma law (Polson, Scott & Windle 2013) stand in for golden vectors.
"""
import math

import numpy as np
import pytest
from scipy import stats

from ._pg_theory import PG_OVERFLOW, PG_SUBNORMAL, pg_cdf, pg_laplace, pg_mean, pg_var


def test_philox_known_answers(oracle):
    # Random123 kat_vectors, philox4x32 10 rounds
    kat = [
        ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
        ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
        ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
         (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ]
    for ctr, key, want in kat:
        assert tuple(int(v) for v in oracle.philox(ctr, key)) == want


def test_u01_open_interval(oracle):
    L = oracle.lib()
    assert 0.0 < L.orc_u01(0) < 1e-15
    assert 1.0 - 1e-15 < L.orc_u01(2**64 - 1) < 1.0


@pytest.mark.parametrize('z', [0.0, 0.3, 1.0, 1.5, 1.5625, 2.5, 5.0, 12.0, -3.0, 40.0, 3.125, 98.0, 300.0, 1e4])
def test_pg1_moments_and_laplace(oracle, z):
    """98, 300, 1e4: past |z| = 96.83, where the right piece's mass has an infinite denominator -- the oracle, a correct
    sampler there, is what the device is held to draw by draw (tests/test_gpu_rng.py)."""
    N = 200_000
    x = oracle.pg1(np.full(N, z), key=99 + int(abs(z) * 16), it=3)
    assert np.all(x > 0)
    m, v = pg_mean(z), pg_var(z)
    assert abs(x.mean() - m) < 5 * np.sqrt(v / N)
    assert abs(x.var() - v) < 0.03 * v
    for t in (0.5, 2.0, 10.0):
        lt = pg_laplace(z, t)
        e = np.exp(-t * x)
        assert abs(e.mean() - lt) < 5 * e.std() / np.sqrt(N)


@pytest.mark.parametrize('z', [0.0, 3.125, 98.0, 300.0, 1e4])
def test_pg1_ks_against_the_exact_cdf(oracle, z):
    x = oracle.pg1(np.full(200_000, z), key=31 + int(z), it=2)
    assert stats.kstest(x, lambda v: pg_cdf(v, z)).pvalue > 1e-3


def _pg_density_mp(mp, x, z):
    """PG(1, z) density (Polson, Scott & Windle 2013, eq. for PG(1, 0) exponentially tilted), at mpmath precision: the
    small-x form of the alternating series below x = 1, its Poisson-summed large-x form above."""
    x, b = mp.mpf(x), abs(mp.mpf(z))
    if x < 1:
        s = mp.nsum(lambda n: (-1) ** n * (2 * n + 1) * mp.exp(-(2 * n + 1) ** 2 / (8 * x)), [0, mp.inf]) / mp.sqrt(2 * mp.pi * x ** 3)
    else:
        s = 4 * mp.nsum(lambda n: (-1) ** n * mp.pi * (n + 0.5) * mp.exp(-2 * (n + 0.5) ** 2 * mp.pi ** 2 * x), [0, mp.inf])
    return mp.cosh(b / 2) * mp.exp(-b * b * x / 2) * s


def test_pg_theory_forms_against_high_precision():
    """tests/_pg_theory.py against mpmath: the CDF's image series against quadrature of the density, the mean, variance and
    Laplace transform against their defining formulas at 40 digits -- on both sides of each form's switch to a series and
    far past the range where the textbook forms overflow (cosh(z/2) at |z| ~ 1420, sinh z at ~ 710)."""
    import mpmath as mp
    mp.mp.dps = 40
    for z in (0.0, 1e-300, 1e-6, 9e-3, 1.1e-2, 0.049, 0.051, 0.7, 3.125, 50.0, 98.0, 700.0, 1500.0, 1e4, 1e6, 1e99):
        b = mp.mpf(z)
        with mp.workdps(40 + (3 * int(-math.log10(z)) if 0 < z < 1 else 0)):   # (the numerator cancels to O(z^3))
            mean = mp.mpf(1) / 4 if z == 0 else mp.tanh(b / 2) / (2 * b)
            var = mp.mpf(1) / 24 if z == 0 else (2 * mp.tanh(b / 2) - b * mp.sech(b / 2) ** 2) / (4 * b ** 3)
        assert abs(pg_mean(z) / mean - 1) < 1e-14 and abs(pg_mean(-z) / mean - 1) < 1e-14, z
        assert abs(pg_var(z) / var - 1) < 1e-12 and abs(pg_var(-z) / var - 1) < 1e-12, z
        for t in (0.5, 10.0):
            lt = mp.cosh(b / 2) / mp.cosh(mp.sqrt((b * b / 2 + t) / 2))
            assert abs(pg_laplace(z, t) / lt - 1) < 1e-13, (z, t)
    for z in (0.0, 2.0, 50.0, 1e3):
        m, sd = pg_mean(z), math.sqrt(pg_var(z))
        for k in (-1.5, 0.0, 2.0):
            x = m + k * sd
            pts = sorted({0.0, x} | {p for p in (m - 6 * sd, m - 3 * sd, m - sd, m) if 0.0 < p < x})
            ref = mp.quad(lambda u: _pg_density_mp(mp, u, z), pts)
            assert abs(pg_cdf(x, z) - ref) < 1e-13, (z, x, float(ref))
    assert pg_cdf(0.0, 1.0) == 0.0 and pg_cdf(-1.0, 1.0) == 0.0 and abs(pg_cdf(50.0, 0.0) - 1.0) < 1e-15


def _pg_tail_denominator(z):
    """1 + k f exp(f t - Z) of the oracle's (and the device's) pg1_draw for Z = |z| / 2 >= 1 / t, in the same order"""
    Z = 0.5 * abs(z)
    fz = 0.125 * math.pi * math.pi + 0.5 * Z * Z
    ex = fz * 0.64 - Z
    return math.inf if ex > 709.79 else 1.0 + 1.2732395447351628 * fz * math.exp(ex)


def test_pg_thresholds_are_where_the_proposal_mass_overflows():
    """The constants the device tests place arguments around (tests/_pg_theory.py): from |z| = 96.831... on the
    denominator of the right piece's mass is infinite, from 96.738... on it is at least 2^1022 (reciprocal subnormal)."""
    below = np.nextafter(PG_OVERFLOW, 0.0)
    assert math.isinf(_pg_tail_denominator(PG_OVERFLOW)) and math.isfinite(_pg_tail_denominator(below))
    assert _pg_tail_denominator(PG_SUBNORMAL) >= 2.0 ** 1022 > _pg_tail_denominator(np.nextafter(PG_SUBNORMAL, 0.0))


def test_pg1_ks_against_truncated_series(oracle):
    rng = np.random.default_rng(0)
    for z in (0.0, 2.0):
        x = oracle.pg1(np.full(20000, z), key=5, it=1)
        k = np.arange(1, 401) - 0.5
        g = rng.standard_exponential((20000, 400))
        ref = (g / (k ** 2 + (z / (2 * np.pi)) ** 2)).sum(axis=1) / (2 * np.pi ** 2)
        assert stats.ks_2samp(x, ref).pvalue > 1e-3


def test_pg1_substreams_are_independent_of_array_position(oracle):
    z = np.linspace(-4, 4, 64)
    a = oracle.pg1(z, key=7, it=2)
    b = oracle.pg1(z[::-1].copy(), key=7, it=2)
    assert not np.array_equal(a, b[::-1])        # draw depends on (index, z)
    assert np.array_equal(a, oracle.pg1(z, key=7, it=2))  # and is reproducible


@pytest.mark.parametrize('shape', [0.3, 1.0, 5.0, 75.0, 5000.0])
def test_std_gamma_distribution(oracle, shape):
    x = np.array([oracle.std_gamma(shape, key=11, it=i) for i in range(20000)])
    assert stats.kstest(x, 'gamma', args=(shape,)).pvalue > 1e-3


def test_block_normal_distribution(oracle):
    L = oracle.lib()
    x = np.array([L.orc_block_normal(3, i, 0, 0, 3) for i in range(50000)])
    assert stats.kstest(x, 'norm').pvalue > 1e-3
    u = np.array([L.orc_block_uniform(3, i, 0, 0, 8) for i in range(50000)])
    assert stats.kstest(u, 'uniform').pvalue > 1e-3
