"""Streaming WAIC, the parts that need no device: ``WAIC`` and ``compare`` against direct numpy, the state names in header
and binding, and the refusals (probit model, Python ``step``, a library without the feature)."""
import os
import re

import numpy as np
import pytest
from scipy.special import logsumexp

from .conftest import ROOT, load_golden
from .test_api_cpu import _inputs
from .test_cpu_abi import cpu_abi  # noqa: F401  (the oracle's build of the C ABI, which does not know the ll_* names)

LL_NAMES = ('ll_stats', 'll_count', 'll_lik', 'll_log', 'll_log2')
SITE_NAMES = ('site_stats', 'site_count', 'site_psi', 'site_occ', 'site_z', 'site_eta', 'site_eta2')


def _histories(seed, n=57, lengths=(120, 333, 400), shift=0.0):
    """Per chain a history l[t, i] = m_i + s_i * noise with m_i in [-6, -0.5] and s_i in [0.3, 0.8], and its sums; every
    third site is not surveyed (its sums are 0, as the engine leaves them).  -> (site_id, histories, counts, sums)."""
    rng = np.random.default_rng(seed)
    site_id = np.array([i for i in range(n) if i % 3 != 1])
    m = rng.uniform(-6.0, -0.5, size=n) + shift
    s = rng.uniform(0.3, 0.8, size=n)
    hist, counts, sums = [], [], []
    for c, T in enumerate(lengths):
        ll = m + 0.2 * c + s * rng.standard_normal((T, n))     # (chains that disagree: pooling is then not a mean of chains)
        full = {k: np.zeros(n) for k in ('lik', 'log', 'log2')}
        full['lik'][site_id] = np.exp(ll[:, site_id]).sum(0)
        full['log'][site_id] = ll[:, site_id].sum(0)
        full['log2'][site_id] = (ll[:, site_id] ** 2).sum(0)
        hist.append(ll[:, site_id])
        counts.append(T)
        sums.append(full)
    return site_id, hist, counts, sums


def test_waic_equals_direct_numpy_on_synthetic_histories():
    """3 chains of 120, 333 and 400 draws (N = 853), 57 sites of which 38 are surveyed.  Tolerances, from the formats:

      lppd_i   1e-12 absolute.  sum L carries a relative error of at most N 2^-53 = 9.5e-14, which is the absolute error of its
               logarithm; logsumexp's own rounding is a few ulp of |lppd_i| <= 8, 4e-15.
      p_waic_i 1e-10 relative.  The variance from plain sums has a relative error of about N 2^-53 (1 + mean^2 / var).  The
               histories have |mean| <= 6.5 (m_i in [-6, -0.5], a chain offset of at most 0.4, a sampling error of the mean far
               below 0.1) and a pooled sd >= 0.27 (s_i >= 0.3, and a sample sd of 853 draws is within 10 % of it): the ratio is at
               most 6.5^2 / 0.27^2 = 580, so 9.5e-14 * 581 = 5.5e-11.  Both premises are asserted.
      elpd, lppd, p_waic, waic
               S times the pointwise bounds with p_waic_i <= 1.1 (s_i <= 0.8 plus the chains' offsets: asserted):
               38 * (1e-12 + 1.1e-10) = 4.3e-9, twice that for waic.
      se       2e-9 absolute: se = 2 sqrt(S / (S - 1)) ||e - mean(e)||, so a perturbation d of the elpd_i moves it by at most
               2 sqrt(S / (S - 1)) ||d|| <= 2 * 1.02 * sqrt(38) * 1.11e-10 = 1.4e-9."""
    from occuspytial_amd.waic import WAIC
    site_id, hist, counts, sums = _histories(42)
    w = WAIC(counts, sums, site_id)
    cat = np.concatenate(hist)
    N, S = cat.shape
    assert N == 853 and S == 38 and w.n_draws.tolist() == [120, 333, 400] and w.n_sites == S
    assert np.array_equal(w.site_id, site_id)
    mean, var = cat.mean(0), cat.var(0, ddof=1)
    assert np.abs(mean).max() <= 6.5 and np.sqrt(var).min() >= 0.27 and var.max() <= 1.1    # the premises of the bounds
    lppd_i = logsumexp(cat, axis=0) - np.log(N)
    fig = dict(lppd=np.abs(w.lppd_i - lppd_i).max(), p_waic=np.max(np.abs(w.p_waic_i - var) / var))
    print('WAIC against numpy:', fig)
    assert fig['lppd'] <= 1e-12
    assert fig['p_waic'] <= 1e-10
    elpd_i = lppd_i - var
    assert np.abs(w.elpd_i - elpd_i).max() <= 1e-12 + 1.1e-10
    assert abs(w.lppd - lppd_i.sum()) <= 38e-12
    assert abs(w.p_waic - var.sum()) <= 38 * 1.1e-10
    assert abs(w.elpd - elpd_i.sum()) <= 4.3e-9
    assert abs(w.waic + 2.0 * elpd_i.sum()) <= 8.6e-9
    assert w.waic == -2.0 * w.elpd
    assert abs(w.se - 2.0 * np.sqrt(S * np.var(elpd_i, ddof=1))) <= 2e-9
    assert w.n_high_var == int(np.count_nonzero(var > 0.4)) and 0 < w.n_high_var < S
    # pooling is the merge of the sums (chains weigh by their draws), not a mean of per-chain values
    per_chain = [WAIC([counts[c]], [sums[c]], site_id) for c in range(3)]
    mean_of_chains = np.mean([p.elpd_i for p in per_chain], axis=0)
    assert not np.allclose(w.elpd_i, mean_of_chains, rtol=1e-6, atol=0)
    for c, p in enumerate(per_chain):
        assert np.abs(p.lppd_i - (logsumexp(hist[c], axis=0) - np.log(counts[c]))).max() <= 1e-12
    with pytest.raises(ValueError):
        WAIC([3, 4], sums, site_id)
    with pytest.raises(ValueError):
        WAIC(counts, sums, [0, 57])


def test_waic_reports_a_negative_rounding_variance_as_zero_and_an_underflow_as_minus_infinity():
    from occuspytial_amd.waic import WAIC
    # a constant history: the variance is 0 up to rounding, which may fall on either side
    ll = np.full(7, -1.0 / 3.0)
    sums = dict(lik=np.exp(ll).sum() * np.ones(2), log=ll.sum() * np.ones(2), log2=np.array([(ll * ll).sum() * (1 - 1e-15), (ll * ll).sum()]))
    w = WAIC([7], [sums], [0, 1])
    assert w.p_waic_i[0] == 0.0 and w.p_waic_i[1] >= 0.0
    under = dict(lik=np.zeros(1), log=np.array([-800.0 * 5]), log2=np.array([800.0 ** 2 * 5]))
    w = WAIC([5], [under], [0])
    assert w.lppd_i[0] == -np.inf and w.elpd == -np.inf


def test_compare_has_a_known_answer_and_refuses_different_sites():
    """Two sets of sums built so that every pointwise value is exact: per site two draws l = a -+ d give sum l = 2 a,
    sum l^2 = 2 a^2 + 2 d^2 and a variance (ddof = 1) of 2 d^2; L is set to make lppd_i = log(lik / 2) a chosen number."""
    from occuspytial_amd.waic import WAIC, compare

    def build(lppd_i, d):
        lppd_i, d = np.asarray(lppd_i, dtype=float), np.asarray(d, dtype=float)
        a = -np.ones_like(d)
        full = dict(lik=2.0 * np.exp(lppd_i), log=2.0 * a, log2=2.0 * a * a + 2.0 * d * d)
        return WAIC([2], [full], np.arange(d.size))

    A = build([-1.0, -2.0, -0.5, -1.5], [0.5, 0.0, 0.25, 0.5])       # p_waic_i = 0.5, 0, 0.125, 0.5
    B = build([-1.5, -2.0, -1.5, -2.5], [0.5, 0.5, 0.25, 0.0])       # p_waic_i = 0.5, 0.5, 0.125, 0
    ea = np.array([-1.5, -2.0, -0.625, -2.0])
    eb = np.array([-2.0, -2.5, -1.625, -2.5])
    assert np.abs(A.elpd_i - ea).max() <= 1e-15 and np.abs(B.elpd_i - eb).max() <= 1e-15
    out = compare(A, B)
    d = ea - eb                                                     # 0.5, 0.5, 1.0, 0.5
    assert abs(out['elpd_diff'] - 2.5) <= 1e-14
    assert abs(out['se_diff'] - np.sqrt(4 * np.var(d, ddof=1))) <= 1e-14 and abs(out['se_diff'] - 0.5) <= 1e-14
    back = compare(B, A)
    assert back['elpd_diff'] == -out['elpd_diff'] and back['se_diff'] == out['se_diff']
    C = WAIC([2], [dict(lik=np.ones(5), log=-np.ones(5), log2=np.ones(5))], [0, 1, 2, 4])
    with pytest.raises(ValueError, match='different sites'):
        compare(A, C)
    with pytest.raises(ValueError, match='different sites'):
        compare(A, WAIC([2], [dict(lik=np.ones(5), log=-np.ones(5), log2=np.ones(5))], [0, 1, 2]))


def test_every_loglik_state_name_is_in_header_and_binding():
    from occuspytial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    comments = ' '.join(re.findall(r'/\*.*?\*/', header, flags=re.S))
    documented = set(re.findall(r'\b(ll_[a-z0-9]+)\b', comments))
    assert set(LL_NAMES) == documented, set(LL_NAMES) ^ documented
    assert tuple(_lib.LOGLIK_FIELDS) == LL_NAMES
    assert not any(name.startswith('site_') for name in _lib.LOGLIK_FIELDS)
    assert set(_lib.SITE_FIELDS) == set(SITE_NAMES)                 # unchanged
    assert re.search(r'#define OCC_ABI_VERSION 7\b', header) and _lib.ABI_VERSION == 7   # no layout change came with them


def test_probit_and_python_step_samplers_refuse_waic(monkeypatch):
    """Both raise before any engine exists: creating one here would need a device."""
    from occuspytial_amd import ProbitRSRGibbs, _engine
    from occuspytial_amd.gibbs.base import GibbsBase

    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(_engine.Engine, '__init__', no_engine)
    Q, W, X, y = _inputs(load_golden('ref_queen150_ragged'))[:4]
    with pytest.raises(NotImplementedError, match='probit'):
        ProbitRSRGibbs(Q, W, X, y, random_state=1, q=10).sample(5, waic=True)

    class PyStep(GibbsBase):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._configure(a[0], None)

        def step(self):
            raise AssertionError('step was called')

    with pytest.raises(NotImplementedError, match='Python'):
        PyStep(Q, W, X, y, random_state=1).sample(5, waic=True)


def test_a_library_without_the_feature_is_refused_and_the_default_asks_nothing(cpu_abi, monkeypatch):  # noqa: F811
    """Every occ_get_state / occ_set_state call goes through a counting wrapper: with the default none names ll_*."""
    from occuspytial_amd import LogitICARGibbs
    asked = []

    def counting(fn):
        def call(handle, chain, name, *rest):
            asked.append(name.decode())
            return fn(handle, chain, name, *rest)
        return call
    monkeypatch.setattr(cpu_abi, 'occ_get_state', counting(cpu_abi.occ_get_state))
    monkeypatch.setattr(cpu_abi, 'occ_set_state', counting(cpu_abi.occ_set_state))
    Q, W, X, y = _inputs(load_golden('ref_queen150_ragged'))[:4]
    out = LogitICARGibbs(Q, W, X, y, random_state=3).sample(5, chains=1, progressbar=False)
    assert out.waic is None and out['alpha'].shape[:2] == (1, 5)
    assert asked and not [name for name in asked if name.startswith('ll_')]     # (the wrapper saw the run's other calls)
    with pytest.raises(ValueError, match=r'no log-likelihood sums .*rebuild it'):
        LogitICARGibbs(Q, W, X, y, random_state=3).sample(5, chains=1, progressbar=False, waic=True)
    assert [name for name in asked if name.startswith('ll_')] == ['ll_stats']
