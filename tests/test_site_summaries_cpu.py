"""Per-site posterior summaries, the parts that need no device: ``SiteSummary`` against direct numpy, the state names in
header and binding, and the refusals (probit model, Python ``step``, a library without the feature)."""
import os
import re

import numpy as np
import pytest

from .conftest import ROOT, load_golden
from .test_api_cpu import _inputs
from .test_cpu_abi import cpu_abi  # noqa: F401  (the oracle's build of the C ABI, which does not know site summaries)

SITE_NAMES = ('site_stats', 'site_count', 'site_psi', 'site_occ', 'site_z', 'site_eta', 'site_eta2')


def test_site_summary_equals_direct_numpy_on_synthetic_histories():
    """3 chains of different lengths: pooled means and eta_sd equal np.mean / np.std(ddof=1) of the concatenated
    histories to 1e-12 relative (float64 sums of <= 10^3 terms of size O(1): 10^3 * 2^-53 ~ 1e-13, ten-fold margin)."""
    from occuspytial_amd.sites import SiteSummary
    rng = np.random.default_rng(42)
    n, lengths = 57, (120, 333, 400)
    hist, counts, sums = [], [], []
    for L in lengths:
        eta = 0.7 * rng.standard_normal((L, n)) + rng.standard_normal(n)
        psi = 1.0 / (1.0 + np.exp(-eta))
        occ = np.clip(psi * rng.uniform(0.5, 1.5, size=(L, n)), 0.0, 1.0)
        z = (rng.uniform(size=(L, n)) < occ).astype(float)
        hist.append(dict(psi=psi, occ=occ, z=z, eta=eta))
        counts.append(L)
        sums.append(dict(psi=psi.sum(0), occ=occ.sum(0), z=z.sum(0), eta=eta.sum(0), eta2=(eta * eta).sum(0)))
    s = SiteSummary(counts, sums)
    assert s.n_draws.tolist() == list(lengths) and s.n_sites == n
    cat = {k: np.concatenate([h[k] for h in hist]) for k in hist[0]}

    def close(a, b):
        return np.max(np.abs(a - b) / np.abs(b)) <= 1e-12

    assert close(s.psi, cat['psi'].mean(0))
    assert close(s.occupancy, cat['occ'].mean(0))
    assert close(s.z_mean, cat['z'].mean(0))
    assert close(s.eta_mean, cat['eta'].mean(0))
    assert close(s.eta_sd, cat['eta'].std(0, ddof=1))
    for c, h in enumerate(hist):
        assert close(s.per_chain['psi'][c], h['psi'].mean(0))
        assert close(s.per_chain['occupancy'][c], h['occ'].mean(0))
        assert close(s.per_chain['z_mean'][c], h['z'].mean(0))
        assert close(s.per_chain['eta_mean'][c], h['eta'].mean(0))
    assert s.per_chain['psi'].shape == (3, n)
    # pooling is the merge of the sums (chains weigh by their draws), not a mean of means
    w = np.array(lengths, dtype=float)[:, None]
    assert close(s.psi, (s.per_chain['psi'] * w).sum(0) / w.sum())
    assert not np.allclose(s.psi, s.per_chain['psi'].mean(0), rtol=1e-9, atol=0)
    with pytest.raises(ValueError):
        SiteSummary([3, 4], sums)


def test_every_site_state_name_is_in_header_and_binding():
    from occuspytial_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    comments = ' '.join(re.findall(r'/\*.*?\*/', header, flags=re.S))
    documented = set(re.findall(r'\b(site_[a-z0-9]+)\b', comments))
    assert set(SITE_NAMES) <= documented, set(SITE_NAMES) - documented
    assert set(_lib.SITE_FIELDS) == set(SITE_NAMES)
    assert re.search(r'#define OCC_ABI_VERSION 7\b', header)   # no layout change came with them


def test_probit_and_python_step_samplers_refuse_site_summaries(monkeypatch):
    """Both raise before any engine exists: creating one here would need a device."""
    from occuspytial_amd import ProbitRSRGibbs, _engine
    from occuspytial_amd.gibbs.base import GibbsBase

    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(_engine.Engine, '__init__', no_engine)
    Q, W, X, y = _inputs(load_golden('ref_queen150_ragged'))[:4]
    with pytest.raises(NotImplementedError, match='probit'):
        ProbitRSRGibbs(Q, W, X, y, random_state=1, q=10).sample(5, site_summaries=True)

    class PyStep(GibbsBase):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._configure(a[0], None)

        def step(self):
            raise AssertionError('step was called')

    with pytest.raises(NotImplementedError, match='Python'):
        PyStep(Q, W, X, y, random_state=1).sample(5, site_summaries=True)


def test_a_library_without_the_feature_is_refused_and_the_default_asks_nothing(cpu_abi):  # noqa: F811
    from occuspytial_amd import LogitICARGibbs
    Q, W, X, y = _inputs(load_golden('ref_queen150_ragged'))[:4]
    with pytest.raises(ValueError, match='no site summaries'):
        LogitICARGibbs(Q, W, X, y, random_state=3).sample(5, chains=1, progressbar=False, site_summaries=True)
    out = LogitICARGibbs(Q, W, X, y, random_state=3).sample(5, chains=1, progressbar=False)
    assert out.sites is None and out['alpha'].shape[:2] == (1, 5)
