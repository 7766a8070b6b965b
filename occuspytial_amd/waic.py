"""Streaming WAIC from the per-site log-likelihood sums the engine keeps on the device (``Engine.loglik_sums``)."""
import numpy as np

SUM_NAMES = ('lik', 'log', 'log2')


class WAIC:
    r"""The widely applicable information criterion of an occupancy model, from three streaming sums per site.

    The likelihood is the site-level marginal one, with the occupancy state :math:`z_i` integrated out.  Over the kept
    iterations the engine adds, at every surveyed site, :math:`L_i` (the likelihood of the site's visits given
    :math:`\alpha, \beta, \eta`), :math:`\ell_i = \log L_i` and :math:`\ell_i^2`, and counts the iterations, per chain.
    This class turns those sums into WAIC; it never sees a draw.

    ``WAIC(counts, sums, site_id)``: ``counts[c]`` the iterations chain ``c`` accumulated, ``sums[c]`` its dict of three
    arrays of length ``n`` (keys ``lik``, ``log``, ``log2``), ``site_id`` the numbers of the ``S`` surveyed sites.  Only
    those sites enter.  The chains are pooled by merging the sums exactly (sum of sums over sum of counts, not a mean of
    per-chain values), as :class:`~occuspytial_amd.sites.SiteSummary` pools; ``N`` is the pooled number of draws.

    Pointwise, ``(S,)``:

    * ``lppd_i`` -- :math:`\log(\sum L / N)`, the log pointwise predictive density;
    * ``p_waic_i`` -- the variance of :math:`\ell` over the draws with ``ddof = 1``;
    * ``elpd_i`` -- ``lppd_i - p_waic_i``.

    Totals: ``lppd``, ``p_waic``, ``elpd`` (sums over the sites), ``waic = -2 elpd``, ``se = 2 sqrt(S var(elpd_i))``
    (``ddof = 1`` over the sites), ``n_draws`` (per chain), ``site_id``, ``n_sites``, and ``n_high_var``, the number of
    sites with ``p_waic_i > 0.4`` -- the usual threshold above which WAIC is held to be unreliable.

    Accuracy of ``p_waic_i``.  It is formed from plain sums, :math:`(\sum\ell^2 - (\sum\ell)^2 / N) / (N - 1)`: both sums
    carry a relative rounding error of about :math:`N\,2^{-53}`, and the subtraction magnifies it by the ratio of what
    is subtracted to what is left, so the variance has a relative error of about
    :math:`N\,2^{-53}\,(1 + \mathrm{mean}^2 / \mathrm{var})`.  For :math:`10^4` draws of a log-likelihood whose mean is ten
    standard deviations from zero that is :math:`10^{-10}`; a variance that rounding turns negative is reported as 0.

    Underflow.  ``lppd_i`` is formed from the plain sum of :math:`L`: at a site whose likelihood underflows to 0 in every
    draw (:math:`\ell < -745`) it is ``-inf``, and so are the totals.  The sum is not shifted.
    """

    def __init__(self, counts, sums, site_id):
        counts = np.atleast_1d(np.asarray(counts, dtype=np.float64))
        if counts.ndim != 1 or len(sums) != counts.size or counts.size < 1:
            raise ValueError('one count and one dict of sums per chain are required')
        if np.any(counts < 0) or np.any(counts != np.floor(counts)):
            raise ValueError('counts are whole numbers of iterations')
        site_id = np.asarray(site_id, dtype=np.int64).ravel()
        tot = {}
        for name in SUM_NAMES:
            full = np.stack([np.asarray(s[name], dtype=np.float64).ravel() for s in sums])
            if full.shape != (counts.size, np.asarray(sums[0]['lik']).size):
                raise ValueError('the sums of every chain must have one value per site')
            if site_id.size and (site_id.min() < 0 or site_id.max() >= full.shape[1]):
                raise ValueError('site_id names a site the sums do not cover')
            tot[name] = full[:, site_id].sum(axis=0)   # the exact merge: sums add
        self.n_draws = counts.astype(np.int64)
        self.site_id = site_id
        self.n_sites = S = site_id.size
        N = float(counts.sum())
        with np.errstate(divide='ignore', invalid='ignore'):
            self.lppd_i = np.log(tot['lik'] / N)
            var = (tot['log2'] - tot['log'] * tot['log'] / N) / (N - 1.0) if N > 1 else np.full(S, np.nan)
            self.p_waic_i = np.maximum(var, 0.0)
            self.elpd_i = self.lppd_i - self.p_waic_i
            self.lppd = float(self.lppd_i.sum())
            self.p_waic = float(self.p_waic_i.sum())
            self.elpd = float(self.elpd_i.sum())
            self.waic = -2.0 * self.elpd
            self.se = 2.0 * float(np.sqrt(S * np.var(self.elpd_i, ddof=1))) if S > 1 else float('nan')
        self.n_high_var = int(np.count_nonzero(self.p_waic_i > 0.4))

    @classmethod
    def from_engine(cls, eng):
        """Read every chain's count and sums from an ``Engine`` / ``EngineGroup`` (once, at the end of a run)."""
        parts = [eng.loglik_sums(c) for c in range(eng.n_chains)]
        return cls([p['count'] for p in parts], parts, eng.prob.site_id)

    def __repr__(self):
        return (f'WAIC(waic={self.waic:.2f}, se={self.se:.2f}, elpd={self.elpd:.2f}, p_waic={self.p_waic:.2f}, '
                f'sites={self.n_sites}, n_draws={self.n_draws.tolist()}, n_high_var={self.n_high_var})')


def compare(a, b):
    r"""``{'elpd_diff', 'se_diff'}`` of two :class:`WAIC` results on the same data: ``elpd_diff = a.elpd - b.elpd``
    (positive: ``a`` predicts better) and ``se_diff = sqrt(S var(a.elpd_i - b.elpd_i))`` (``ddof = 1`` over the sites), the
    standard error of the paired difference.  Both must cover the same ``site_id``, else ``ValueError``.  This is what
    the ``r`` / ``q`` knob of the reduced-rank model, the choice between it and the ICAR prior, and a choice between
    covariate sets are decided with."""
    if a.site_id.shape != b.site_id.shape or not np.array_equal(a.site_id, b.site_id):
        raise ValueError('the two results cover different sites: WAIC compares models on the same data')
    d = a.elpd_i - b.elpd_i
    S = d.size
    with np.errstate(invalid='ignore'):
        se = float(np.sqrt(S * np.var(d, ddof=1))) if S > 1 else float('nan')
    return {'elpd_diff': float(a.elpd - b.elpd), 'se_diff': se}
