"""Per-site posterior summaries from the running sums the engine keeps on the device (``Engine.site_sums``)."""
import numpy as np

SUM_NAMES = ('psi', 'occ', 'z', 'eta', 'eta2')


class SiteSummary:
    r"""The posterior map of an occupancy model: one value per site, from streaming moments.

    The engine adds five terms per site and kept iteration -- :math:`\psi_i = \mathrm{expit}(x_i\beta + \eta_i)`, the
    conditional occupancy probability :math:`P(z_i = 1 \mid \alpha, \beta, \eta, y)` of the z update, the new
    :math:`z_i`, :math:`\eta_i` and :math:`\eta_i^2` -- and counts the iterations, per chain.  This class turns those sums
    into means; it never sees a draw.

    ``SiteSummary(counts, sums)``: ``counts[c]`` the iterations chain ``c`` accumulated, ``sums[c]`` its dict of the
    five arrays of length ``n`` (keys ``psi``, ``occ``, ``z``, ``eta``, ``eta2``).

    Attributes, pooled over the chains by merging the sums exactly (sum of sums over sum of counts, not a mean of
    means, so chains of different length weigh by their draws):

    * ``n_draws`` -- ``(chains,)`` iterations per chain;
    * ``psi`` -- posterior mean occupancy probability;
    * ``occupancy`` -- :math:`P(z_i = 1 \mid \text{data})`, Rao-Blackwellised (exactly 1 at a site with a detection);
    * ``z_mean`` -- the raw frequency of :math:`z_i = 1`;
    * ``eta_mean``, ``eta_sd`` -- the spatial effect (reduced-rank model: :math:`(K\theta)_i`) and its posterior standard
      deviation with ``ddof = 1`` over the pooled draws, as ``diagnostics.py`` takes variances;
    * ``per_chain[name]`` -- ``(chains, n)``: the same means for every chain alone (``psi``, ``occupancy``, ``z_mean``,
      ``eta_mean``).

    Accuracy of ``eta_sd``.  It is formed from plain sums, :math:`(\sum\eta^2 - (\sum\eta)^2 / N) / (N - 1)`: both sums
    carry a relative rounding error of about :math:`N\,2^{-53}`, and the subtraction magnifies it by the ratio of what
    is subtracted to what is left, so the variance has a relative error of about
    :math:`N\,2^{-53}\,(1 + \mathrm{mean}^2 / \mathrm{var})`.  For :math:`10^4` draws of an effect whose mean is ten
    standard deviations from zero that is :math:`10^{-10}`; a variance that rounding turns negative is reported as 0.
    """

    def __init__(self, counts, sums):
        counts = np.atleast_1d(np.asarray(counts, dtype=np.float64))
        if counts.ndim != 1 or len(sums) != counts.size or counts.size < 1:
            raise ValueError('one count and one dict of sums per chain are required')
        if np.any(counts < 0) or np.any(counts != np.floor(counts)):
            raise ValueError('counts are whole numbers of iterations')
        S = {}
        for name in SUM_NAMES:
            S[name] = np.stack([np.asarray(s[name], dtype=np.float64).ravel() for s in sums])
            if S[name].shape != S['psi'].shape:
                raise ValueError('the sums of every chain must have one value per site')
        self.n_draws = counts.astype(np.int64)
        self.n_sites = S['psi'].shape[1]
        self._sums = S
        N = float(counts.sum())
        with np.errstate(divide='ignore', invalid='ignore'):
            per = counts[:, None]
            self.per_chain = {'psi': S['psi'] / per, 'occupancy': S['occ'] / per, 'z_mean': S['z'] / per,
                              'eta_mean': S['eta'] / per}
            tot = {name: S[name].sum(axis=0) for name in SUM_NAMES}   # the exact merge: sums add
            self.psi = tot['psi'] / N
            self.occupancy = tot['occ'] / N
            self.z_mean = tot['z'] / N
            self.eta_mean = tot['eta'] / N
            var = (tot['eta2'] - tot['eta'] * tot['eta'] / N) / (N - 1.0) if N > 1 else np.full(self.n_sites, np.nan)
            self.eta_sd = np.sqrt(np.maximum(var, 0.0))

    @classmethod
    def from_engine(cls, eng):
        """Read every chain's count and sums from an ``Engine`` / ``EngineGroup`` (once, at the end of a run)."""
        parts = [eng.site_sums(c) for c in range(eng.n_chains)]
        return cls([p['count'] for p in parts], parts)

    def __repr__(self):
        return f'SiteSummary(sites={self.n_sites}, n_draws={self.n_draws.tolist()})'
