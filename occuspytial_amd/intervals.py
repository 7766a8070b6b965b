"""Per-site credible intervals of the occupancy probability from the histograms the engine keeps on the device
(``Engine.hist_counts``)."""
import math

import numpy as np

BINS_DEFAULT, BINS_MIN, BINS_MAX = 64, 4, 1024


def interval_bins(value):
    """The ``site_intervals`` keyword of ``sample`` / ``resume`` as a number of bins: ``False`` is 0 (off), ``True`` is 64, an
    integer from 4 to 1024 is itself; anything else -- ``None`` and floats included -- is refused."""
    if isinstance(value, (bool, np.bool_)):
        return BINS_DEFAULT if value else 0
    if isinstance(value, (int, np.integer)) and BINS_MIN <= int(value) <= BINS_MAX:
        return int(value)
    raise ValueError('site_intervals must be True, False or a number of bins from 4 to 1024')


class SiteIntervals:
    r"""Credible intervals, quantiles and exceedance probabilities of :math:`\psi_i` per site, without the draws.

    :math:`\psi_i = \mathrm{expit}(x_i\beta + \eta_i)` lives in (0, 1).  Per site and chain the engine keeps a histogram of it
    with ``B`` equal bins -- bin ``b`` counts the iterations with :math:`b/B \le \psi_i < (b+1)/B` (the last one takes
    :math:`\psi_i = 1` as well) -- so every quantile of :math:`\psi_i` is known to within ``1 / B``, with an exact bracket.
    This class never sees a draw.

    ``SiteIntervals(counts)``: ``counts`` of shape ``(chains, B, n)``, whole numbers.  The chains are pooled by the exact
    merge: the counts add.

    With ``N`` the pooled draws of a site, ``k = max(1, ceil(q N))`` (``q N`` within 1e-9 of a whole number is that number:
    ``q`` itself is rounded), ``c_b`` the cumulative counts and ``b*`` the smallest
    ``b`` with ``c_b >= k``:

    * ``bounds(q)`` -- ``(lo, hi) = (b*/B, (b*+1)/B)``, arrays of length ``n``: they bracket the ``k``-th smallest pooled
      draw of :math:`\psi_i` exactly;
    * ``quantile(q)`` -- ``lo + (k - c_{b*-1} - 1/2) / count_{b*} / B``: interpolated inside the bin, so within ``1 / B`` of
      that draw;
    * ``interval(prob=0.95)`` -- the equal-tailed interval ``(quantile((1 - prob) / 2), quantile((1 + prob) / 2))``;
      ``width(prob=0.95)`` its width; ``median`` is ``quantile(0.5)``;
    * ``prob_above(t)`` -- :math:`P(\psi_i \ge t \mid \text{data})`: the share of the draws in the bins above ``t``, exact
      when ``t B`` is whole and interpolated linearly inside ``t``'s bin otherwise;
    * ``n_draws`` -- ``(chains,)`` iterations per chain; ``per_chain_counts`` -- the counts as given; ``bins``;
      ``n_sites``; ``resolution = 1 / B``.

    A site without a draw gives NaN everywhere.
    """

    def __init__(self, counts):
        raw = np.asarray(counts)
        if raw.ndim != 3 or raw.shape[0] < 1 or not BINS_MIN <= raw.shape[1] <= BINS_MAX:
            raise ValueError('counts must have the shape (chains, bins, sites) with 4 to 1024 bins')
        if raw.dtype.kind not in 'iuf' or (raw.dtype.kind == 'f' and not np.all(np.isfinite(raw))):
            raise ValueError('counts are whole numbers')
        if np.any(raw < 0) or (raw.dtype.kind == 'f' and np.any(raw != np.floor(raw))):
            raise ValueError('counts are whole numbers, none below zero')
        self.per_chain_counts = raw.astype(np.int64)
        self.bins = int(raw.shape[1])
        self.n_sites = int(raw.shape[2])
        self.resolution = 1.0 / self.bins
        per_site = self.per_chain_counts.sum(axis=1)                       # (chains, n): every site of a chain counts every iteration
        self.n_draws = per_site.max(axis=1) if self.n_sites else np.zeros(raw.shape[0], dtype=np.int64)
        self._pooled = self.per_chain_counts.sum(axis=0)                   # the exact merge: counts add
        self._cum = np.cumsum(self._pooled, axis=0)
        self._total = self._cum[-1] if self.n_sites else np.zeros(0, dtype=np.int64)

    @classmethod
    def from_engine(cls, eng):
        """Read every chain's histograms from an ``Engine`` / ``EngineGroup`` (once, at the end of a run)."""
        return cls(np.stack([eng.hist_counts(c)['counts'] for c in range(eng.n_chains)]))

    def _locate(self, q):
        """-> (k, b*, draws of the bins below b*, count of b*, sites with a draw) of the ``q`` quantile, per site."""
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError('a quantile is asked for with 0 <= q <= 1')
        N = self._total
        some = N > 0
        x = q * N.astype(np.float64)
        near = np.rint(x)                                  # (q N a whole number but for the rounding of q: 0.025 N, (1 - 0.95) / 2 N)
        x = np.where(np.abs(x - near) <= 1e-9 * np.maximum(near, 1.0), near, np.ceil(x))
        k = np.clip(x.astype(np.int64), 1, np.maximum(N, 1))
        b = np.argmax(self._cum >= k[None, :], axis=0) if self.n_sites else np.zeros(0, dtype=np.int64)
        col = np.arange(self.n_sites)
        inside = self._pooled[b, col]
        below = self._cum[b, col] - inside
        return k, b, below, inside, some

    def bounds(self, q):
        """``(lo, hi)``: the edges of the bin that holds the ``k``-th smallest pooled draw of every site."""
        _, b, _, _, some = self._locate(q)
        lo = np.where(some, b / self.bins, np.nan)
        hi = np.where(some, (b + 1) / self.bins, np.nan)
        return lo, hi

    def quantile(self, q):
        """The ``q`` quantile of psi per site, interpolated inside its bin: within ``resolution`` of the ``k``-th draw."""
        k, b, below, inside, some = self._locate(q)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(some, b / self.bins + (k - below - 0.5) / inside / self.bins, np.nan)

    def interval(self, prob=0.95):
        """The equal-tailed credible interval of psi per site: ``(lower, upper)``."""
        prob = float(prob)
        if not 0.0 < prob < 1.0:
            raise ValueError('the probability of an interval lies strictly between 0 and 1')
        return self.quantile((1.0 - prob) / 2.0), self.quantile((1.0 + prob) / 2.0)

    def width(self, prob=0.95):
        lo, hi = self.interval(prob)
        return hi - lo

    @property
    def median(self):
        return self.quantile(0.5)

    def prob_above(self, t):
        """P(psi_i >= t | data) per site: exact when ``t * bins`` is whole, interpolated inside ``t``'s bin otherwise."""
        t = float(t)
        if not 0.0 <= t <= 1.0:
            raise ValueError('psi lies between 0 and 1: so must the threshold')
        j = t * self.bins
        whole = round(j)
        N = self._total.astype(np.float64)
        above = lambda first: self._pooled[first:].sum(axis=0).astype(np.float64)   # noqa: E731
        with np.errstate(divide='ignore', invalid='ignore'):
            if abs(j - whole) <= 1e-9:                     # (t = j / B as floating point gives back j only to rounding)
                return np.where(N > 0, above(int(whole)) / N, np.nan)
            first = math.floor(j)
            part = (first + 1 - j) * self._pooled[first]
            return np.where(N > 0, (above(first + 1) + part) / N, np.nan)

    def __repr__(self):
        return f'SiteIntervals(sites={self.n_sites}, bins={self.bins}, n_draws={self.n_draws.tolist()})'

