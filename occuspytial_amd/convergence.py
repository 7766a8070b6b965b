"""Per-site convergence diagnostics -- R-hat, effective sample size and Monte-Carlo standard error of psi and eta at every
site -- from the batch-means sums the engine keeps on the device (``Engine.conv_sums``)."""
import math

import numpy as np

BATCH_MAX = 1 << 30
SLOTS = 11
QUANTITIES = {'psi': 1, 'eta': 6}   # the first of a quantity's five slots (ref, s1, s2, run, bsq); slot 0 is cnt
REF, S1, S2, RUN, BSQ = range(5)


def diagnostics_batch(value, kept=None):
    """The ``site_diagnostics`` keyword of ``sample`` / ``resume`` as a batch length: ``False`` is 0 (off), ``True`` is
    ``max(1, floor(sqrt(kept)))`` with ``kept`` the iterations the call keeps, an integer from 1 to 2^30 is itself; anything
    else -- ``None`` and floats included -- is refused."""
    if isinstance(value, (bool, np.bool_)):
        if not value:
            return 0
        return max(1, math.isqrt(max(int(kept or 0), 0)))
    if isinstance(value, (int, np.integer)) and 1 <= int(value) <= BATCH_MAX:
        return int(value)
    raise ValueError('site_diagnostics must be True, False or a batch length from 1 to 2^30')


class SiteDiagnostics:
    r"""R-hat across chains, effective sample size and Monte-Carlo standard error of the posterior mean, per site, for the
    occupancy probability :math:`\psi_i` (``'psi'``) and the spatial effect :math:`\eta_i` (``'eta'``), without the draws.

    ``SiteDiagnostics(per_chain_sums, L)``: ``per_chain_sums`` of shape ``(chains, 11, n)`` -- per chain and site the count
    ``cnt``, then ``ref, s1, s2, run, bsq`` of psi, then the same five of eta: with ``d = v - ref`` the value of an iteration
    less the first one counted, ``s1`` and ``s2`` the sums of ``d`` and ``d d``, ``run`` the sum of ``d`` over the unfinished
    batch and ``bsq`` the sum of the squared sums of the finished batches of ``L`` iterations.

    Per chain, with ``N = cnt``, ``a = floor(N / L)`` batches and ``T = s1 - run``:

    * chain mean ``ref + s1 / N``; chain variance ``(s2 - s1^2 / N) / (N - 1)``;
    * ``sigma2 = (bsq / L - T^2 / (a L)) / (a - 1)``: ``L`` times the ddof-1 variance of the ``a`` batch means, the
      batch-means estimate of the asymptotic variance.

    Per site, with ``W`` and ``sigma2`` averaged over chains:

    * ``mean(q)`` -- the posterior mean pooled over chains; ``var(q)`` -- ``W``;
    * ``ess(q)`` -- ``sum(N_c) W / sigma2``; ``mcse(q)`` -- ``sqrt(sigma2 / sum(N_c))``; both NaN with fewer than two
      finished batches, ESS also at a site that never moved (``W = 0``);
    * ``rhat(q)`` -- ``sqrt(((N - 1) / N W + B / N) / W)`` with ``B / N`` the ddof-1 variance of the chains' means: NaN
      with one chain, 1 at a site that never moved, ``ValueError`` when the chains counted different numbers of iterations;
    * ``worst(q, k=10)`` -- the indices of the ``k`` sites of largest R-hat (of smallest ESS with one chain), worst first;
    * ``n_draws`` -- ``(chains,)`` iterations per chain; ``batch`` -- ``L``; ``n_batches`` -- ``(chains,)``;
      ``per_chain_sums`` -- the sums as given; ``n_sites``.
    """

    def __init__(self, per_chain_sums, L):
        raw = np.asarray(per_chain_sums, dtype=np.float64)
        if raw.ndim != 3 or raw.shape[0] < 1 or raw.shape[1] != SLOTS:
            raise ValueError('per_chain_sums must have the shape (chains, 11, sites)')
        if isinstance(L, (bool, np.bool_)) or not isinstance(L, (int, np.integer)) or not 1 <= int(L) <= BATCH_MAX:
            raise ValueError('the batch length is a whole number from 1 to 2^30')
        cnt = raw[:, 0, :]
        if np.any(cnt < 0) or np.any(cnt != np.floor(cnt)) or np.any(cnt != cnt[:, :1]):
            raise ValueError('the counts of a chain are one whole number, not below zero')
        self.per_chain_sums = raw
        self.batch = int(L)
        self.n_chains = int(raw.shape[0])
        self.n_sites = int(raw.shape[2])
        self.n_draws = cnt[:, 0].astype(np.int64) if self.n_sites else np.zeros(self.n_chains, dtype=np.int64)
        self.n_batches = self.n_draws // self.batch

    @classmethod
    def from_engine(cls, eng):
        """Read every chain's sums from an ``Engine`` / ``EngineGroup`` (once, at the end of a run)."""
        parts = [eng.conv_sums(c) for c in range(eng.n_chains)]
        return cls(np.stack([p['sums'] for p in parts]), parts[0]['batch'])

    def _chains(self, q):
        """-> per chain and site: (N, a, mean, var, sigma2), the first two of shape (chains, 1)."""
        if q not in QUANTITIES:
            raise ValueError("the quantity is 'psi' or 'eta'")
        five = self.per_chain_sums[:, QUANTITIES[q]:QUANTITIES[q] + 5, :]
        ref, s1, s2, run, bsq = (five[:, k, :] for k in (REF, S1, S2, RUN, BSQ))
        N = self.n_draws.astype(np.float64)[:, None]
        a = self.n_batches.astype(np.float64)[:, None]
        L = float(self.batch)
        with np.errstate(divide='ignore', invalid='ignore'):
            mean = np.where(N > 0, ref + s1 / N, np.nan)
            var = np.where(N > 1, (s2 - s1 * s1 / N) / (N - 1.0), np.nan)
            T = s1 - run
            sigma2 = np.where(a > 1, (bsq / L - T * T / (a * L)) / (a - 1.0), np.nan)
        return N, a, mean, np.maximum(var, 0.0), np.maximum(sigma2, 0.0)   # (maximum keeps a NaN)

    def mean(self, q):
        """The posterior mean per site, pooled over chains."""
        N, _, mean, _, _ = self._chains(q)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(N > 0, N * mean, 0.0).sum(axis=0) / N.sum()

    def var(self, q):
        """``W``: the chains' mean of the within-chain variance, per site."""
        return self._chains(q)[3].mean(axis=0)

    def sigma2(self, q):
        """The chains' mean of the batch-means estimate of the asymptotic variance, per site (NaN below two batches)."""
        return self._chains(q)[4].mean(axis=0)

    def ess(self, q):
        """The effective sample size of the pooled draws per site."""
        N, _, _, var, sigma2 = self._chains(q)
        W, s2 = var.mean(axis=0), sigma2.mean(axis=0)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(W > 0, N.sum() * W / s2, np.nan)

    def mcse(self, q):
        """The Monte-Carlo standard error of the pooled posterior mean per site."""
        N, _, _, _, sigma2 = self._chains(q)
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.sqrt(sigma2.mean(axis=0) / N.sum())

    def rhat(self, q):
        """The potential scale reduction factor across chains per site."""
        N, _, mean, var, _ = self._chains(q)
        if np.any(self.n_draws != self.n_draws[0]):
            raise ValueError(f'R-hat needs chains of one length: these counted {self.n_draws.tolist()} iterations')
        if self.n_chains < 2:
            return np.full(self.n_sites, np.nan)
        n = float(self.n_draws[0])
        W = var.mean(axis=0)
        between = mean.var(axis=0, ddof=1)   # B / N
        with np.errstate(divide='ignore', invalid='ignore'):
            r = np.sqrt(((n - 1.0) / n * W + between) / W)
        return np.where(W > 0, r, np.where(W == 0, 1.0, np.nan))

    def worst(self, q, k=10):
        """The indices of the ``k`` sites of largest R-hat -- of smallest ESS with one chain --, worst first; a site whose
        figure is NaN comes last."""
        k = max(0, min(int(k), self.n_sites))
        if self.n_chains > 1:
            key = -np.nan_to_num(self.rhat(q), nan=-np.inf)
        else:
            key = np.nan_to_num(self.ess(q), nan=np.inf)
        return np.argsort(key, kind='stable')[:k]

    def __repr__(self):
        return f'SiteDiagnostics(sites={self.n_sites}, batch={self.batch}, n_draws={self.n_draws.tolist()})'
