"""Held-out predictive scoring from the sums the engine keeps on the device (``Engine.holdout_sums``), and the helpers of a
K-fold run: :func:`split` makes the folds, the user fits one sampler per fold with the fold's sites left out, and
:func:`combine` joins the folds' scores."""
import hashlib

import numpy as np

SLOTS = ('cnt', 'lik', 'log', 'log2', 'pd')   # the five slots per held-out entry, in the engine's order


def _site_rows(W, y, site, q):
    """One site's withheld visits as ``(V, q)`` float64 and ``(V,)`` float64, or ``ValueError``."""
    w = np.asarray(W[site], dtype=np.float64)
    v = np.asarray(y[site], dtype=np.float64).ravel()
    if w.ndim == 1 and q == 1:
        w = w.reshape(-1, 1)
    if w.ndim != 2 or w.shape[1] != q:
        raise ValueError('W_test[%r] must have %d columns (the detection covariates of the fitted problem), not shape %s' % (site, q, w.shape))
    if w.shape[0] < 1 or w.shape[0] != v.size:
        raise ValueError('W_test[%r] and y_test[%r] must have the same number of visits, at least one' % (site, site))
    if not np.all(np.isfinite(w)):
        raise ValueError('W_test[%r] must be finite' % (site,))
    if not np.all((v == 0.0) | (v == 1.0)):
        raise ValueError('y_test[%r] must hold 0 and 1 only' % (site,))
    return w, v


def holdout_arg(arg, problem):
    """The ``holdout=`` argument of ``sample`` / ``resume`` -- ``(W_test, y_test)``, dicts keyed by site like the
    constructor's ``W`` and ``y`` -- as the array the library takes under the state name ``holdout_data``:
    ``[H, R, site[H], ptr[H + 1], y[R], W[R q] row-major]``, the entries in ascending order of site.

    ``ValueError`` on anything but a pair of non-empty dicts, on keys that differ between the two, on a site outside
    ``[0, n)`` or one that ``problem`` surveys (a held-out site is left out of the fitted ``W`` and ``y``), on a wrong
    number of columns, unequal or zero visits, a non-finite covariate, or a ``y`` that is not 0 or 1."""
    try:
        W, y = arg
    except (TypeError, ValueError):
        raise ValueError('holdout must be a pair (W_test, y_test) of dicts keyed by site') from None
    if not hasattr(W, 'keys') or not hasattr(y, 'keys') or len(W) < 1:
        raise ValueError('holdout must be a pair (W_test, y_test) of non-empty dicts keyed by site')
    if set(W.keys()) != set(y.keys()):
        raise ValueError('W_test and y_test must have the same sites as keys')
    n, q = int(problem.n), int(problem.q)
    surveyed = set(int(s) for s in np.asarray(problem.site_id).ravel())
    keyed = {}
    for site in W.keys():
        if isinstance(site, (bool, np.bool_)) or not isinstance(site, (int, np.integer)):
            raise ValueError('a held-out site is an integer site number, not %r' % (site,))
        if not 0 <= int(site) < n:
            raise ValueError('held-out site %d is outside [0, %d)' % (int(site), n))
        if int(site) in surveyed:
            raise ValueError('site %d is surveyed in the fitted problem: a held-out site is left out of W and y' % int(site))
        keyed[int(site)] = site
    sites = sorted(keyed)
    rows = [_site_rows(W, y, keyed[s], q) for s in sites]
    ptr = np.concatenate([[0], np.cumsum([w.shape[0] for w, _ in rows])])
    return np.concatenate([[len(sites), ptr[-1]], sites, ptr, np.concatenate([v for _, v in rows]),
                           np.concatenate([w.ravel() for w, _ in rows])]).astype(np.float64)


def unpack(packed, q):
    """``(site (H,), ptr (H + 1,), y (R,), W (R, q))`` of the array :func:`holdout_arg` packs."""
    packed = np.asarray(packed, dtype=np.float64).ravel()
    H, R = int(packed[0]), int(packed[1])
    if packed.size != 2 + 2 * H + 1 + R + R * int(q):
        raise ValueError('the packed held-out data have the wrong length for %d entries, %d rows and %d columns' % (H, R, int(q)))
    site = packed[2:2 + H].astype(np.int64)
    ptr = packed[2 + H:3 + 2 * H].astype(np.int64)
    y = packed[3 + 2 * H:3 + 2 * H + R]
    return site, ptr, y, packed[3 + 2 * H + R:].reshape(R, int(q))


def _data_ids(packed, q):
    """One 64-bit fingerprint per entry of its site and its withheld detection history: what says that two scores were
    formed on the same withheld data.  The covariates are the model's, not the data's: two models that are compared may
    well differ in them."""
    site, ptr, y, _ = unpack(packed, q)
    ids = np.empty(site.size, dtype=np.uint64)
    for h in range(site.size):
        a, b = ptr[h], ptr[h + 1]
        d = hashlib.sha256(np.int64(site[h]).tobytes() + np.ascontiguousarray(y[a:b]).tobytes())
        ids[h] = int.from_bytes(d.digest()[:8], 'little')
    return ids


def _auc(score, label):
    """Area under the ROC curve from ranks, ties averaged (the Mann-Whitney statistic); NaN when ``label`` is all one value."""
    label = np.asarray(label, dtype=bool)
    n1 = int(label.sum())
    n0 = label.size - n1
    if n1 == 0 or n0 == 0:
        return float('nan')
    _, inv, cnt = np.unique(score, return_inverse=True, return_counts=True)
    last = np.cumsum(cnt)                       # the highest rank of every tie group
    rank = (last - (cnt - 1) / 2.0)[inv]        # ... and the group's mean rank
    return float((rank[label].sum() - n1 * (n1 + 1) / 2.0) / (n1 * n0))


class HoldoutScore:
    r"""How well a fit predicts detection histories it has not seen, at sites it did not survey.

    Over the kept iterations the engine adds, per held-out site, :math:`L` -- the marginal likelihood of the site's
    withheld visits given the draw's :math:`\alpha, \beta, \eta`, the occupancy state integrated out --
    :math:`\ell = \log L`, :math:`\ell^2` and ``pd``, the predictive probability of at least one detection in those
    visits, and counts the iterations, per chain.  This class turns those sums into scores; it never sees a draw.

    ``HoldoutScore(per_chain_sums, sites, detected)``: ``per_chain_sums[c]`` the ``(5, H)`` sums of chain ``c`` (rows
    ``cnt``, ``lik``, ``log``, ``log2``, ``pd``; a dict with the key ``sums``, as ``Engine.holdout_sums`` returns, is taken
    too), ``sites`` the ``H`` held-out site numbers, ``detected`` whether each withheld history has a detection.  The
    chains are pooled by adding sums; ``N`` is the pooled count per site.

    Pointwise, ``(H,)``: ``elpd_i`` = :math:`\log(\sum L / N)`, the log predictive density of the withheld history (``-inf``
    at a site whose likelihood underflowed to 0 in every draw: the sum is not shifted, as in
    :class:`~occuspytial_amd.waic.WAIC`); ``mean_loglik_i`` = :math:`\sum\ell / N`; ``p_detect`` = :math:`\sum` ``pd``
    :math:`/ N`.  Totals: ``elpd`` (the sum over the sites), ``se = sqrt(H var(elpd_i))`` (``ddof = 1`` over the sites;
    NaN for one site), ``brier = mean((p_detect - detected)^2)``, ``auc`` (rank-based, ties averaged, NaN when
    ``detected`` is all one value), ``n_draws`` (per chain), ``sites``, ``detected``, ``n_sites``.
    """

    def __init__(self, per_chain_sums, sites, detected, data_ids=None):
        parts = [np.asarray(p['sums'] if hasattr(p, 'keys') else p, dtype=np.float64) for p in per_chain_sums]
        sites = np.asarray(sites, dtype=np.int64).ravel()
        if not parts or any(p.shape != (len(SLOTS), sites.size) for p in parts):
            raise ValueError('one (5, H) array of sums per chain is required, H the number of held-out sites')
        for p in parts:
            if np.any(p[0] < 0) or np.any(p[0] != np.floor(p[0])) or np.any(p[0] != p[0, 0]):
                raise ValueError('the cnt row of a chain holds one whole number of iterations at every site')
        n_draws = np.array([p[0, 0] if p.shape[1] else 0 for p in parts], dtype=np.int64)
        self._set(np.sum(parts, axis=0), sites, detected, n_draws, data_ids)   # the exact merge: sums add

    def _set(self, sums, sites, detected, n_draws, data_ids):
        detected = np.asarray(detected).ravel()
        if detected.size != sites.size or not np.all((detected == 0) | (detected == 1)):
            raise ValueError('detected holds one 0 / 1 flag per held-out site')
        if np.unique(sites).size != sites.size:
            raise ValueError('a held-out site appears twice')
        self.sums = sums
        self.sites = sites
        self.detected = detected.astype(bool)
        self.n_sites = H = sites.size
        self.n_draws = n_draws
        self.data_ids = None if data_ids is None else np.asarray(data_ids, dtype=np.uint64).ravel()
        N = sums[0]
        with np.errstate(divide='ignore', invalid='ignore'):
            self.elpd_i = np.log(sums[1] / N)
            self.mean_loglik_i = sums[2] / N
            self.p_detect = sums[4] / N
            self.elpd = float(self.elpd_i.sum())
            self.se = float(np.sqrt(H * np.var(self.elpd_i, ddof=1))) if H > 1 else float('nan')
            self.brier = float(np.mean((self.p_detect - self.detected) ** 2))
        self.auc = _auc(self.p_detect, self.detected)

    @classmethod
    def from_engine(cls, eng):
        """Read every chain's sums from an ``Engine`` / ``EngineGroup`` (once, at the end of a run)."""
        site, ptr, y, _ = unpack(eng._holdout, eng.prob.q)
        detected = np.add.reduceat(y, ptr[:-1]) > 0
        return cls([eng.holdout_sums(c) for c in range(eng.n_chains)], site, detected, _data_ids(eng._holdout, eng.prob.q))

    def __repr__(self):
        return (f'HoldoutScore(elpd={self.elpd:.2f}, se={self.se:.2f}, brier={self.brier:.4f}, auc={self.auc:.3f}, '
                f'sites={self.n_sites}, n_draws={self.n_draws.tolist()})')


def _same_data(a, b):
    if not np.array_equal(a.sites, b.sites) or not np.array_equal(a.detected, b.detected):
        return False
    return a.data_ids is None or b.data_ids is None or np.array_equal(a.data_ids, b.data_ids)


def compare(a, b):
    r"""``{'elpd_diff', 'se_diff'}`` of two :class:`HoldoutScore` results on the same withheld data: ``elpd_diff = a.elpd -
    b.elpd`` (positive: ``a`` predicts better) and ``se_diff = sqrt(H var(a.elpd_i - b.elpd_i))`` (``ddof = 1`` over the
    sites), the standard error of the paired difference.  Results over different sites, or over the same sites with
    different withheld visits, are refused with ``ValueError``."""
    if not _same_data(a, b):
        raise ValueError('the two results cover different sites or different withheld data: held-out scores compare models on the same data')
    d = a.elpd_i - b.elpd_i
    H = d.size
    with np.errstate(invalid='ignore'):
        se = float(np.sqrt(H * np.var(d, ddof=1))) if H > 1 else float('nan')
    return {'elpd_diff': float(a.elpd - b.elpd), 'se_diff': se}


def combine(scores):
    """The disjoint folds of a K-fold run as one :class:`HoldoutScore` over all their sites, in ascending order of site
    (``n_draws``: the folds' per-chain counts one after the other).  Overlapping sites are refused with ``ValueError``."""
    scores = list(scores)
    if not scores:
        raise ValueError('at least one score is required')
    sites = np.concatenate([s.sites for s in scores])
    if np.unique(sites).size != sites.size:
        raise ValueError('the folds overlap: a site is held out in more than one of them')
    order = np.argsort(sites, kind='stable')
    ids = None if any(s.data_ids is None for s in scores) else np.concatenate([s.data_ids for s in scores])[order]
    out = HoldoutScore.__new__(HoldoutScore)
    out._set(np.concatenate([s.sums for s in scores], axis=1)[:, order], sites[order], np.concatenate([s.detected for s in scores])[order],
             np.concatenate([s.n_draws for s in scores]), ids)
    return out


def split(W, y, k, seed=None, blocks=None):
    """The ``k`` folds of a K-fold run: yields ``(W_train, y_train, W_test, y_test)``, dicts keyed by site, ``k`` times.

    The surveyed sites (the keys of ``W`` and ``y``) are grouped into folds by site, or by ``blocks[site]`` when given -- a
    mapping or an array with the block of every site -- for spatially blocked cross-validation: a block is never divided
    between folds.  The groups are dealt to the folds in turn, in ascending order, or in the order ``seed`` shuffles them
    into: the folds are disjoint, cover every surveyed site once, and are the same for the same ``seed``."""
    if set(W.keys()) != set(y.keys()):
        raise ValueError('W and y must have the same sites as keys')
    sites = sorted(W.keys())
    label = {s: (blocks[s] if blocks is not None else s) for s in sites}
    groups = sorted(set(label.values()))
    k = int(k)
    if k < 2 or k > len(groups):
        raise ValueError('k must lie between 2 and the number of %s (%d)' % ('blocks' if blocks is not None else 'sites', len(groups)))
    order = np.arange(len(groups)) if seed is None else np.random.default_rng(seed).permutation(len(groups))
    fold = {groups[g]: j % k for j, g in enumerate(order)}
    for f in range(k):
        test = [s for s in sites if fold[label[s]] == f]
        train = [s for s in sites if fold[label[s]] != f]
        yield {s: W[s] for s in train}, {s: y[s] for s in train}, {s: W[s] for s in test}, {s: y[s] for s in test}
