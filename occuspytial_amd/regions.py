"""Finite-sample occupancy per region from the counts the engine records per draw (``Engine.region_draws``)."""
import numpy as np

MAX_REGIONS = 256   # region ids are whole numbers in [-1, MAX_REGIONS); -1: the site belongs to no region


def region_ids(regions, n):
    """The ``regions=`` argument of ``sample`` / ``resume`` as an array of ``n`` region ids, or ``None`` for ``None``.

    ``True`` is the whole lattice as one region; an integer array of length ``n`` gives the region of every site, ``-1``
    for a site of no region.  Anything else -- ``False``, a float or boolean array, a wrong length, an id below ``-1`` or
    of ``MAX_REGIONS`` and above -- is a ``ValueError``.
    """
    if regions is None:
        return None
    if regions is True:
        return np.zeros(int(n), dtype=np.int64)
    if isinstance(regions, (bool, np.bool_, str, bytes)) or np.isscalar(regions):
        raise ValueError('regions must be None, True or an integer array with one region id per site')
    try:
        ids = np.asarray(regions)
    except Exception:
        raise ValueError('regions must be None, True or an integer array with one region id per site') from None
    if ids.dtype.kind not in 'iu':
        raise ValueError('regions must hold integers (the region of every site, -1 for none), not %s' % ids.dtype)
    if ids.shape != (int(n),):
        raise ValueError('regions must have one region id per site: shape (%d,), not %s' % (int(n), ids.shape))
    if ids.size and (ids.min() < -1 or ids.max() >= MAX_REGIONS):
        raise ValueError('region ids lie in [-1, %d)' % MAX_REGIONS)
    return ids.astype(np.int64)


class RegionOccupancy:
    r"""Occupied sites per region and draw: :math:`N_g(t) = \sum_{i \in g} z_i(t)`, the finite-sample occupancy.

    ``RegionOccupancy(ids, detected_sites, occupied)``: ``ids`` the region of every site (``-1``: none), ``detected_sites``
    the sites with a detection, ``occupied`` the counts ``(chains, draws, G)`` with ``G = max(ids) + 1`` (at least 1).

    * ``ids`` -- ``(n,)`` the map;
    * ``n_regions`` -- ``G``;
    * ``sizes`` -- ``(G,)`` sites per region;
    * ``detected`` -- ``(G,)`` sites with a detection per region: their z is 1 in every draw, so this is the floor of
      every count;
    * ``occupied`` -- ``(chains, draws, G)`` float64 counts, the ``post['occupied']`` of the same result;
    * ``pao`` -- ``occupied / sizes``, the proportion of area occupied per draw (NaN for a region without sites).

    The draws are dependent across sites, so intervals, effective sample sizes and R-hat of a region's count come from
    these rows (``post.summary``), never from per-site means.
    """

    def __init__(self, ids, detected_sites, occupied):
        ids = np.asarray(ids, dtype=np.int64).ravel()
        occupied = np.asarray(occupied, dtype=np.float64)
        G = max(int(ids.max()) + 1, 1) if ids.size else 1
        if occupied.ndim != 3 or occupied.shape[2] != G:
            raise ValueError('occupied must be (chains, draws, %d)' % G)
        seen = np.zeros(ids.size, dtype=bool)
        seen[np.asarray(detected_sites, dtype=np.int64)] = True
        self.ids = ids
        self.n_regions = G
        self.sizes = np.bincount(ids[ids >= 0], minlength=G).astype(np.int64)
        self.detected = np.bincount(ids[(ids >= 0) & seen], minlength=G).astype(np.int64)
        self.occupied = occupied
        with np.errstate(divide='ignore', invalid='ignore'):
            self.pao = occupied / self.sizes

    def __repr__(self):
        return f'RegionOccupancy(regions={self.n_regions}, chains={self.occupied.shape[0]}, draws={self.occupied.shape[1]})'
