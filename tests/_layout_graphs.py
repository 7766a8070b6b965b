"""Small deterministic graphs, one per branch of the layout of Q (occuspytial_amd/csrc/occ_layout.hpp) that the kernels
walking a row take: true SELL-64 bases (``ell_w = 0``) with rows of at most 8 / at most 16 / more than 16 off-diagonals, an
ELL layout wider than 16, slices of width 0 (64 aligned sites without neighbours) and a single isolated site -- plus the two
graphs of the general (non-diagonal) tile form.  tests/test_layout_graphs_cpu.py pins what each of them reaches (layout,
planner), tests/test_gpu_layout_graphs.py runs them on the device.  Every builder returns a scipy CSR ``Q = D - W`` in which
a site without neighbours has an EMPTY row (no stored diagonal); ``survey`` hangs a small occupancy survey on it."""
import numpy as np
from scipy import sparse


def laplacian(n, rows, cols, weights=None):
    """``Q = D - W`` of the undirected edges (rows[e], cols[e]); a repeated edge counts once; no stored zero."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    keep = lo != hi
    edge, first = np.unique(lo[keep] * n + hi[keep], return_index=True)
    lo, hi = edge // n, edge % n
    w = np.ones(edge.size) if weights is None else np.asarray(weights, dtype=np.float64)[keep][first]
    A = sparse.coo_matrix((np.concatenate([w, w]), (np.concatenate([lo, hi]), np.concatenate([hi, lo]))), shape=(n, n)).tocsr()
    Q = (sparse.diags(np.asarray(A.sum(axis=1)).ravel()) - A).tocsr()
    Q.eliminate_zeros()
    Q.sort_indices()
    return Q


def _ring_with_chords(m, hubs, chords, seed, matching=False):
    """Edges of a ring of m sites in which every site of ``hubs`` has ``chords`` chords to random sites that are neither hubs
    nor its ring neighbours (distinct per hub), and the first hub one more, to the fifth: the longest rows have
    2 + chords + 1 off-diagonals.  ``matching``: every site but the hubs also has one chord to a random partner."""
    rng = np.random.default_rng(seed)
    i = np.arange(m)
    rows, cols = [i], [(i + 1) % m]
    if matching:
        perm = rng.permutation(np.setdiff1d(i, hubs))
        rows.append(perm[0:perm.size - 1:2])
        cols.append(perm[1:perm.size:2])
    hubs = np.asarray(hubs)
    rows.append(hubs[:1])
    cols.append(hubs[4:5])
    for h in hubs:
        free = np.setdiff1d(i, np.concatenate([hubs, [(h - 1) % m, (h + 1) % m]]))
        rows.append(np.full(chords, h))
        cols.append(rng.choice(free, size=chords, replace=False))
    return np.concatenate(rows), np.concatenate(cols)


def _place(m, n, empty_slice):
    """Site numbers of ring sites 0 .. m-1 among n sites when slice ``empty_slice`` (64 aligned sites) stays without neighbours."""
    site = np.arange(n)
    return site[(site // 64) != empty_slice][:m]


def sell8(n=640, chords=5, seed=0):
    """Ring of n sites; 8 sites of slice 3 have ``chords`` random chords each: slices of width 2 + chords + 1 and of width 3, true SELL bases."""
    r, c = _ring_with_chords(n, 3 * 64 + 8 * np.arange(8) + 3, chords, seed)
    return laplacian(n, r, c)


def sell16():
    """The same with 12 chords: rows of up to 15 off-diagonals (k_iter's 16-wide window)."""
    return sell8(chords=12, seed=1)


def hub():
    """The irregular areal graph of ``make_graph_problem(700, k=4)`` plus one site joined to 40 random others: one row of more
    than 16 off-diagonals in a graph of narrow slices (the planner leaves it one launch per MINRES step)."""
    from occuspytial_amd.utils import make_graph_problem
    Q = make_graph_problem(n=700, k=4, visits=1, p=2, q=2, random_state=3)[0].tocoo()
    n = Q.shape[0]
    off = Q.row < Q.col
    rng = np.random.default_rng(3)
    deg = np.bincount(Q.row[off], minlength=n) + np.bincount(Q.col[off], minlength=n)
    centre = int(np.flatnonzero(deg == 6)[0])
    near = np.concatenate([[centre], Q.col[Q.row == centre]])
    spokes = rng.choice(np.setdiff1d(np.arange(n), near), size=40, replace=False)
    return laplacian(n, np.concatenate([Q.row[off], np.full(40, centre)]), np.concatenate([Q.col[off], spokes]))


WIDE_STEPS = [(di, dj) for di in (-2, -1, 0, 1, 2) for dj in (-2, -1, 0, 1, 2) if (di, dj) != (0, 0)]  # 24 neighbours


def lattice_edges(nr, nc, steps):
    ii, jj = np.divmod(np.arange(nr * nc), nc)
    rows, cols = [], []
    for di, dj in steps:
        ok = (ii + di >= 0) & (ii + di < nr) & (jj + dj >= 0) & (jj + dj < nc)
        rows.append(np.flatnonzero(ok))
        cols.append((ii[ok] + di) * nc + jj[ok] + dj)
    return np.concatenate(rows), np.concatenate(cols)


def wide_ell():
    """23 x 29 lattice, every site joined to the 24 others of the 5 x 5 block around it (queen, the rook moves of length 2,
    the knight moves and the diagonal moves of length 2): uniform ELL of width 24, no diagonal form."""
    r, c = lattice_edges(23, 29, WIDE_STEPS)
    return laplacian(23 * 29, r, c)


def one_isolated():
    """sell8 on 639 sites plus site 639 without a neighbour."""
    r, c = _ring_with_chords(639, 3 * 64 + 8 * np.arange(8) + 3, 5, 0)
    return laplacian(640, r, c)


def with_empty_slice(empty_slice, n=640, seed=2):
    """A sell8-type graph on n - 64 of n sites; the 64 sites of slice ``empty_slice`` have no neighbour.  The chords start in
    the first slice behind the empty one."""
    m = n - 64
    hub_slice = (empty_slice + 1) % (n // 64)
    site = _place(m, n, empty_slice)
    ring_of = np.full(n, -1)
    ring_of[site] = np.arange(m)
    r, c = _ring_with_chords(m, ring_of[hub_slice * 64 + 8 * np.arange(8) + 3], 5, seed)
    return laplacian(n, site[r], site[c])


def empty_first():
    return with_empty_slice(0)


def empty_middle():
    return with_empty_slice(4)


def empty_last():
    return with_empty_slice(9)


def two_components():
    """Two rings with chords, 320 sites each, no isolated site."""
    r0, c0 = _ring_with_chords(320, 64 + 8 * np.arange(8) + 3, 5, 4)
    r1, c1 = _ring_with_chords(320, 128 + 8 * np.arange(8) + 3, 5, 5)
    return laplacian(640, np.concatenate([r0, r1 + 320]), np.concatenate([c0, c1 + 320]))


def weighted_queen(nr=61, nc=67, seed=6):
    """``make_lattice_problem``'s queen lattice with every edge weight multiplied by a symmetric random factor in [0.5, 2] and
    the diagonal recomputed: ELL of width 8 without a diagonal form."""
    from occuspytial_amd.utils import rand_precision_mat
    Q = rand_precision_mat(nr, nc, max_neighbors=8).astype(float).tocoo()
    up = Q.row < Q.col
    factor = np.random.default_rng(seed).uniform(0.5, 2.0, int(up.sum()))
    return laplacian(nr * nc, Q.row[up], Q.col[up], -Q.data[up] * factor)


def sell_tiles(n=4400, empty_slice=30, seed=7):
    """True SELL bases at a size that fills 18 tiles of 256 sites (n is no multiple of 256): a ring on n - 64 sites in which
    every site also has a chord to a random partner ANYWHERE (most sites have a neighbour in another XCD's band of tiles)
    and 8 sites have 5 more (rows of at most 8 off-diagonals); the 64 sites of an inner slice have no neighbour."""
    m = n - 64
    site = _place(m, n, empty_slice)
    r, c = _ring_with_chords(m, 10 * 64 + 8 * np.arange(8) + 3, 5, seed, matching=True)
    return laplacian(n, site[r], site[c])


GRAPHS = dict(sell8=sell8, sell16=sell16, hub=hub, wide_ell=wide_ell, one_isolated=one_isolated, empty_last=empty_last,
              empty_first=empty_first, empty_middle=empty_middle)
EMPTY = ('empty_first', 'empty_middle', 'empty_last')
# the seed of each case's survey and start (test_layout_graphs_cpu.py holds the oracle's solve sensitivity at these seeds)
SEEDS = dict(sell8=3, sell16=3, hub=3, wide_ell=3, one_isolated=3, empty_last=3, empty_first=3, empty_middle=3, two_components=3,
             weighted_queen=3, sell_tiles=3)
_CACHE = {}


def graph(name):
    """The graph of a name (built once; treat as read-only)."""
    if name not in _CACHE:
        _CACHE[name] = {**GRAPHS, 'two_components': two_components, 'weighted_queen': weighted_queen, 'sell_tiles': sell_tiles}[name]()
    return _CACHE[name]


def isolated_sites(Q):
    return np.flatnonzero(np.diff(Q.indptr) == 0)


def residual(Q, tau, om, rhs, xz):
    """||[rhs; 1] - A xz|| / ||[rhs; 1]|| of the joint system A = blockdiag(tau Q + diag(omega))^2, in numpy"""
    n = Q.shape[0]
    A = tau * Q + sparse.diags(om)
    b = np.concatenate([rhs, np.ones(n)])
    return np.linalg.norm(b - np.concatenate([A @ xz[:n], A @ xz[n:]])) / np.linalg.norm(b)


def closed_form_deviation(Q, om, rhs, xz):
    """Largest distance of xz from x_i = rhs_i / omega_i, z_i = 1 / omega_i over the sites without neighbours, relative to the
    largest closed-form value of each half."""
    iso, n = isolated_sites(Q), Q.shape[0]
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    return max(rel(xz[iso], rhs[iso] / om[iso]), rel(xz[n + iso], 1.0 / om[iso]))


def survey(Q, seed):
    """A ``FlatProblem`` on Q: p = q = 2, ragged visits (1 to 3), one site in 20 never surveyed, some detections."""
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import _expit
    n = Q.shape[0]
    rng = np.random.default_rng(seed)
    alpha, beta = rng.standard_normal(2), rng.standard_normal(2)
    X = rng.uniform(-2, 2, (n, 2))
    X[:, 0] = 1
    z = rng.binomial(1, _expit(X @ beta))
    visits = rng.integers(1, 4, n)
    W, y = {}, {}
    for i in range(n):
        if i % 20 == 7:
            continue
        Wi = rng.uniform(-2, 2, (int(visits[i]), 2))
        Wi[:, 0] = 1
        W[i] = Wi
        y[i] = rng.binomial(1, z[i] * _expit(Wi @ alpha))
    prob = FlatProblem(Q, W, X, y)
    assert len(prob.not_surveyed) == len(range(7, n, 20)) and 0 < len(prob.obs) < prob.S
    return prob
