"""Disconnected test graphs of the per-component sum-to-zero constraint (tests/test_components_cpu.py,
tests/test_gpu_components.py), built here from nothing but numpy.

``small()``: a 5x4 rook lattice, a 3x3 queen lattice, a weighted path of 3 sites and two singleton sites, one surveyed and
one not -- n = 34, k = 5.  ``heavy()``: a 53x49 rook lattice with two islands, whose mainland takes the second level's wave
branch.  ``large()``: a 19x17 rook lattice (323 sites), a 6x6 queen lattice and one singleton -- n = 360,
k = 3; its components cross the 64-site slices and the 256-site tiles of the solve, and its rows have at most 8 neighbours,
so the tile form can be forced.  Site numbers are permuted: no component is contiguous.  Two chains' worth of data: p = q = 2,
two or three ragged visits.
"""
import numpy as np
from scipy import sparse


def lattice_edges(rows, cols, queen):
    idx = np.arange(rows * cols).reshape(rows, cols)
    e = [(idx[:, :-1], idx[:, 1:]), (idx[:-1, :], idx[1:, :])]
    if queen:
        e += [(idx[:-1, :-1], idx[1:, 1:]), (idx[:-1, 1:], idx[1:, :-1])]
    return [(int(a), int(b), 1.0) for u, v in e for a, b in zip(u.ravel(), v.ravel())]


def assemble(blocks, seed):
    """blocks: (number of sites, [(a, b, weight)]) per component, in local numbers.  -> Q (csr, permuted), the component of
    every permuted site numbered in the order of `blocks`, and the permutation (new number of every old site)."""
    n = sum(m for m, _ in blocks)
    perm = np.random.default_rng(seed).permutation(n)
    W = np.zeros((n, n))
    comp = np.zeros(n, dtype=np.int64)
    base = 0
    for c, (m, edges) in enumerate(blocks):
        comp[perm[base:base + m]] = c
        for a, b, w in edges:
            i, j = perm[base + a], perm[base + b]
            W[i, j] = W[j, i] = w
        base += m
    Q = np.diag(W.sum(axis=1)) - W
    return sparse.csr_matrix(Q), comp, perm


def lowest_site_labels(comp):
    """`comp` renumbered by each component's lowest site: what graph.components must return."""
    order = sorted(set(comp.tolist()), key=lambda c: int(np.flatnonzero(comp == c)[0]))
    rank = {c: r for r, c in enumerate(order)}
    return np.array([rank[c] for c in comp.tolist()], dtype=np.int32)


def survey(n, surveyed, seed, alpha=(0.4, 0.8), beta=(0.3, -0.6), visits=(2, 3)):
    """X (n x 2), W and y dicts over `surveyed` with ragged visits, simulated from a plain occupancy model."""
    rng = np.random.default_rng(seed)
    X = np.column_stack([np.ones(n), rng.standard_normal(n)])
    psi = 1.0 / (1.0 + np.exp(-(X @ np.asarray(beta))))
    z = rng.random(n) < psi
    W, y = {}, {}
    for s in surveyed:
        v = int(rng.integers(visits[0], visits[1] + 1))
        Ws = np.column_stack([np.ones(v), rng.standard_normal(v)])
        pdet = 1.0 / (1.0 + np.exp(-(Ws @ np.asarray(alpha))))
        W[int(s)] = Ws
        y[int(s)] = ((rng.random(v) < pdet) & z[s]).astype(np.float64)
    return X, W, y


def small():
    """-> dict(Q, comp, labels, k, X, W, y, singles=(surveyed singleton, unsurveyed singleton))"""
    blocks = [(20, lattice_edges(5, 4, False)), (9, lattice_edges(3, 3, True)), (3, [(0, 1, 0.5), (1, 2, 2.0)]), (1, []), (1, [])]
    Q, comp, perm = assemble(blocks, seed=34)
    n = 34
    rng = np.random.default_rng(341)
    in_c = lambda c: np.flatnonzero(comp == c)
    # 14 of the rook lattice's 20 sites, 2 of the queen lattice's 9, none of the path's, the first singleton
    surveyed = np.concatenate([rng.choice(in_c(0), 14, replace=False), rng.choice(in_c(1), 2, replace=False), in_c(3)])
    surveyed = np.sort(surveyed)
    X, W, y = survey(n, surveyed, seed=342)
    return dict(Q=Q, comp=comp, labels=lowest_site_labels(comp), k=5, X=X, W=W, y=y, n=n,
                singles=(int(in_c(3)[0]), int(in_c(4)[0])))


def large():
    blocks = [(323, lattice_edges(19, 17, False)), (36, lattice_edges(6, 6, True)), (1, [])]
    Q, comp, perm = assemble(blocks, seed=360)
    n = 360
    rng = np.random.default_rng(3601)
    surveyed = np.sort(rng.choice(n, 200, replace=False))
    X, W, y = survey(n, surveyed, seed=3602)
    single = int(np.flatnonzero(comp == 2)[0])
    return dict(Q=Q, comp=comp, labels=lowest_site_labels(comp), k=3, X=X, W=W, y=y, n=n, singles=(single,))


def connected(rows=6, cols=6):
    """A connected rook lattice with data: one component."""
    Q, comp, perm = assemble([(rows * cols, lattice_edges(rows, cols, False))], seed=66)
    n = rows * cols
    surveyed = np.sort(np.random.default_rng(661).choice(n, 24, replace=False))
    X, W, y = survey(n, surveyed, seed=662)
    return dict(Q=Q, comp=comp, labels=np.zeros(n, dtype=np.int32), k=1, X=X, W=W, y=y, n=n, singles=())


def heavy():
    """A mainland and two islands: a 53x49 rook lattice (2 597 sites: 82 chunks of 32, more than the 64 a single thread adds
    at the second level, so one WAVE adds them), a 3x3 queen lattice and one singleton -- n = 2 607, k = 3, permuted."""
    blocks = [(2597, lattice_edges(53, 49, False)), (9, lattice_edges(3, 3, True)), (1, [])]
    Q, comp, perm = assemble(blocks, seed=2607)
    n = 2607
    surveyed = np.sort(np.random.default_rng(26071).choice(n, 1200, replace=False))
    X, W, y = survey(n, surveyed, seed=26072)
    single = int(np.flatnonzero(comp == 2)[0])
    return dict(Q=Q, comp=comp, labels=lowest_site_labels(comp), k=3, X=X, W=W, y=y, n=n, singles=(single,))


def wave_sum(v):
    """The engine's wave sum of 64 lane values, addition by addition (occ_state.hpp: wave_sum): inside a quad (l0 + l1) +
    (l2 + l3); the quads of a row of 16 by pairs, then the pairs; the rows (R0 + R1) and (R2 + R3), then their sum."""
    v = [float(t) for t in v]
    assert len(v) == 64
    rows = []
    for r in range(4):
        q = [(v[16 * r + 4 * j] + v[16 * r + 4 * j + 1]) + (v[16 * r + 4 * j + 2] + v[16 * r + 4 * j + 3]) for j in range(4)]
        rows.append((q[0] + q[1]) + (q[2] + q[3]))
    return (rows[0] + rows[1]) + (rows[2] + rows[3])


def component_sums(xz, labels):
    """(sum x, sum z) of every component in float64, in the engine's documented order (occ_comp_plan.hpp): chunks of 32 sites in
    ascending site order, each summed left to right from 0.0; then, for at most 64 chunks, the chunks left to right from 0.0;
    for more, lane l of a wave adds the chunks l, l + 64, ... from 0.0 and the 64 lanes are added by wave_sum."""
    n = labels.size
    x, z = xz[:n], xz[n:]
    out = {}
    for c in np.unique(labels):
        sites = np.flatnonzero(labels == c)
        chunks = []
        for b in range(0, sites.size, 32):
            cx = cz = 0.0
            for i in sites[b:b + 32]:
                cx += x[i]
                cz += z[i]
            chunks.append((cx, cz))
        if len(chunks) <= 64:
            sx = sz = 0.0
            for cx, cz in chunks:
                sx += cx
                sz += cz
        else:
            lx, lz = [0.0] * 64, [0.0] * 64
            for j, (cx, cz) in enumerate(chunks):   # (ascending j: lane j % 64 adds its chunks in turn)
                lx[j % 64] += cx
                lz[j % 64] += cz
            sx, sz = wave_sum(lx), wave_sum(lz)
        out[int(c)] = (sx, sz)
    return out
