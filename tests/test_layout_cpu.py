"""The problem layout (occuspytial_amd/csrc/occ_layout.hpp) on the CPU: every array the host derives from the caller's
problem -- SELL-64 / ELL and diagonal form of Q, transposed designs, index sets, prior products -- against an independent
restatement in numpy, exactly; every refusal's message; and that a peer of a multi-GPU group sizes its arrays as the root's.
Each graph is chosen for a branch (GRAPHS).  Built with g++ on demand (`make plan`, occ_plan_capi.cpp), driven through ctypes."""
import ctypes as C
import glob
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')
NPRE = 8
ARRAYS = ('sell_ptr', 'sell_col', 'sell_val', 'qdiag', 'ell_w', 'dia_off', 'dia_val', 'dia_mask', 'Xt', 'Wt', 'yrow', 'row_site',
          'site_sidx', 'obs_site', 'hyp', 'wmax', 'row_t')
UPLOADED = ('sell_ptr', 'sell_col', 'sell_val', 'qdiag', 'dia_mask', 'Xt', 'Wt', 'yrow', 'row_site', 'site_sidx', 'site_ptr',
            'obs_site', 'hyp')  # create_impl's uploads of a layout: what a group broadcasts


@pytest.fixture(scope='module')
def lib():
    subprocess.run(['make', '-s', '-C', CSRC, 'plan'], check=True)
    lib = C.CDLL(os.path.join(ROOT, 'build', 'libocc_plan.so'))
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    lib.occ_layout_build.restype = C.c_void_p
    lib.occ_layout_build.argtypes = [C.c_int32] * 5 + [i32, i32, f64, C.c_int32, f64, i32, i32, f64, f64, f64, f64, f64, f64, C.c_char_p, C.c_int32]
    lib.occ_layout_peer.restype = C.c_void_p
    lib.occ_layout_peer.argtypes = [C.c_void_p]
    lib.occ_layout_free.argtypes = [C.c_void_p]
    lib.occ_layout_array.restype = C.c_int64
    lib.occ_layout_array.argtypes = [C.c_void_p, C.c_char_p, f64, C.c_int64]
    return lib


def arrays_of(lib, handle, names):
    out = {}
    for name in names:
        n = lib.occ_layout_array(handle, name.encode(), None, 0)
        assert n >= 0, name
        buf = np.zeros(max(n, 1))
        lib.occ_layout_array(handle, name.encode(), buf.ctypes.data_as(C.POINTER(C.c_double)), n)
        out[name] = buf[:n]
    return out


def layout(lib, pr, prior_factor=False, peer=False):
    """The engine's layout of problem `pr` (and, with peer, what a peer sizes from its header); ValueError: its refusal."""
    i32 = lambda a: np.ascontiguousarray(a, np.int32)
    f64 = lambda a: np.ascontiguousarray(a, np.float64)
    keep = [i32(pr['indptr']), i32(pr['indices']), f64(pr['data']), f64(pr['X']), i32(pr['site_id']), i32(pr['site_ptr']),
            f64(pr['W']), f64(pr['y']), f64(pr['a_mu']), f64(pr['a_prec']), f64(pr['b_mu']), f64(pr['b_prec'])]
    ptr = [a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double)) for a in keep]
    err = C.create_string_buffer(512)
    n, S, R = len(pr['indptr']) - 1, len(pr['site_id']), len(pr['y'])
    h = lib.occ_layout_build(n, S, R, pr['X'].shape[1], pr['W'].shape[1], ptr[0], ptr[1], ptr[2], int(prior_factor), *ptr[3:], err, 512)
    if not h:
        raise ValueError(err.value.decode())
    out = arrays_of(lib, h, ARRAYS)
    if peer:
        hp = lib.occ_layout_peer(h)
        out = (arrays_of(lib, h, UPLOADED + ('ell_w', 'dia_off', 'dia_val')), arrays_of(lib, hp, UPLOADED + ('ell_w', 'dia_off', 'dia_val')))
        lib.occ_layout_free(hp)
    lib.occ_layout_free(h)
    return out


def restate(pr):
    """Every array of the layout from the CSR input and the site arrays, in numpy."""
    indptr, indices, data = (np.asarray(pr[k]) for k in ('indptr', 'indices', 'data'))
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    off = indices != rows
    qdiag = np.zeros(n)
    qdiag[rows[~off]] = data[~off]
    r, c, v = rows[off], indices[off], data[off]  # the off-diagonals, in CSR column order
    cnt = np.bincount(r, minlength=n)
    nslice = -(-n // 64)
    width = np.array([cnt[s * 64:s * 64 + 64].max() for s in range(nslice)])
    wmax = int(width.max())
    ell = wmax > 0 and wmax * 64 * nslice <= math.floor(1.25 * 64 * width.sum()) + 64
    if ell:
        width[:] = wmax
    sell_ptr = np.concatenate([[0], 64 * np.cumsum(width)])
    sell_col, sell_val = np.zeros(sell_ptr[-1] + 64), np.zeros(sell_ptr[-1] + 64)  # 64 spare slots
    for s in range(nslice):  # padding: the lane's own row, or the last one
        sell_col[sell_ptr[s]:sell_ptr[s + 1]] = np.tile(np.minimum(s * 64 + np.arange(64), n - 1), width[s])
    pos = sell_ptr[r // 64] + 64 * (np.arange(len(r)) - np.repeat(np.cumsum(cnt) - cnt, cnt)) + r % 64
    sell_col[pos], sell_val[pos] = c, v
    offs = np.unique(c - r)  # sorted
    dia = 0 < len(offs) <= NPRE and all(len(np.unique(v[c - r == o])) == 1 for o in offs)
    dia_mask = np.zeros(n if dia else 0)
    for t, o in enumerate(offs if dia else []):
        dia_mask[r[c - r == o]] += 1 << t
    site_id, site_ptr, y = np.asarray(pr['site_id']), np.asarray(pr['site_ptr']), np.asarray(pr['y'])
    S, R = len(site_id), len(y)
    site_sidx = -np.ones(n)
    site_sidx[site_id] = np.arange(S)
    row_t = np.repeat(np.arange(S), np.diff(site_ptr))  # (no surveyed site: no row belongs to one)
    yrow, row_site, rt = np.zeros(R), np.zeros(R), np.zeros(R)
    yrow[:len(row_t)] = y[:len(row_t)] != 0
    obs_site = np.array([yrow[site_ptr[t]:site_ptr[t + 1]].any() for t in range(S)], dtype=float)
    row_site[:len(row_t)] = site_id[row_t] - 2.0 ** 31 * obs_site[row_t]  # bit 31 of an int
    rt[:len(row_t)] = row_t
    hyp = np.concatenate([pr['a_prec'].ravel(), pr['a_prec'] @ pr['a_mu'], pr['b_prec'].ravel(), pr['b_prec'] @ pr['b_mu']])
    return dict(sell_ptr=sell_ptr, sell_col=sell_col, sell_val=sell_val, qdiag=qdiag, ell_w=[wmax if ell else 0], wmax=[wmax],
                dia_off=offs if dia else [], dia_val=[v[c - r == o][0] for o in offs] if dia else [], dia_mask=dia_mask,
                Xt=pr['X'].T.ravel(), Wt=pr['W'].T.ravel(), yrow=yrow, row_site=row_site, site_sidx=site_sidx, obs_site=obs_site,
                hyp=hyp, row_t=rt)


def csr(A):
    """Q = D - A of a symmetric weight matrix, as CSR with the diagonal."""
    Q = np.diag(A.sum(1)) - A
    nz = Q != 0
    return dict(indptr=np.concatenate([[0], np.cumsum(nz.sum(1))]), indices=np.nonzero(nz)[1], data=Q[nz])


def lattice(nr, nc, steps):
    A = np.zeros((nr * nc, nr * nc))
    for i in range(nr):
        for j in range(nc):
            for di, dj in steps:
                if 0 <= i + di < nr and 0 <= j + dj < nc:
                    A[i * nc + j, (i + di) * nc + j + dj] = 1.0
    return A


ROOK = [(0, 1), (0, -1), (1, 0), (-1, 0)]
QUEEN = ROOK + [(1, 1), (1, -1), (-1, 1), (-1, -1)]


def queen9_one_heavy_edge():
    A = lattice(9, 9, QUEEN)
    A[40, 41] = A[41, 40] = 2.0
    return A


def star(n):
    A = np.zeros((n, n))
    A[0, 1:] = A[1:, 0] = 1.0
    return A


def ring(n):
    A = np.zeros((n, n))
    i = np.arange(n)
    A[i, (i + 1) % n] = A[(i + 1) % n, i] = 1.0
    return A


# name: (weights, n, slices, ELL width (0: true SELL bases), diagonals of the diagonal form (0: none))
GRAPHS = {
    'rook3x4': (lambda: lattice(3, 4, ROOK), 12, 1, 4, 4),           # one partial slice; mask bits missing at row ends
    'queen9x9': (lambda: lattice(9, 9, QUEEN), 81, 2, 8, NPRE),      # second slice partial; exactly NPRE diagonals
    'queen9x9_heavy_edge': (queen9_one_heavy_edge, 81, 2, 8, 0),     # same offsets, unequal values
    'queen6x6_rook2': (lambda: lattice(6, 6, QUEEN + [(0, 2), (0, -2), (2, 0), (-2, 0)]), 36, 1, 12, 0),  # 12 offsets > NPRE
    'star130': (lambda: star(130), 130, 3, 0, 0),                    # widths 129 / 1 / 1: 24 768 slots > 10 544
    'ring64': (lambda: ring(64), 64, 1, 2, 4),                       # the slice boundary, from below
    'ring65': (lambda: ring(65), 65, 2, 2, 4),                       # ... and from above
}


def problem(name, surveyed=True):
    """The graph with S < n shuffled surveyed sites, ragged visits (one site without a visit row) and some detections."""
    pr = csr(GRAPHS[name][0]())
    n = len(pr['indptr']) - 1
    rng = np.random.default_rng(n)
    S = (2 * n) // 3 if surveyed else 0
    visits = rng.integers(1, 4, S)
    visits[S // 2:S // 2 + 1] = 0
    R = int(visits.sum()) if surveyed else 3
    p, q = 3, 2
    dyadic = lambda *shape: rng.integers(-8, 9, shape) / 4.0  # products and sums exact, fused or not
    pr.update(site_id=rng.permutation(n)[:S], site_ptr=np.concatenate([[0], np.cumsum(visits)]), y=(rng.random(R) < 0.3).astype(float),
              X=rng.standard_normal((n, p)), W=rng.standard_normal((R, q)),
              a_mu=dyadic(q), a_prec=dyadic(q, q), b_mu=dyadic(p), b_prec=dyadic(p, p))
    return pr


@pytest.mark.parametrize('surveyed', [True, False], ids=['sites', 'S0'])
@pytest.mark.parametrize('name', list(GRAPHS))
def test_layout_equals_its_restatement(lib, name, surveyed):
    pr = problem(name, surveyed)
    got, want = layout(lib, pr), restate(pr)
    for a in ARRAYS:
        assert np.array_equal(got[a], np.asarray(want[a], dtype=float)), a
    _, n, nslice, ell_w, ndia = GRAPHS[name]
    assert (len(pr['indptr']) - 1, len(got['sell_ptr']) - 1, got['ell_w'][0], len(got['dia_off'])) == (n, nslice, ell_w, ndia)
    assert len(got['dia_val']) == ndia and len(got['dia_mask']) == (n if ndia else 0)
    if surveyed:
        assert got['obs_site'].any() and not got['obs_site'].all() and (np.diff(pr['site_ptr']) == 0).any()


def test_mask_bits_are_missing_at_row_ends(lib):
    got = layout(lib, problem('rook3x4'))
    assert list(got['dia_off']) == [-4, -1, 1, 4]
    assert list(got['dia_mask'][:5]) == [0b1100, 0b1110, 0b1110, 0b1010, 0b1101]


@pytest.mark.parametrize('name', list(GRAPHS))
def test_a_peer_sizes_its_arrays_as_the_root(lib, name):
    root, peer = layout(lib, problem(name), peer=True)
    for a in UPLOADED:
        assert len(peer[a]) == len(root[a]), a
    for a in ('ell_w', 'dia_off', 'dia_val', 'sell_ptr'):
        assert np.array_equal(peer[a], root[a]), a


def changed(pr, **over):
    out = dict(pr)
    for k, f in over.items():
        out[k] = np.array(pr[k], copy=True)
        f(out[k])
    return out


def _set(i, v):
    return lambda a: a.__setitem__(i, v)


SINGULAR = 'Spatial precision matrix Q must be singular.'
COLUMNS = 'Q columns must be sorted, unique and in range'
SITE_ID = r'site_id entries must be unique and in \[0, n\)'
# (rook3x4, row 0: columns 0 1 4; surveyed sites 8, visits 3 1 3 1 0 ...)
REFUSALS = [
    ('indptr_start', dict(indptr=_set(0, 1)), 'malformed Q indptr'),
    ('indptr_short', dict(indptr=_set(12, 11)), 'malformed Q indptr'),
    ('columns_unsorted', dict(indices=lambda a: a.__setitem__(slice(1, 3), [4, 1])), COLUMNS),
    ('columns_repeated', dict(indices=_set(2, 1)), COLUMNS),
    ('columns_out_of_range', dict(indices=_set(2, 12)), COLUMNS),
    ('positive_off_diagonal', dict(data=lambda a: a.__setitem__(slice(0, 3), [0.0, 1.0, -1.0])), 'Q must have non-positive off-diagonal entries'),
    ('row_sum', dict(data=_set(0, 2.5)), SINGULAR),
    ('all_zero', dict(data=lambda a: a.fill(0.0)), SINGULAR),
    ('site_id_repeated', dict(site_id=lambda a: a.__setitem__(1, a[0])), SITE_ID),
    ('site_id_out_of_range', dict(site_id=_set(1, 12)), SITE_ID),
    ('site_ptr_start', dict(site_ptr=_set(0, 1)), 'site_ptr does not span the rows'),
    ('site_ptr_end', dict(site_ptr=lambda a: a.__setitem__(-1, a[-1] - 1)), 'site_ptr does not span the rows'),
    ('site_ptr_decreasing', dict(site_ptr=lambda a: a.__setitem__(2, a[1] - 1)), 'site_ptr must be non-decreasing'),
]


@pytest.mark.parametrize('case,over,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(lib, case, over, message):
    with pytest.raises(ValueError, match='^' + message):
        layout(lib, changed(problem('rook3x4'), **over))


def test_a_prior_factor_lifts_the_sign_and_row_sum_checks(lib):
    pr = changed(problem('rook3x4'), data=lambda a: a.__setitem__(slice(0, 3), [0.0, 1.0, -1.0]))
    got, want = layout(lib, pr, prior_factor=True), restate(pr)
    for a in ARRAYS:
        assert np.array_equal(got[a], np.asarray(want[a], dtype=float)), a
    layout(lib, changed(problem('rook3x4'), data=_set(0, 2.5)), prior_factor=True)


# Which branch the Q of each golden fixture takes: (ELL width, diagonals).  What the GPU parity tests cover of the layout
# (the probit fixtures' Q is never laid out: that model reads its basis, not Q).
GOLDEN_BRANCHES = {
    'ref_graph300_weighted': (10, 0), 'ref_queen150_hparams': (8, 8), 'ref_queen150_ragged': (8, 8), 'ref_queen400_v3': (8, 8),
    'ref_rook400_v3': (4, 4), 'ref_rsr150_q10': (8, 8), 'ref_rsr150_r05': (8, 8),
}  # none reaches true SELL bases (ell_w = 0): the graphs of tests/_layout_graphs.py do (test_layout_graphs_cpu.py pins them)


def test_branches_of_the_golden_fixtures(lib):
    taken = {}
    for path in sorted(glob.glob(os.path.join(ROOT, 'tests', 'golden', 'ref_*.npz'))):
        name = os.path.basename(path)[:-4]
        if 'probit' in name:
            continue
        g = np.load(path)
        n = len(g['Q_indptr']) - 1
        one = np.ones((1, 1))
        got = layout(lib, dict(indptr=g['Q_indptr'], indices=g['Q_indices'], data=g['Q_data'], X=np.zeros((n, 1)), W=np.zeros((0, 1)),
                               y=np.zeros(0), site_id=np.zeros(0), site_ptr=np.zeros(1), a_mu=one[0], a_prec=one, b_mu=one[0], b_prec=one))
        taken[name] = (int(got['ell_w'][0]), len(got['dia_off']))
        print('%-24s n = %3d  %s  %s' % (name, n, 'ELL, width %d' % got['ell_w'][0] if got['ell_w'][0] else 'SELL (true bases)',
                                         'diagonal form, %d diagonals' % len(got['dia_off']) if len(got['dia_off']) else 'no diagonal form'))
    assert taken == GOLDEN_BRANCHES
