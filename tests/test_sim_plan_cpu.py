"""The host's part of the field simulator (occ_sim_plan.hpp) on the CPU, through the stand-alone program occ_sim_check.cpp
that `make sim_check` builds with g++ under AddressSanitizer and UBSan: the sign-and-root slots against numpy, the component
tables, ld and the tile counts, every refusal word for word -- and the symbols of include/occ_sim.h in the built library.
"""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import sparse

from . import _components_graphs as cg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')

# the refusals, word for word (tests/test_gpu_simulate.py matches the same texts through the C ABI)
REFUSALS = {
    'n': 'n must lie in [1, 2^30)',
    'b_max': 'b_max must lie in [1, 64]',
    'b': 'b must lie in [1, b_max]',
    'first': 'first + b must not exceed 2^32',
    'negative': 'first must not be negative',
    'tol': 'tol must lie in (0, 1)',
    'max_iter': 'max_iter must lie in [1, 2^31)',
    'check_every': 'check_every must be at least 1',
    'labels': 'labels must give two neighbouring sites the same component',
    'label range': 'component_id holds whole numbers from 0 to n - 1',
    'singular': 'Spatial precision matrix Q must be singular.',
    'columns': 'Q columns must be sorted, unique and in range',
}


def star(n=200):
    r, c = np.zeros(n - 1, dtype=int), np.arange(1, n)
    W = sparse.coo_matrix((np.ones(2 * (n - 1)), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n)).tocsr()
    return (sparse.diags(np.asarray(W.sum(axis=1)).ravel()) - W).tocsr()


@pytest.fixture(scope='module')
def sim_check():
    subprocess.run(['make', '-s', '-C', CSRC, 'sim_check'], check=True)
    exe = os.path.join(ROOT, 'build', 'occ_sim_check')

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])   # (a sanitizer report ends the program with a non-zero status)
        assert r.stderr == '', r.stderr[-2000:]
        return r.stdout.splitlines()
    return run


def plan_request(Q, labels, b_max, indices=None, data=None):
    Q = sparse.csr_matrix(Q).astype(np.float64)
    Q.sort_indices()
    ix = Q.indices if indices is None else indices
    qd = Q.data if data is None else data
    nums = lambda a: ' '.join(str(int(v)) for v in a)  # noqa: E731
    return 'plan %d %d %d\n%s\n%s\n%s\n%s\n' % (Q.shape[0], Q.nnz, b_max, nums(Q.indptr), nums(ix), ' '.join(repr(float(v)) for v in qd),
                                                nums(labels))


def parse_plan(lines):
    head = lines[0].split()
    assert head[0] == 'ok', lines[0]
    out = {'head': [int(v) for v in head[1:]], 'rows': {}}
    for ln in lines[1:]:
        if ln.startswith('row '):
            left, right = ln.split(':', 1)
            _, i, d, dinv = left.split()
            slots = [tuple(s.split()) for s in right.split(';') if s.strip()]
            out['rows'][int(i)] = (float(d), float(dinv), [(int(j), float(v), float(sr)) for j, v, sr in slots])
        else:
            name, *vals = ln.split()
            out[name] = np.array([int(v) for v in vals], dtype=np.int64)
    return out


GRAPHS = {'small': lambda: (cg.small()['Q'], cg.small()['labels']), 'large': lambda: (cg.large()['Q'], cg.large()['labels']),
          'star200': lambda: (star(), np.zeros(200, dtype=np.int32))}


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_slots_and_component_tables(sim_check, name):
    Q, labels = GRAPHS[name]()
    Q = sparse.csr_matrix(Q)
    Q.sort_indices()
    n = Q.shape[0]
    plan = parse_plan(sim_check(plan_request(Q, labels, 17)))
    ld, ntile, nslice, ell_w, k, nchunk = plan['head']
    assert (ld, ntile, nslice) == (32, -(-n // 256), -(-n // 64))
    assert k == len(set(labels.tolist()))
    if name == 'star200':
        assert ell_w == 0                                       # true SELL-64: slice 0 is 199 wide, the others 1
    else:
        assert ell_w == int(np.diff(Q.indptr).max()) - 1
    dense = Q.toarray()
    for i in range(n):
        d, dinv, slots = plan['rows'][i]
        assert d == dense[i, i] and dinv == (1.0 / dense[i, i] if dense[i, i] > 0 else 0.0)
        cols = [j for j in Q.indices[Q.indptr[i]:Q.indptr[i + 1]] if j != i]
        assert [s[0] for s in slots[:len(cols)]] == cols        # the row's off-diagonals in column order
        for (j, v, sr), jj in zip(slots, cols):
            w = -dense[i, jj]
            assert v == dense[i, jj]
            assert sr == (np.sqrt(w) if i < jj else -np.sqrt(w)) if w > 0 else sr == 0.0
        assert all(v == 0.0 and sr == 0.0 and 0 <= j < n for j, v, sr in slots[len(cols):])   # padding
    # every site is in exactly one component table: the list is a permutation, cut into chunks that tile it, and a chunk's
    # sites share one label
    lst, cs, cc, size = plan['list'], plan['chunk_start'], plan['comp_chunk'], plan['comp_size']
    assert sorted(lst.tolist()) == list(range(n))
    assert cs[0] == 0 and cs[-1] == n and np.all(np.diff(cs) >= 1) and np.all(np.diff(cs) <= 32) and len(cs) == nchunk + 1
    assert cc[0] == 0 and cc[-1] == nchunk and len(cc) == k + 1
    seen = np.zeros(n, dtype=int)
    for m in range(k):
        sites = lst[cs[cc[m]]:cs[cc[m + 1]]]
        seen[sites] += 1
        assert len(set(labels[sites].tolist())) == 1 and size[m] == len(sites) == int((labels == labels[sites[0]]).sum())
        assert np.all(np.diff(sites) > 0)
    assert np.all(seen == 1)


def test_ld_and_tile_counts(sim_check):
    req = ''.join('size %d %d\n' % (n, b) for n in (34, 64, 65, 256, 257) for b in (1, 16, 17, 64))
    got = iter(sim_check(req))
    for n in (34, 64, 65, 256, 257):
        for b in (1, 16, 17, 64):
            ld = {1: 16, 16: 16, 17: 32, 64: 64}[b]
            assert next(got).split() == ['size', str(ld), str(ld), str({34: 1, 64: 1, 65: 1, 256: 1, 257: 2}[n]),
                                         str({34: 1, 64: 1, 65: 2, 256: 4, 257: 5}[n])]


def test_refusals_word_for_word(sim_check):
    ask = lambda text: sim_check(text)[0]  # noqa: E731
    assert ask('create 0 16\n') == 'refused: ' + REFUSALS['n']
    assert ask('create %d 16\n' % 2 ** 30) == 'refused: ' + REFUSALS['n']
    assert ask('create 34 0\n') == 'refused: ' + REFUSALS['b_max'] == ask('create 34 65\n')
    assert ask('create 34 64\n') == 'ok'
    assert ask('draw 0 17 16\n') == 'refused: ' + REFUSALS['b'] == ask('draw 0 0 16\n')
    assert ask('draw %d 5 16\n' % (2 ** 32 - 4)) == 'refused: ' + REFUSALS['first']
    assert ask('draw %d 4 16\n' % (2 ** 32 - 4)) == 'ok'
    assert ask('draw -1 4 16\n') == 'refused: ' + REFUSALS['negative']
    assert ask('solve 0 10 16\n') == 'refused: ' + REFUSALS['tol'] == ask('solve 1 10 16\n')
    assert ask('solve 1e-10 0 16\n') == 'refused: ' + REFUSALS['max_iter']
    assert ask('solve 1e-10 10 0\n') == 'refused: ' + REFUSALS['check_every']
    assert ask('solve 1e-10 10 16\n') == 'ok'
    g = cg.small()
    Q = sparse.csr_matrix(g['Q'])
    Q.sort_indices()
    assert ask(plan_request(Q, np.zeros(34, dtype=int), 65)) == 'refused: ' + REFUSALS['b_max']
    assert ask(plan_request(Q, np.arange(34), 16)) == 'refused: ' + REFUSALS['labels']
    assert ask(plan_request(Q, np.full(34, 34), 16)) == 'refused: ' + REFUSALS['label range']
    assert ask(plan_request(Q, np.zeros(34, dtype=int), 16))[:2] == 'ok'      # (a coarser labelling joins no two neighbours wrongly)
    assert ask(plan_request(Q + sparse.identity(34), g['labels'], 16)) == 'refused: ' + REFUSALS['singular']
    assert ask(plan_request(Q, g['labels'], 16, data=-Q.data)).startswith('refused: Q must have non-positive off-diagonal entries')
    ix = Q.indices.copy()
    row = int(np.argmax(np.diff(Q.indptr)))                                   # the row's first column repeated in its second entry
    ix[Q.indptr[row] + 1] = ix[Q.indptr[row]]
    assert ask(plan_request(Q, g['labels'], 16, indices=ix)) == 'refused: ' + REFUSALS['columns']


def test_every_symbol_of_the_header_is_exported():
    """Every occ_sim_* that include/occ_sim.h declares is in the binding, with its argument count, and in the built library."""
    import ctypes

    from occuspytial_amd import _sim_lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'occ_sim.h')).read(), flags=re.S)
    declared = re.findall(r'\b(occ_sim_\w+)\s*\(', text)
    assert sorted(declared) == sorted(name for name, _, _ in _sim_lib.SYMBOLS) and len(set(declared)) == len(declared) == 8
    assert int(re.search(r'#define OCC_SIM_VERSION (\d+)', text).group(1)) == _sim_lib.VERSION
    assert int(re.search(r'#define OCC_SIM_MAX_B (\d+)', text).group(1)) == _sim_lib.MAX_B
    for name, _, argtypes in _sim_lib.SYMBOLS:
        args = re.search(r'\b%s\s*\(([^)]*)\)' % name, text).group(1).strip()
        assert (0 if args == 'void' else args.count(',') + 1) == len(argtypes), name
    assert _sim_lib.LIB_PATH == os.path.join(ROOT, 'occuspytial_amd', 'libocc_sim.so')
    assert os.path.exists(_sim_lib.LIB_PATH), 'run __graft_entry__.build()'
    lib = ctypes.CDLL(_sim_lib.LIB_PATH)
    for name, _, _ in _sim_lib.SYMBOLS:
        assert hasattr(lib, name), name
    assert _sim_lib.load().occ_sim_version() == _sim_lib.VERSION
    # a library of its own: the other two know nothing of it, and `make all` builds it
    assert 'occ_sim' not in open(os.path.join(ROOT, 'include', 'occ_gibbs.h')).read()
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    assert re.search(r'^all:.*\$\(OUT\).*\$\(BASIS_OUT\).*\$\(SIM_OUT\)', mk, flags=re.M)
    assert re.search(r'^\trm -f .*\$\(SIM_OUT\)', mk, flags=re.M)
