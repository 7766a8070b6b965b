"""Wall time of the field simulator's solve (libocc_sim.so: x = Q^+ u by conjugate gradients) per batch and per iteration, on
100x100 and 500x500 queen lattices at b = 16 and 64 columns, beside the host alternatives on the same right-hand sides.

    python tools/sim_time.py [--reps 3] [--host-columns 2] [--dense-max-n 10000] [--dense-limit 1800] [--out profiles/sim_time.jsonl]

Per (size, b), in a child process of its own under a time limit: one handle, one draw (timed), one warm-up solve, then --reps
solves of the same right-hand sides timed with a host clock -- a solve ends in a wait for the handle's stream, so the clock
covers the device's work; per iteration = that time over the iterations of the slowest column (the launches go on until every
column is done).  The host alternatives: scipy.sparse.linalg.cg with the same Jacobi preconditioner, start and tolerance on
--host-columns of the device's own right-hand sides, one after the other (its time per column, times b, is what the batch would
take); and, once per size where n <= --dense-max-n, the dense path of utils.make_data -- pinvh(Q) and one eigh-based
multivariate normal draw -- which needs an n x n array.  One JSON line per child, appended to --out.

A child that fails or runs out of time ends the tool with its exit status, and nothing further is started on the device."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(TOOLS), TOOLS]

SIZES = ((100, 100), (500, 500))
BATCHES = (16, 64)
KEY = 0x1234ABCD5678EF01
TOL = 1e-10


def lattice(rows, cols):
    from scipy import sparse

    from occuspytial_amd.utils import rand_precision_mat
    return sparse.csr_matrix(rand_precision_mat(rows, cols)).astype(float)


def measure(rows, cols, b, reps, host_columns):
    from scipy import sparse
    from scipy.sparse.linalg import cg

    from occuspytial_amd._sim_lib import DeviceFieldOps
    Q = lattice(rows, cols)
    n = rows * cols
    t0 = time.perf_counter()
    ops = DeviceFieldOps(Q, np.zeros(n, dtype=np.int32), b)
    create_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ops.draw(KEY, 0, b)
    draw_first_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ops.draw(KEY, 0, b)
    draw_s = time.perf_counter() - t0
    info = ops.solve(tol=TOL)                                  # warm-up: the first launches load the code object
    solve_s = []
    for _ in range(reps):
        t0 = time.perf_counter()
        info = ops.solve(tol=TOL)
        solve_s.append(time.perf_counter() - t0)
    U, X = ops.get(1), ops.get(0)
    ops.close()
    iters = int(info['iterations'].max())
    med = float(np.median(solve_s))
    line = {'shape': f'{rows}x{cols}', 'n': n, 'b': b, 'tol': TOL, 'create_s': round(create_s, 4), 'draw_first_s': round(draw_first_s, 5),
            'draw_s': round(draw_s, 5), 'solve_s': [round(v, 5) for v in solve_s], 'solve_median_s': med,
            'iterations_min': int(info['iterations'].min()), 'iterations_max': iters, 'us_per_iteration': 1e6 * med / iters,
            'ms_per_draw': 1e3 * med / b, 'residual_max': float(info['residual'].max())}
    # the host: scipy's CG, Jacobi-preconditioned, from 0, to the same relative residual, on the device's own right-hand sides
    d = Q.diagonal()
    M = sparse.diags(1.0 / d)
    host_s, host_it, host_diff = [], [], []
    for c in range(min(host_columns, b)):
        count = [0]
        t0 = time.perf_counter()
        x, code = cg(Q, U[:, c], rtol=TOL, atol=0.0, maxiter=4 * n + 100, M=M, callback=lambda _: count.__setitem__(0, count[0] + 1))
        host_s.append(time.perf_counter() - t0)
        host_it.append(count[0])
        x -= x.mean()
        host_diff.append(float(np.linalg.norm(x - X[:, c]) / np.linalg.norm(X[:, c])) if code == 0 else None)
    hmed = float(np.median(host_s))
    line.update({'scipy_cg_s_per_column': [round(v, 4) for v in host_s], 'scipy_cg_iterations': host_it, 'scipy_cg_batch_s': hmed * b,
                 'scipy_cg_over_device': hmed * b / med, 'scipy_cg_relative_difference': host_diff, 'host_threads': os.environ.get('OMP_NUM_THREADS')})
    return line


def measure_dense(rows, cols):
    """The dense path of utils.make_data at this size: pinvh(Q) once, then one draw by the eigh-based multivariate normal."""
    from scipy.linalg import pinvh
    Q = lattice(rows, cols)
    n = rows * cols
    t0 = time.perf_counter()
    cov = pinvh(Q.toarray(), rtol=1e-5)
    pinvh_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    np.random.default_rng(0).multivariate_normal(np.zeros(n), cov, method='eigh')
    draw_s = time.perf_counter() - t0
    return {'shape': f'{rows}x{cols}', 'n': n, 'dense': True, 'pinvh_s': round(pinvh_s, 3), 'first_draw_s': round(draw_s, 3),
            'array_bytes': 8 * n * n, 'host_threads': os.environ.get('OMP_NUM_THREADS')}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--host-columns', type=int, default=2)
    ap.add_argument('--dense-max-n', type=int, default=10000)
    ap.add_argument('--limit', type=int, default=300, help='seconds per child')
    ap.add_argument('--dense-limit', type=int, default=1800, help='seconds for the dense path (host only: two n x n eigendecompositions)')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(TOOLS), 'profiles', 'sim_time.jsonl'))
    ap.add_argument('--one', type=int, nargs=3, metavar=('ROWS', 'COLS', 'B'), help='(child) measure this size and print its line; B = 0: the dense path')
    a = ap.parse_args(argv)
    if a.one:
        rows, cols, b = a.one
        print(json.dumps(measure(rows, cols, b, a.reps, a.host_columns) if b else measure_dense(rows, cols)), flush=True)
        return 0
    jobs = [(r, c, b) for r, c in SIZES for b in BATCHES] + [(r, c, 0) for r, c in SIZES if r * c <= a.dense_max_n]
    for rows, cols, b in jobs:
        cmd = [sys.executable, os.path.abspath(__file__), '--one', str(rows), str(cols), str(b), '--reps', str(a.reps), '--host-columns',
               str(a.host_columns)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit if b else a.dense_limit)
        except subprocess.TimeoutExpired:
            print(f'{rows}x{cols} b={b}: no result within {a.limit if b else a.dense_limit} s; stopping', file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f'{rows}x{cols} b={b}: exit status {r.returncode}; stopping', file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        line = r.stdout.strip().splitlines()[-1]
        json.loads(line)
        print(line, flush=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
