"""Cost of the per-component correction pass: us per iteration of occ_run under constraint='component' against
constraint='global' on the SAME disconnected graph -- two 100x50 queen lattices as one graph of 10 000 sites, 4 chains.

    python tools/component_time.py [--iters 2000] [--reps 5] [--warm 2000] [--out profiles/component_time.jsonl]

The mode belongs to a handle from before its first iteration, so each mode has an engine of its own (same keys, same start);
the two are timed alternately, `reps` times each, after `--warm` warm-up iterations (the first timed pass of a mode has
still come out slower than the rest: the line keeps every pass, the increase is the difference of the medians).  One JSON line is appended to --out.  The
difference is four launches per iteration (k_comp_part, k_comp_coef, k_comp_eta, k_beta_sums) and what they move: 16 B of Xv
and 4 B of the list per site, then Xv again, the labels and eta, then eta, omega_b, z and X for beta's partial sums."""
import argparse
import json
import os
import sys
import time

import numpy as np
from scipy import sparse

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(TOOLS), TOOLS]


def two_lattices(rows=100, cols=50, visits=5, seed=0):
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(rows, cols, visits=visits, p=2, q=2, random_state=seed)
    Q2, W2, X2, y2, *_ = make_lattice_problem(rows, cols, visits=visits, p=2, q=2, random_state=seed + 1)
    n = rows * cols
    W.update({s + n: w for s, w in W2.items()})
    y.update({s + n: v for s, v in y2.items()})
    return sparse.block_diag((Q, Q2), format='csr'), W, np.vstack([X, X2]), y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warm', type=int, default=2000)
    ap.add_argument('--chains', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(TOOLS), 'profiles', 'component_time.jsonl'))
    a = ap.parse_args()
    from occuspytial_amd._engine import Engine
    from occuspytial_amd._problem import FlatProblem, chain_generators, default_start
    Q, W, X, y = two_lattices()
    engines, stats = {}, {}
    for mode in ('global', 'component'):
        prob = FlatProblem(Q, W, X, y, constraint=mode)
        gens = chain_generators(10, a.chains)
        starts = [default_start(g, prob) for g in gens]
        eng = Engine(prob, [int(g.bit_generator.random_raw()) for g in gens])
        for c, st in enumerate(starts):
            eng.set_start(c, st['alpha'], st['beta'], st['tau'], st['eta'])
            eng.set('z', prob.z0, c)
        eng.run(a.warm, a.warm - 1)
        engines[mode] = eng
    times = {m: [] for m in engines}
    for _ in range(a.reps):
        for mode, eng in engines.items():
            t0 = time.perf_counter()
            eng.run(a.iters, a.iters - 1)
            times[mode].append((time.perf_counter() - t0) / a.iters * 1e6)
    for mode, eng in engines.items():
        stats[mode] = eng.stats()
        eng.close()
    line = dict(sites=int(Q.shape[0]), components=2, chains=a.chains, iters=a.iters,
                global_us=times['global'], component_us=times['component'],
                increase_us=float(np.median(times['component']) - np.median(times['global'])),
                persistent_solve=stats['component']['persistent_solve'], krylov_mean={m: stats[m]['krylov_mean'] for m in stats})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'a') as f:
        f.write(json.dumps(line) + '\n')
    print(json.dumps(line))


if __name__ == '__main__':
    main()
