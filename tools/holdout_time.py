"""Cost of the held-out predictive scoring (state names holdout_*): us per iteration of occ_run with the switch on against the
switch off of the SAME build, at 100x100 x 4 chains (the headline workload) and 500x500 x 1 chain with 20 % of the sites
withheld (every fifth site is left out of the problem and held out with its five visits), in the manner of tools/conv_time.py.
Per size: 200 warm-up iterations, then 2 000 kept iterations timed in two modes -- ``off`` and ``holdout`` (holdout_stats on: one
more launch per kept iteration) -- alternating, three times each (a short re-warm after every flip: a flip drops the captured
graphs).  One JSON line per size, appended to --out (``last_count``: holdout_count of every chain after the last ``holdout``
pass, ``last_elpd``: the score those sums give).

Every size runs in a child process of its own under a time limit; a child that fails or runs out of time ends the tool with
its exit status, and nothing further is started on the device."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = ((100, 100, 4), (500, 500, 1))


def measure(rows, cols, chains, iters, warm, reps, every):
    import numpy as np
    from occuspytial_amd._engine import Engine
    from occuspytial_amd._problem import FlatProblem, chain_generators, default_start
    from occuspytial_amd.holdout import HoldoutScore
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(rows, cols, visits=5, p=2, q=2, random_state=0)
    held = list(range(0, rows * cols, every))
    Wt, yt = {s: W.pop(s) for s in held}, {s: y.pop(s) for s in held}
    prob = FlatProblem(Q, W, X, y)
    gens = chain_generators(10, chains)
    eng = Engine(prob, [int(g.bit_generator.random_raw()) for g in gens])
    for i, g in enumerate(gens):
        st = default_start(g, prob)
        eng.set_start(i, st['alpha'], st['beta'], st['tau'], st['eta'])
    eng.holdout_data(Wt, yt)
    eng.run(warm, warm - 1)
    modes = ('off', 'holdout')
    us = {mode: [] for mode in modes}
    last = None
    for _ in range(reps):
        for mode in modes:
            if mode == 'holdout' or eng._holdout_on:
                eng.holdout_stats(mode == 'holdout')
            eng.run(50, 49)
            t0 = time.perf_counter()
            eng.run(iters, 0)
            us[mode].append(1e6 * (time.perf_counter() - t0) / iters)
            if mode == 'holdout':
                last = HoldoutScore.from_engine(eng)
    st = eng.stats()
    out = {'shape': f'{rows}x{cols}', 'n': rows * cols, 'R': int(prob.R), 'chains': chains, 'iters': iters, 'held_out': len(held),
           'held_rows': int(sum(len(v) for v in yt.values())), 'sums_bytes': 40 * len(held) * chains, 'persistent_solve': st['persistent_solve'],
           'fused_fallbacks': st['fused_fallbacks'], 'last_count': last.n_draws.tolist(), 'last_elpd': float(last.elpd)}
    for mode in modes:
        out[mode + '_us'] = [round(v, 3) for v in us[mode]]
        out[mode + '_median_us'] = float(np.median(us[mode]))
    out['holdout_increase_us'] = out['holdout_median_us'] - out['off_median_us']
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=2000)
    ap.add_argument('--warm', type=int, default=200)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--every', type=int, default=5, help='every k-th site is withheld (5: 20 %%)')
    ap.add_argument('--limit', type=int, default=300, help='seconds per size')
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'holdout_time.jsonl'))
    ap.add_argument('--one', type=int, nargs=3, metavar=('ROWS', 'COLS', 'CHAINS'), help='(child) measure this size and print its line')
    a = ap.parse_args()
    if a.one:
        print(json.dumps(measure(*a.one, a.iters, a.warm, a.reps, a.every)), flush=True)
        return 0
    for rows, cols, chains in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), '--one', str(rows), str(cols), str(chains), '--iters', str(a.iters),
               '--warm', str(a.warm), '--reps', str(a.reps), '--every', str(a.every)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f'{rows}x{cols}: no result within {a.limit} s; stopping', file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f'{rows}x{cols}: exit status {r.returncode}; stopping', file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        line = r.stdout.strip().splitlines()[-1]
        json.loads(line)
        print(line, flush=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
