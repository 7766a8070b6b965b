"""Set-up time of the reduced-rank basis, host against device (recorded, not gated): appends to profiles/basis_time.jsonl.

    python tools/basis_time.py [--out profiles/basis_time.jsonl] [--skip-host-10000] [--cases 40x50,100x100,250x250]

Per case: the wall time of ``FlatProblem.enable_rsr`` with ``basis='host'`` and with ``basis='device'`` (the whole call: basis,
``K'QK`` and its eigenfactor), and for the device the driver's own account: outer rounds, applications of the operator, the
seconds inside the device primitives and inside the host's b x b ``cholesky`` / ``eigh``.  Then the Gram kernel alone: the
median of a few ``gram(0)`` calls at that case's final block, as TFLOP/s of the b (b + 16) n flops of its upper triangle of
tiles (the call includes the copy of the b x b result to the host, so this is a lower bound of the kernel's own rate; DESIGN
§10 measures ``k_rsr_gram32`` at 54 TFLOP/s by the kernel's time alone).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {'40x50': dict(rows=40, cols=50, q=100, r=None, host=True),
         '100x100': dict(rows=100, cols=100, q=None, r=0.5, host=True),
         '250x250': dict(rows=250, cols=250, q=1024, r=None, host=False)}


def gram_rate(Q, X, b, reps=5):
    from occuspytial_amd._basis_lib import DeviceBasisOps
    n = X.shape[0]
    ops = DeviceBasisOps(Q, X, b)
    ops.set_block(np.random.default_rng(0).standard_normal((n, b)))
    ops.gram(0)
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ops.gram(0)
        times.append(time.perf_counter() - t0)
    ops.close()
    bc = (b + 15) // 16 * 16
    sec = float(np.median(times))
    return {'gram_b': b, 'gram_seconds': sec, 'gram_tflops': bc * (bc + 16) * n / sec / 1e12}


def run_case(name, spec, host):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.basis import moran_basis
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(spec['rows'], spec['cols'], visits=1, p=2, q=2, random_state=0)
    prob = FlatProblem(Q, W, X, y)
    rec = {'case': name, 'n': prob.n, 'p': prob.p, 'q': spec['q'], 'r': spec['r']}
    kw = dict(q=spec['q']) if spec['q'] else dict(r=spec['r'])
    t0 = time.perf_counter()
    dev = prob.enable_rsr(basis='device', **kw)
    rec['device_seconds'] = time.perf_counter() - t0
    rec['m'] = dev['dim']
    _, info = moran_basis(prob.Q, prob.X, return_info=True, **kw)
    rec.update(outer=info['outer'], block=info['block'], applies=info['applies'], basis_seconds=info['seconds'],
               seconds_device_primitives=info['seconds_ops'], seconds_host_dense=info['seconds_dense'])
    rec.update(gram_rate(prob.Q, prob.X, info['block']))
    if host and spec['host']:
        t0 = time.perf_counter()
        h = prob.enable_rsr(basis='host', **kw)
        rec['host_seconds'] = time.perf_counter() - t0
        rec['host_m'] = h['dim']
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'basis_time.jsonl'))
    ap.add_argument('--cases', default='40x50,100x100,250x250')
    ap.add_argument('--skip-host-10000', action='store_true', help='do not time the dense host path at 100x100')
    a = ap.parse_args()
    for name in a.cases.split(','):
        spec = CASES[name]
        rec = run_case(name, spec, host=not (a.skip_host_10000 and name == '100x100'))
        line = json.dumps(rec)
        print(line, flush=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
