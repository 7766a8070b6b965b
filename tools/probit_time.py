"""Iterations per second of ProbitRSRGibbs on one MI355X, 4 chains batched, at 40x50 (q = 100 basis columns) and
100x100 (the reference's threshold r = 0.5: 1 256 columns on this lattice), with LogitRSRGibbs at the same sizes for
comparison, and the per-kernel times of Engine.profile (``occ_profile``: each probit kernel in a captured graph of back-to-back launches).  One JSON line per
size.  Under ``rocprofv3 --kernel-trace --stats -- python tools/probit_time.py`` the kernel statistics of the same
runs land in rocprofv3's output directory (profiles/probit_* keeps them).

The bytes model: one iteration streams Phi (n x m doubles) twice -- k_pb_proj (u = Phi' s) and k_pb_eta (eta = Phi c) --
for all chains at once; everything else is O(n C + R C + m C).  ``phi_bound_us`` is that traffic at 5.3 TB/s (HBM;
Phi stays in the 256 MB MALL at both sizes, so the bound is loose)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_US = 5.3e6


def _timed(eng, iters, warm):
    eng.run(warm, warm - 1)
    t0 = time.perf_counter()
    eng.run(iters, iters - 1)
    return (time.perf_counter() - t0) / iters


def measure(rows, cols, q=None, r=0.5, chains=4, iters=400, warm=40, logit=True):
    from occuspytial_amd import LogitRSRGibbs, ProbitRSRGibbs
    from occuspytial_amd._engine import Engine
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(rows, cols, visits=3, p=3, q=2, random_state=0)
    out = {'shape': f'{rows}x{cols}', 'n': rows * cols, 'chains': chains}
    for name, cls in (('probit', ProbitRSRGibbs),) + ((('logit_rsr', LogitRSRGibbs),) if logit else ()):
        s = cls(Q, W, X, y, random_state=1, r=r, q=q)
        P = s._problem
        m = s.fixed.q
        eng = Engine(P, [101 + c for c in range(chains)], device=0)
        samplers = [s] + [s.copy() for _ in range(chains - 1)]
        for c, t in enumerate(samplers):
            t.__dict__['state'] = type(s.state)(**s.state.__dict__)
            t._initialize_posterior_state(None)
            eng.set_start(c, t.state.alpha, t.state.beta, t.state.tau, t.state.eta)
            if name == 'probit':
                eng.set('eps', t.state.eps, c)
            eng.set('z', P.z0, c)
        n_it = iters if name == 'probit' else max(iters // 8, 20)
        sec = _timed(eng, n_it, warm)
        out['m'] = m
        out[f'{name}_iter_us'] = 1e6 * sec
        out[f'{name}_iters_per_s'] = 1.0 / sec
        if name == 'probit':
            prof = eng.profile(50)
            out['probit_kernels_avg_us'] = {k: round(v['avg_us'], 2) for k, v in prof.items() if v['launches']}
            phi_bytes = 2 * P.n * m * 8
            out['phi_bound_us'] = phi_bytes / HBM_BYTES_PER_US
            out['phi_fraction_of_bound'] = out['phi_bound_us'] / out['probit_iter_us']
        eng.close()
    if logit:
        out['speedup_vs_logit_rsr'] = out['logit_rsr_iter_us'] / out['probit_iter_us']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=400)
    ap.add_argument('--no-logit', action='store_true')
    a = ap.parse_args()
    for rows, cols, q in ((40, 50, 100), (100, 100, None)):
        print(json.dumps(measure(rows, cols, q=q, iters=a.iters, logit=not a.no_logit)), flush=True)


if __name__ == '__main__':
    main()
