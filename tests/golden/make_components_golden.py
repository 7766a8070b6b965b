"""Writes tests/golden/components34.npz: the draws of the dense numpy restatement (tests/_components_reference.py) on the
34-site graph of tests/_components_graphs.py -- 2 chains of 3 000 iterations, the first 500 dropped -- under the
per-component constraints (alpha, beta, tau) and under the global one (tau alone: what the two settings must differ in).

    python -m tests.golden.make_components_golden        (from the repository root; about a minute)

Data only: tests/test_gpu_components.py compares the engine's posterior means with these, tests/test_components_cpu.py
checks that the two settings are as far apart in log tau as the GPU test needs.
"""
import os

import numpy as np

from .. import _components_graphs as G
from .. import _components_reference as R

SIZE, BURNIN, SEEDS = 3000, 500, (1, 2)
# tau ~ Gamma(A0, rate B0), so that tau | rest has the shape A0 + rank(Q) / 2: n - k under 'component', n - 1 under 'global'.
# (Under the package's default Gamma(0.5, 0.005) the posterior of log tau on 34 Bernoulli sites has an exponential left tail --
# the likelihood does not bound eta as tau -> 0 -- and chains of 3 000 iterations do not pin its mean: the restatement's own
# chain means ranged from -6.5 to 4.0 over six seeds.  With Gamma(5, 1) four seeds agree within 0.04.)
A0, B0 = 5.0, 1.0


def main():
    g = G.small()
    n, k = g['n'], g['k']
    comp = [R.run_chain(g, 'component', SIZE, seed, tau_shape=A0 + 0.5 * (n - k), tau_rate=B0) for seed in SEEDS]
    glob = [R.run_chain(g, 'global', SIZE, seed + 10, tau_shape=A0 + 0.5 * (n - 1), tau_rate=B0) for seed in SEEDS]
    out = dict(alpha=np.stack([c[0][BURNIN:] for c in comp]), beta=np.stack([c[1][BURNIN:] for c in comp]),
               tau=np.stack([c[2][BURNIN:] for c in comp]), global_tau=np.stack([c[2][BURNIN:] for c in glob]),
               size=np.int64(SIZE), burnin=np.int64(BURNIN), tau_shape=np.float64(A0 + 0.5 * (n - k)), tau_rate=np.float64(B0))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'components34.npz'), **out)
    lt, lg = np.log(out['tau']), np.log(out['global_tau'])
    print('log tau: component %.4f (mcse %.4f), global %.4f (mcse %.4f)' % (lt.mean(), R.batch_means_mcse(lt), lg.mean(), R.batch_means_mcse(lg)))


if __name__ == '__main__':
    main()
