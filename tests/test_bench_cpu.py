"""bench.py's N > 1 control flow, rehearsed on CPU before the first 8-GPU run (reference ``gibbs/parallel.py:20-41`` fans the
chains out one process each; ``base.py:293-306`` gives chain k its own generator): 8 plain processes, one per "GPU", find each
other through RANK / WORLD_SIZE / MASTER_PORT and the product's file rendezvous, rank 0 generates the problem and the others
receive it, every rank runs the metric's 4 chains (the weak-scaling line: 32 chains), then the metric's literal 4 chains are
split over the 8 ranks -- ranks 4 to 7 own nothing and still take part in every collective.  The compute backend is the CPU
restatement behind the engine's own C ABI (``tests/_bench_worker.py``).  Asserted: ONE JSON line, on rank 0; eight ranks seen;
every chain's draws equal those of a single process running the same chains."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from .conftest import ROOT
from .test_cpu_abi import ABI_LIB, cpu_abi  # noqa: F401  (fixture)

ARGS = ['--lattice', '9', '10', '--visits', '3', '--steps', '7', '--warmup', '3', '--no-cpu-baseline']


def _launch(world, port, extra=()):
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   PYTHONPATH=ROOT, OMP_NUM_THREADS='1', OPENBLAS_NUM_THREADS='1', MKL_NUM_THREADS='1')
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', '_bench_worker.py'), '--gpus', str(world)] + ARGS + list(extra),
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = []
    for p in procs:
        out, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
        outs.append(out)
    return outs


def _single_process_last_draws(n_chains, warmup=3, steps=7, state=None):
    """The same chains in ONE batch of one process: bench.py's seeding rule (chain c owns the c-th generator of seed 10:
    start values first, then its Philox key).  `state`: a dict that receives eta and z of every chain after the run."""
    from occuspytial_amd._engine import Engine
    from occuspytial_amd._problem import FlatProblem, chain_generators, default_start
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(9, 10, visits=3, p=2, q=2, random_state=0)
    prob = FlatProblem(Q, W, X, y)
    gens = chain_generators(10, n_chains)
    starts = [default_start(g, prob) for g in gens]
    eng = Engine(prob, [int(g.bit_generator.random_raw()) for g in gens])
    for c, st in enumerate(starts):
        eng.set_start(c, st['alpha'], st['beta'], st['tau'], st['eta'])
    eng.run(warmup, warmup - 1)
    a, b, t = eng.run(steps, 0)
    if state is not None:
        for name in ('eta', 'z'):
            state[name] = np.stack([eng.get(name, c) for c in range(n_chains)])
    eng.close()
    return [np.concatenate([a[c, -1], b[c, -1], t[c, -1:]]) for c in range(n_chains)]


def _check_dump(path, draws, state):
    """bench.py --dump-outputs: float64 files, chains in global order, equal to the same chains run in one process."""
    got = {name: np.load(os.path.join(path, name + '.npy')) for name in ('alpha', 'beta', 'tau', 'eta', 'z')}
    assert all(a.dtype == np.float64 for a in got.values())
    rows = np.array(draws)
    assert np.array_equal(got['alpha'], rows[:, :2]) and np.array_equal(got['beta'], rows[:, 2:4]) and np.array_equal(got['tau'], rows[:, 4])
    assert np.array_equal(got['eta'], state['eta']) and np.array_equal(got['z'], state['z'])
    assert got['eta'].shape == (len(draws), 90)


def test_eight_ranks_run_bench_py_and_agree_with_one_process(cpu_abi, tmp_path):  # noqa: F811
    outs = _launch(8, 29671, ['--full', '--dump-outputs', str(tmp_path)])
    lines = [ln for ln in outs[0].splitlines() if ln.strip()]
    assert len(lines) == 1, outs[0][-2000:]                       # ONE line, on rank 0 ...
    assert all(not o.strip() for o in outs[1:])                   # ... and nothing on the other ranks' stdout
    d = json.loads(lines[0])
    assert d['n_gpus'] == 8 and d['steps'] == 7 and d['warmup'] == 3 and d['scaling'] == 'weak' and d['value'] > 0
    assert d['metric'].startswith('Gibbs iterations/sec') and d['unit'] == 'iterations/s'
    assert d['config']['total_chains'] == 32 and d['config']['chains_per_gpu'] == 4
    assert abs(d['value'] - 32 * 7 / (d['ms_per_step'] * 7e-3)) < 1e-6 * d['value']
    assert abs(d['value_per_gpu'] * 8 - d['value']) < 1e-9 * d['value']
    r = d['ranks']
    assert r['ranks_seen_by_file_rendezvous'] == 8 and len(r['members']) == 8, r
    assert sorted(m['rank'] for m in r['members']) == list(range(8)) and all(m['chains'] == 4 for m in r['members'])
    assert 'file rendezvous' in r['communicator']
    # the weak line: 32 chains, chain c on rank c // 4 -- the draws of a single process running all 32
    state = {}
    want = _single_process_last_draws(32, state=state)
    _check_dump(tmp_path, want, state)
    assert len(d['last_draws']) == 32
    for c in range(32):
        assert np.array_equal(np.asarray(d['last_draws'][c]), want[c]), c
    # the metric's 4 chains split over 8 ranks: ranks 4-7 are empty and everybody still arrives
    s = d['split_4_chains']
    assert s['chains_per_gpu'] == [1, 1, 1, 1, 0, 0, 0, 0] and s['total_chains'] == 4 and s['scaling'] == 'strong' and s['value'] > 0
    want4 = _single_process_last_draws(4)
    assert len(s['last_draws']) == 4
    for c in range(4):
        assert np.array_equal(np.asarray(s['last_draws'][c]), want4[c]), c


def test_one_rank_line_has_the_same_chains(cpu_abi, tmp_path):  # noqa: F811
    """The N = 1 line of the same workload carries the draws the 8-rank line's first four chains carry (same seed rule).
    A plain run is lean: no roofline pass, no CPU baseline; --dump-outputs writes the last step's outputs."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_bench_worker.py')] + ARGS + ['--dump-outputs', str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['n_gpus'] == 1 and 'ranks' not in d and 'split_4_chains' not in d and d['vs_baseline'] is None
    assert 'roofline' not in d and 'cpu_baseline' not in d
    assert d['steps'] == 7 and abs(d['value'] - 4 * 7 / (d['ms_per_step'] * 7e-3)) < 1e-6 * d['value']
    state = {}
    want = _single_process_last_draws(4, state=state)
    for c in range(4):
        assert np.array_equal(np.asarray(d['last_draws'][c]), want[c])
    _check_dump(tmp_path, want, state)


def test_one_rank_full_line_adds_the_roofline(cpu_abi):  # noqa: F811
    """--full on one rank: the roofline pass runs after the timed region and the timed chains are unchanged by it."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK'):
        env.pop(k, None)
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_bench_worker.py')] + ARGS + ['--full'], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d['roofline']['bound'] == 'hbm' and d['roofline']['peak'] > 0 and 'cpu_baseline' not in d
    want = _single_process_last_draws(4)
    for c in range(4):
        assert np.array_equal(np.asarray(d['last_draws'][c]), want[c])
