"""The z update's four optional outputs beside each other while their switches come and go.

One word on the handle, the OR of the chains' switches, decides which kernel family stands where ``k_z_ob`` stands.  What
that can get wrong is a switch going off while a higher or a lower one stays on: the family must follow the highest switch
still on, an output below it must go on being served and one above it must stop.  Every comparison is between two ways of
running the engine on the same keys and starts, so every comparison is equality.  Workloads: the ICAR model on an 18x15
lattice (270 sites: two workgroups of 256, five slices of 64, no multiple of either) with two covariates of each kind; the
generic kernels on the 17x19 lattice of ``test_gpu_ppc.py`` with nine; the probit handle, which has ``region_stats`` alone.
"""
import signal

import numpy as np
import pytest

from ._outputs_gpu import engine_with
from .test_gpu_parity import KEY, _random_start
from .test_gpu_regions import _ids, _probit_problem
from .test_gpu_site_summaries import _workload_g

pytestmark = pytest.mark.gpu
STATE = ('alpha', 'beta', 'tau', 'z', 'eta')
OUTPUTS = ('site', 'll', 'region', 'ppc')   # in the order of their levels, 1 to 4


@pytest.fixture(autouse=True)
def _time_limit():
    """120 s per test (each takes a few seconds)."""
    def late(signum, frame):
        raise TimeoutError('a test of test_gpu_outputs.py ran past its time limit')
    old = signal.signal(signal.SIGALRM, late)
    signal.alarm(120)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def _probit_engine(prob, keys, starts, ids=None, on=True):
    return engine_with(prob, keys, starts, ids=ids, region_on=on)


def _icar():
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(18, 15, visits=3, p=2, q=2, random_state=21)
    prob = FlatProblem(Q, W, X, y)
    return prob, [KEY + 13 * c for c in range(2)], [_random_start(prob, 40 + c) for c in range(2)]


def _generic():
    prob, keys, starts = _workload_g()
    rng = np.random.default_rng(19)
    second = dict(alpha=0.3 * rng.standard_normal(9), beta=0.3 * rng.standard_normal(9), tau=0.8,
                  eta=(lambda e: e - e.mean())(rng.standard_normal(prob.n)))
    return prob, [keys[0], keys[0] + 5], [starts[0], second]


def _switch(eng, name, on):
    {'site': eng.site_stats, 'll': eng.loglik_stats, 'region': eng.region_stats, 'ppc': eng.ppc_stats}[name](on)


def _answer(eng, name, chain):
    """What the handle says about one output of one chain now: its sums or rows, or the text of its refusal."""
    try:
        if name == 'site':
            return eng.site_sums(chain)
        if name == 'll':
            return eng.loglik_sums(chain)
        return eng.region_draws(chain) if name == 'region' else eng.ppc_draws(chain)
    except ValueError as e:
        return str(e)


def _equal(a, b):
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray) and isinstance(b, np.ndarray):
        return a.shape == b.shape and np.array_equal(a, b)
    return isinstance(a, str) and a == b


# before call k (0-based) these switches are flipped, in this order -> the levels 0, 1, 2, 3, 4, 2, 0.  On the way down the
# LOWER switch of each pair goes off first, so a higher one stays on while it does (the family must not change), and then
# the higher one goes off while the two lowest stay on (the family must fall to theirs).
WALK = [(), (('site', True),), (('ll', True),), (('region', True),), (('ppc', True),),
        (('region', False), ('ppc', False)), (('site', False), ('ll', False))]
ON_DURING = {'site': (1, 2, 3, 4, 5), 'll': (2, 3, 4, 5), 'region': (3, 4), 'ppc': (4,)}


@pytest.mark.parametrize('workload', ['icar', 'generic'])
def test_outputs_switched_on_and_off_beside_each_other(workload):
    """Seven run(6, 0) calls.  `walk` switches the outputs on one after the other and off again; `never` switches nothing;
    only[x] has output x alone, on for the calls `walk` has it on.  After every call the draws and alpha, beta, tau, z, eta
    of all six engines are bit-equal, and `walk` answers for every output and chain what only[x] answers -- the sums or rows
    while on, and while off what a handle with that output alone gives: a refusal before the first switch-on, readable
    sums afterwards, (0, G) and (0, 4) rows."""
    prob, keys, starts = {'icar': _icar, 'generic': _generic}[workload]()
    from occuspytial_amd._engine import Engine
    ids = _ids(prob.n, 7)

    def engine():
        eng = Engine(prob, keys)
        for c, st in enumerate(starts):
            eng.set_start(c, **st)
        return eng
    walk, never = engine(), engine()
    only = {x: engine() for x in OUTPUTS}
    walk.regions(ids)
    only['region'].regions(ids)
    for k, flips in enumerate(WALK):
        for name, on in flips:
            _switch(walk, name, on)
            _switch(only[name], name, on)
        draws = walk.run(6, 0)
        for other in [never] + list(only.values()):
            for u, v in zip(draws, other.run(6, 0)):
                assert np.array_equal(u, v), (k, 'recorded draws')
            for c in range(2):
                for nm in STATE:
                    assert np.array_equal(walk.get(nm, c), other.get(nm, c)), (k, nm, c)
        for name in OUTPUTS:
            for c in range(2):
                got, want = _answer(walk, name, c), _answer(only[name], name, c)
                assert _equal(got, want), (k, name, c, got, want)
        # ... and what those answers are, stated: an output that is on has this call's rows / every kept iteration so far
        calls_on = {x: sum(1 for j in ON_DURING[x] if j <= k) for x in OUTPUTS}
        for c in range(2):
            for x in ('site', 'll'):
                a = _answer(walk, x, c)
                assert ('have not been switched on' in a) if calls_on[x] == 0 else a['count'] == 6 * calls_on[x], (k, x, a)
            assert walk.region_draws(c).shape == ((6, 7) if k in ON_DURING['region'] else (0, 7))
            p = _answer(walk, 'ppc', c)
            assert ('has not been switched on' in p) if k < 4 else p.shape == ((6, 4) if k == 4 else (0, 4)), (k, p)
    for eng in [walk, never] + list(only.values()):
        eng.close()


def test_the_three_kinds_of_draws_beside_each_other():
    """The draws of a call from one description (occ_draws.hpp): `all` has the regions, the predictive check and the spatial
    check on for chain 0 and the regions alone for chain 1; only[x] has kind x alone, switched the same way.  run(7, 3), then
    run(2, 1): the draws and alpha, beta, tau, z, eta of the four engines are bit-equal, `all` answers for every kind and
    chain what only[x] answers, and the rows are the LAST call's.  A checkpoint holds the engine's switches (what the
    methods set for every chain, not one chain's later change) and no rows: draws belong to a call."""
    from occuspytial_amd import _lib
    from occuspytial_amd._engine import Engine
    prob, keys, starts = _icar()
    ids = _ids(prob.n, 7)
    kinds = tuple(_lib.DRAWS_KINDS)
    assert kinds == ('region', 'ppc', 'moran')
    off_for_chain_1 = ('ppc', 'moran')

    def engine(on):
        eng = Engine(prob, keys)
        for c, st in enumerate(starts):
            eng.set_start(c, **st)
        for kind in on:
            k = _lib.DRAWS_KINDS[kind]
            if k.input:
                eng.regions(ids)
            getattr(eng, k.fields[-2])(True)
            if kind in off_for_chain_1:
                eng.set(k.fields[-2], 0.0, 1)
        return eng
    every, only = engine(kinds), {x: engine((x,)) for x in kinds}
    width = {'region': 7, 'ppc': 4, 'moran': 8}
    for n_iter, burnin in ((7, 3), (2, 1)):
        keep = n_iter - burnin
        draws = every.run(n_iter, burnin)
        for x, other in only.items():
            for u, v in zip(draws, other.run(n_iter, burnin)):
                assert np.array_equal(u, v), (x, 'recorded draws')
            for c in range(2):
                for nm in STATE:
                    assert np.array_equal(every.get(nm, c), other.get(nm, c)), (x, nm, c)
        for x in kinds:
            rows_name = _lib.DRAWS_KINDS[x].fields[-1]
            for c in range(2):
                got, want = getattr(every, rows_name)(c), getattr(only[x], rows_name)(c)
                on = c == 0 or x not in off_for_chain_1
                assert got.shape == ((keep if on else 0), width[x]), (n_iter, x, c, got.shape)
                assert got.shape == want.shape and np.array_equal(got, want), (n_iter, x, c)
                assert every.get(rows_name, c).size == (keep * width[x] if on else 0)
                assert every.get(_lib.DRAWS_KINDS[x].fields[-2], c)[0] == float(on)
        assert np.any(every.region_draws(0)) and np.any(every.ppc_draws(0)) and np.any(every.moran_draws(0))
    ckpt = every.checkpoint()
    assert np.array_equal(ckpt['region_id'], np.tile(ids, (2, 1)))
    for x in kinds:
        assert np.array_equal(ckpt[_lib.DRAWS_KINDS[x].fields[-2]], np.ones(2)) and _lib.DRAWS_KINDS[x].fields[-1] not in ckpt
    fresh = Engine(prob, keys)
    fresh.restore(ckpt)
    for x in kinds:
        k = _lib.DRAWS_KINDS[x]
        assert getattr(fresh, k.on) is True
        for c in range(2):
            assert fresh.get(k.fields[-2], c)[0] == 1.0
            assert getattr(fresh, k.fields[-1])(c).shape == (0, width[x]), (x, c)
    assert np.array_equal(fresh.get('region_id'), ids)
    for eng in [every, fresh] + list(only.values()):
        eng.close()


def test_probit_region_switch_on_and_off():
    """The probit handle's one output, five run(10, 0) calls (its captured graph holds eight iterations, so every call
    replays it once and steps twice): off, both chains on, chain 0 off while chain 1 stays on, both off, both on.  Draws
    and state equal those of a handle that never counted; a chain's rows equal those of a handle that always counted."""
    prob, keys, starts = _probit_problem(2)
    ids = _ids(prob.n, 7)
    walk, always, never = (_probit_engine(prob, keys, starts, ids, on=False), _probit_engine(prob, keys, starts, ids),
                           _probit_engine(prob, keys, starts))
    for k, switches in enumerate([(0, 0), (1, 1), (0, 1), (0, 0), (1, 1)]):
        for c, on in enumerate(switches):
            walk.set('region_stats', float(on), c)
        draws = walk.run(10, 0)
        for other in (always, never):
            for u, v in zip(draws, other.run(10, 0)):
                assert np.array_equal(u, v), k
            for c in range(2):
                for nm in ('alpha', 'beta', 'eta', 'eps', 'z', 'c'):
                    assert np.array_equal(walk.get(nm, c), other.get(nm, c)), (k, nm, c)
        for c, on in enumerate(switches):
            assert walk.get('region_stats', c)[0] == on
            rows = walk.region_draws(c)
            assert rows.shape == ((10, 7) if on else (0, 7)), (k, c)
            if on:
                assert np.array_equal(rows, always.region_draws(c)), (k, c)
    for eng in (walk, always, never):
        eng.close()
