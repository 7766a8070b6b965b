"""Sum-to-zero per connected component, everything that needs no GPU: ``graph.components``, the ``constraint`` keyword of
the problem and the samplers, the launch order with the correction pass (occ_plan.hpp: seq_launches), the host's tables of
the pass under the sanitizers (occ_comp_plan.hpp as a stand-alone program), the stand-in library's refusal, and the stored
draws of the dense restatement (tests/golden/components34.npz)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy import sparse

from . import _components_graphs as G
from . import _components_reference as R
from .test_order_cpu import (BEHIND, BETA_PARTIAL, COUNTERS, EAGER, ETA_INIT, EVENT_NODES, HOST_WATCHED, ITER, K_LAST, MAIN, MINRES,
                             ONE_STREAM, RSR_ONE_STREAM, S_CAPTURED, S_EAGER, S_FUSED, S_RSR, SIDE, STREAM_EVENTS, Z_OB)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')
COMP_PART, COMP_COEF, COMP_ETA, COMP_BETA = 13, 14, 15, 16   # occ::Kind, behind the reduced-rank kinds


# ---- graph.components ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('make', [G.small, G.large, G.connected])
def test_components_of_the_test_graphs(make):
    from occuspytial_amd.graph import components
    g = make()
    k, labels = components(g['Q'])
    assert k == g['k'] and labels.dtype == np.int32 and np.array_equal(labels, g['labels'])
    assert labels[0] == 0 and np.array_equal(np.unique(labels), np.arange(k))
    firsts = [int(np.flatnonzero(labels == c)[0]) for c in range(k)]
    assert firsts == sorted(firsts)                      # numbered by lowest site
    sizes = np.bincount(g['comp'])
    assert sorted(np.bincount(labels).tolist()) == sorted(sizes.tolist())


def test_components_ignore_stored_zeros_and_the_diagonal():
    from occuspytial_amd.graph import components
    # sites 0-1 joined, site 2 with an explicit zero row (stored zeros, its diagonal too), sites 3-4 joined by a stored zero only
    rows = [0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4]
    cols = [0, 1, 0, 1, 0, 2, 4, 3, 4, 3, 4]
    vals = [1., -1., -1., 1., 0., 0., 0., 0., 0., 0., 0.]
    Q = sparse.csr_matrix((vals, (rows, cols)), shape=(5, 5))
    k, labels = components(Q)
    assert k == 4 and labels.tolist() == [0, 0, 1, 2, 3]
    assert components(np.zeros((3, 3)))[0] == 3


# ---- the keyword: FlatProblem -----------------------------------------------------------------------------------------
def _prob(g, **kw):
    from occuspytial_amd._problem import FlatProblem
    return FlatProblem(g['Q'], g['W'], g['X'], g['y'], **kw)


def test_tau_shape_default_counts_the_rank_of_q():
    g = G.small()
    assert _prob(g, constraint='component').tau_shape == 0.5 + 0.5 * (34 - 5)
    assert _prob(g).tau_shape == _prob(g, constraint='global').tau_shape == 0.5 + 0.5 * 33
    assert _prob(g, constraint='component', hparams={'tau_shape': 3.25}).tau_shape == 3.25
    assert _prob(g, constraint='component', hparams={'tau_rate': 0.1}).tau_shape == 0.5 + 0.5 * 29
    assert _prob(G.connected(), constraint='component').tau_shape == 0.5 + 0.5 * 35
    with pytest.raises(ValueError, match="constraint must be 'global' or 'component'"):
        _prob(g, constraint='islands')


def test_default_start_is_centred_per_component_from_the_same_variates():
    from occuspytial_amd._problem import default_start
    g = G.small()
    a = default_start(np.random.default_rng(3), _prob(g, constraint='component'))
    b = default_start(np.random.default_rng(3), _prob(g))
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(a[name], b[name])
    labels = g['labels']
    raw = np.random.default_rng(3)
    raw.gamma(0.5, 1 / 0.005)
    eta = raw.standard_normal(34)                       # the same variates, in the same place of the stream
    assert np.array_equal(b['eta'], eta - eta.mean())
    for c in range(5):
        m = labels == c
        if m.sum() == 1:
            assert a['eta'][m][0] == 0.0
        else:
            assert np.allclose(a['eta'][m], eta[m] - eta[m].mean(), rtol=0, atol=1e-15) and abs(a['eta'][m].sum()) < 1e-14
    one = G.connected()
    c1, c2 = (default_start(np.random.default_rng(4), _prob(one, constraint=k)) for k in ('component', 'global'))
    assert np.array_equal(c1['eta'], c2['eta'])          # one component: the global path, bit for bit


def test_arrays_round_trip_carries_the_mode():
    from occuspytial_amd._engine import ProblemMeta
    from occuspytial_amd._problem import FlatProblem
    g = G.small()
    p = _prob(g, constraint='component')
    d = p.to_arrays()
    back = FlatProblem.from_arrays(d)
    assert back.constraint == 'component' and back.n_components == 5 and np.array_equal(back.component_labels, g['labels'])
    assert back.tau_shape == p.tau_shape
    plain = _prob(g).to_arrays()
    assert 'component_labels' not in plain
    old = FlatProblem.from_arrays(plain)                 # a dict without the key: the global constraint
    assert old.constraint == 'global' and old.n_components == 1 and old.component_labels is None
    assert set(ProblemMeta.of(_prob(g)).to_dict()) == set(ProblemMeta.FIELDS)
    meta = ProblemMeta(**ProblemMeta.of(p).to_dict())
    assert meta.constraint == 'component' and meta.n_components == 5 and np.array_equal(meta.component_labels, g['labels'])
    assert ProblemMeta(**ProblemMeta.of(_prob(g)).to_dict()).constraint == 'global'


# ---- the keyword: the samplers refuse before an engine exists -----------------------------------------------------------
def test_samplers_refuse_before_an_engine_exists(monkeypatch):
    from occuspytial_amd import LogitICARGibbs, LogitRSRGibbs, ProbitRSRGibbs, _lib
    from occuspytial_amd.gibbs.base import GibbsBase

    def no_library():
        raise AssertionError('the engine library was asked for')
    monkeypatch.setattr(_lib, 'load', no_library)
    g = G.small()
    args = (g['Q'], g['W'], g['X'], g['y'])
    for cls in (LogitRSRGibbs, ProbitRSRGibbs):
        with pytest.raises(ValueError, match="has no constraint='component': its spatial effect K theta carries no sum-to-zero"):
            cls(*args, constraint='component')
    for cls in (LogitICARGibbs, LogitRSRGibbs, ProbitRSRGibbs):
        with pytest.raises(ValueError, match="constraint must be 'global' or 'component'"):
            cls(*args, constraint='each')

    class Stepper(GibbsBase):   # a sampler that steps in Python
        def __init__(self, Q, W, X, y, constraint='global'):
            super().__init__(Q, W, X, y)
            self._configure(Q, None, constraint=constraint)

    with pytest.raises(ValueError, match="Stepper steps in Python: constraint='component'"):
        Stepper(*args, constraint='component')
    assert Stepper(*args)._problem.constraint == 'global'
    s = LogitICARGibbs(*args, constraint='component')
    assert s._problem.constraint == 'component' and s._problem.n_components == 5 and s.fixed.tau_shape == 15.0
    assert LogitICARGibbs(*args).fixed.tau_shape == 17.0
    assert LogitICARGibbs(*args, hparams={'tau_shape': 2.0}, constraint='component').fixed.tau_shape == 2.0


# ---- the stand-in library does not know the state name ------------------------------------------------------------------
def test_stand_in_library_answers_rebuild_it(monkeypatch, oracle):
    from occuspytial_amd import LogitICARGibbs, _lib
    from .test_cpu_abi import ABI_LIB
    if not os.path.exists(ABI_LIB):
        oracle.build()
    monkeypatch.setattr(_lib, 'LIB_PATH', ABI_LIB)
    monkeypatch.setattr(_lib, '_lib', None)
    assert _lib.load().occ_device_count() == 0
    g = G.small()
    args = (g['Q'], g['W'], g['X'], g['y'])
    with pytest.raises(ValueError, match=r"the loaded engine library has no constraint='component' \(.*\): rebuild it"):
        LogitICARGibbs(*args, random_state=1, constraint='component').sample(4, chains=1, progressbar=False)
    out = LogitICARGibbs(*args, random_state=1).sample(4, chains=1, progressbar=False)        # 'global' runs unchanged
    assert out['tau'].shape == (1, 4)
    one = G.connected()
    a, b = (LogitICARGibbs(one['Q'], one['W'], one['X'], one['y'], random_state=2, constraint=k).sample(6, chains=2, progressbar=False)
            for k in ('component', 'global'))
    for name in ('alpha', 'beta', 'tau'):   # one component: no call about the labels reaches the library, the same chains
        assert np.array_equal(a[name], b[name])


# ---- the launch order with the correction pass ----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def order():
    subprocess.run(['make', '-s', '-C', CSRC, 'plan'], check=True)
    lib = C.CDLL(os.path.join(ROOT, 'build', 'libocc_plan.so'))
    for name, nargs in (('occ_order_launches', 6), ('occ_order_launches_comp', 7)):
        getattr(lib, name).restype = C.c_int32
        getattr(lib, name).argtypes = [C.c_int32] * nargs + [C.POINTER(C.c_int32), C.c_int32]

    def launches(mode, where, solve, p=0, cap=0, gate_kernel=False, comp=None):
        out = (C.c_int32 * (3 * 64))()
        if comp is None:
            n = lib.occ_order_launches(mode, where, solve, p, cap, int(gate_kernel), out, 64)
        else:
            n = lib.occ_order_launches_comp(mode, where, solve, p, cap, int(gate_kernel), int(comp), out, 64)
        assert n >= 0
        return [tuple(out[3 * i:3 * i + 3]) for i in range(n)]
    return launches


def correction(e):
    return [(COMP_PART, e, 0), (COMP_COEF, e, 0), (COMP_ETA, e, 0), (COMP_BETA, e, 0)]


def test_correction_follows_the_last_launch_of_every_icar_solve(order):
    """k > 1: the four launches (chunk sums, coefficients, eta, beta's partial sums again) stand directly behind the solve's last launch -- k_iter, or k_beta_partial of a captured or
    a host-watched per-step solve -- and so in front of the z update, on the stream that holds the solve."""
    for e in (0, 1):
        got = order(EVENT_NODES, MAIN, S_FUSED, p=e, comp=1)
        assert got[:5] == [(ITER, e, 0)] + correction(e) and got[6] == (Z_OB, e, 0)
        got = order(EVENT_NODES, MAIN, S_CAPTURED, p=e, cap=2, comp=1)
        assert got[:7] == [(ETA_INIT, e, 0)] + [(MINRES, e, k) for k in range(1, 6)] + [(BETA_PARTIAL, e, 5)]
        assert got[7:11] == correction(e) and got[12] == (Z_OB, e, 0)
        got = order(EVENT_NODES, EAGER, S_EAGER, p=e, comp=1)
        i = got.index((BETA_PARTIAL, e, K_LAST))
        assert got[i - 1] == (MINRES, e, HOST_WATCHED) and got[i + 1:i + 5] == correction(e) and got[i + 5] == (Z_OB, e, 0)
        got = order(EVENT_NODES, EAGER, S_FUSED, p=e, comp=1)
        i = got.index((ITER, e, 0))
        assert got[i + 1:i + 5] == correction(e) and got[i + 5] == (Z_OB, e, 0)
    # the counters' graphs: GRAPH_SEQ sequences of alternating parity, the pass in each; nothing of it on the side stream
    got = order(COUNTERS, MAIN, S_FUSED, p=1, comp=1)
    assert got == [(ITER, 1, 0)] + correction(1) + [(Z_OB, 1, 0), (ITER, 0, 0)] + correction(0) + [(Z_OB, 0, 0)]
    for mode in (COUNTERS, EVENT_NODES, STREAM_EVENTS):
        assert order(mode, SIDE, S_FUSED, comp=1) == order(mode, SIDE, S_FUSED)
    assert order(STREAM_EVENTS, MAIN, S_FUSED, comp=1) == [(ITER, 0, 0)] + correction(0)
    assert order(STREAM_EVENTS, BEHIND, S_FUSED, comp=1) == [(Z_OB, 0, 0)]
    # the reduced-rank model has no such pass
    for mode in (RSR_ONE_STREAM, COUNTERS):
        assert order(mode, MAIN, S_RSR, comp=1) == order(mode, MAIN, S_RSR)


def test_one_component_emits_what_is_emitted_today(order):
    """k == 1 (comp = 0): the same sequence as the entry point without the argument, for every mode, place, solve shape,
    parity and gate.  (A solve carried to the next sequence is the device's decision, Ctl::koff: the pure function emits the
    same launches for it, and the pass's kernels leave a carrying chain alone -- tests/test_gpu_components.py forces carries
    with a small captured cap and asks for the same bits.)"""
    for mode in (COUNTERS, RSR_ONE_STREAM, EVENT_NODES, STREAM_EVENTS, ONE_STREAM):
        for where in (MAIN, SIDE, BEHIND, EAGER):
            for solve in (S_RSR, S_FUSED, S_CAPTURED, S_EAGER):
                for p in (0, 1):
                    for gate in (False, True):
                        assert order(mode, where, solve, p, 3, gate, comp=0) == order(mode, where, solve, p, 3, gate)
    kinds = {k for m in (COUNTERS, EVENT_NODES) for l in order(m, MAIN, S_FUSED, comp=0) for k in l[:1]}
    assert not kinds & {COMP_PART, COMP_COEF, COMP_ETA, COMP_BETA}


# ---- the host's tables, under AddressSanitizer and UBSan ----------------------------------------------------------------
@pytest.fixture(scope='module')
def comp_check():
    subprocess.run(['make', '-s', '-C', CSRC, 'comp_check'], check=True)
    exe = os.path.join(ROOT, 'build', 'occ_comp_check')

    def run(labels):
        text = '%d\n%s\n' % (len(labels), ' '.join(str(int(v)) for v in labels))
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr   # (the program checks that the chunks tile the list and none straddles a component)
        return r.stdout.split()
    return run


def test_chunk_tables_tile_the_list(comp_check):
    for make in (G.small, G.large):
        g = make()
        sizes = np.bincount(g['labels'])
        want = int(np.sum((sizes + 31) // 32))
        assert comp_check(g['labels']) == ['ok', str(g['k']), str(want), '0', str(min(32, sizes.max()))]
        assert comp_check(g['comp'] * 7)[:3] == ['ok', str(g['k']), str(want)]      # any numbering
    n = 5000                                              # all singletons but one edge
    lab = np.arange(n)
    lab[4321] = 17
    assert comp_check(lab) == ['ok', str(n - 1), str(n - 1), '0', '2']
    big = np.zeros(100000, dtype=np.int64)                # one component of 100 000 sites: 3 125 chunks, a wave's second level
    assert comp_check(big) == ['ok', '1', '3125', '1', '32']
    two = np.concatenate([np.zeros(2049), np.ones(2048)]).astype(np.int64)   # 65 and 64 chunks: one heavy, one light
    assert comp_check(two) == ['ok', '2', '129', '1', '32']
    assert comp_check([0, 3, 1])[0] == 'refused:' and comp_check([-1, 0])[0] == 'refused:'
    assert comp_check([]) == ['ok', '0', '0', '0', '0']


# ---- the dense restatement and its stored draws -------------------------------------------------------------------------
def test_devroye_sampler_has_the_moments_of_pg1():
    rng = np.random.default_rng(9)
    for c in (0.0, 0.7, 3.0):
        x = np.array([R.pg1_devroye(c, rng) for _ in range(4000)])
        mean = 0.25 if c == 0 else np.tanh(c / 2) / (2 * c)
        var = 1 / 24 if c == 0 else (np.sinh(c) - c) / (4 * c ** 3 * np.cosh(c / 2) ** 2)
        assert abs(x.mean() - mean) < 5 * np.sqrt(var / x.size), (c, x.mean(), mean)
        assert abs(x.var() - var) < 0.15 * var, (c, x.var(), var)


def test_restatement_centres_every_component_and_its_settings_differ():
    """The stored draws: under the global constraint log tau sits far outside the band the GPU test allows around the
    per-component posterior mean (4 batch-means MCSE of the restatement), so that test can tell the two models apart on this
    graph.  Chosen graph: tests/_components_graphs.py small() as the issue describes it -- it needed no enlarging."""
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'components34.npz'))
    assert z['alpha'].shape == (2, 2500, 2) and z['beta'].shape == (2, 2500, 2) and z['tau'].shape == (2, 2500)
    lt, lg = np.log(z['tau']), np.log(z['global_tau'])
    band = 4 * R.batch_means_mcse(lt)
    assert abs(lg.mean() - lt.mean()) > band, (lg.mean(), lt.mean(), band)
    # a short run of the restatement itself: every component centred, the single sites at exactly 0; under the global
    # constraint the sites sum to zero together and the components do not
    g = G.small()
    labels = g['labels']
    *_, eta = R.run_chain(g, 'component', 40, seed=1, tau_shape=float(z['tau_shape']), tau_rate=float(z['tau_rate']), with_eta=True)
    assert all(abs(eta[labels == c].sum()) < 1e-10 for c in range(5)) and np.all(eta[list(g['singles'])] == 0.0)
    *_, eta = R.run_chain(g, 'global', 40, seed=1, with_eta=True)
    assert abs(eta.sum()) < 1e-10 and max(abs(eta[labels == c].sum()) for c in range(5)) > 1e-3


def test_a_library_that_knows_the_name_keeps_its_own_words(monkeypatch, oracle):
    """Only "unknown state name" becomes "rebuild it": another refusal of the labels reaches the caller as the library worded it,
    and the half-made engine is closed either way."""
    from occuspytial_amd import _lib
    from occuspytial_amd._engine import Engine
    from .test_cpu_abi import ABI_LIB
    if not os.path.exists(ABI_LIB):
        oracle.build()
    monkeypatch.setattr(_lib, 'LIB_PATH', ABI_LIB)
    monkeypatch.setattr(_lib, '_lib', None)
    g = G.small()
    prob = _prob(g, constraint='component')
    closed = []
    real_close = Engine.close
    monkeypatch.setattr(Engine, 'close', lambda self: (closed.append(1), real_close(self))[1])

    def refuse(words, kind=ValueError):
        def set_(self, name, value, chain=0):
            raise kind(words)
        return set_
    monkeypatch.setattr(Engine, 'set', refuse('component_id belongs to the ICAR model'))
    with pytest.raises(ValueError, match='^component_id belongs to the ICAR model$'):
        Engine(prob, [1])
    monkeypatch.setattr(Engine, 'set', refuse('HIP engine failure: out of memory', _lib.EngineUnavailable))
    with pytest.raises(_lib.EngineUnavailable, match='out of memory'):
        Engine(prob, [1])
    assert len(closed) >= 2
