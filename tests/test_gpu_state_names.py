"""The plain state names of a chain on the MI355X (occuspytial_amd/csrc/occ_names.hpp: STATE), name by name and model by model:
``alpha beta tau eta theta z xz c eps iter k exists omega_a omega_b rhs minres_itn rsr_gram link`` and the two ``debug_*``
words, through ``occ_get_state`` / ``occ_set_state`` of ``LogitICARGibbs``, the reduced-rank and the probit model, two
chains each.  What a name's length is, who reads and writes it and what a mistake earns is written out here from
include/occ_gibbs.h; ``_lib.STATE_NAMES`` is compared with it, not consulted.

The problem is a 6 x 7 lattice with 30 surveyed sites of one to three visits: n = 42, S = 30, R = 61, 2n = 84, p = 2, q = 3,
m = 5, m*m = 25 and 1 are pairwise distinct, so a wrong unit cannot hide behind an equal length."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from ._outputs_gpu import time_limit as _time_limit  # noqa: F401 (autouse in this module)

pytestmark = pytest.mark.gpu

MODELS = ('icar', 'rsr', 'probit')
KEYS = [0x51A7E0001, 0x51A7E0002]
EVERY, LOGIT = set(MODELS), {'icar', 'rsr'}
# name -> (length in the problem's sizes, the models that read it, the models that write it)
NAMES = {
    'alpha': ('q', EVERY, EVERY), 'beta': ('p', EVERY, EVERY), 'tau': ('1', EVERY, EVERY), 'iter': ('1', EVERY, EVERY),
    'eta': ('n', EVERY, EVERY), 'z': ('n', EVERY, EVERY), 'k': ('n', EVERY, set()), 'exists': ('S', EVERY, set()),
    'omega_a': ('R', EVERY, EVERY), 'omega_b': ('n', EVERY, set()), 'rhs': ('n', LOGIT, set()), 'xz': ('2n', LOGIT, LOGIT),
    'minres_itn': ('1', LOGIT, set()), 'theta': ('m', {'rsr', 'probit'}, {'rsr', 'probit'}), 'rsr_gram': ('m*m', {'rsr'}, set()),
    'eps': ('n', {'probit'}, {'probit'}), 'c': ('m', {'probit'}, {'probit'}), 'link': ('1', {'probit'}, set()),
    'debug_close_window': ('1', set(), LOGIT), 'debug_maxiter': ('1', set(), LOGIT),
}
IN_THE_SCALARS = ('alpha', 'beta', 'tau', 'iter')       # their wrong length is worded like an unknown name
REDRAWS = ('alpha', 'beta', 'tau', 'iter', 'eta', 'z', 'omega_a', 'xz', 'theta', 'debug_maxiter')   # a write sets need_prologue
# the probit model's theta written back passes through eta = K theta (m = 5 products), c = Phi' eta (n = 42) and theta = G c (5):
# at most 52 roundings of 2^-53 each, on terms a few times the result's largest entry (|K|, |Phi|, |G| <= a few): below 1e-13 of
# it; 1e-12 leaves a factor of ten
ROUNDING = 1e-12
UNKNOWN, NOT_WRITABLE, WRONG_LENGTH ='^unknown state name$', '^unknown state name or wrong length$', '^wrong length$'


def _problem(model):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(6, 7, visits=3, p=2, q=3, random_state=5)
    kept = [i for i in range(42) if i % 7 not in (2, 5)]                       # 12 sites are not surveyed
    W = {i: W[i][:(2 if j == 0 else 1 + j % 3)] for j, i in enumerate(kept)}   # 2, 2, 3, 1, 2, 3, ...: 61 rows
    y = {i: y[i][:len(W[i])] for i in kept}
    prob = FlatProblem(Q, W, X, y)
    if model == 'rsr':
        prob.enable_rsr(q=5)
    if model == 'probit':
        prob.enable_probit(q=5)
    return prob


def _sizes(prob, model):
    m = 0 if model == 'icar' else (prob.probit if model == 'probit' else prob.rsr)['dim']
    return {'1': 1, 'n': prob.n, 'S': prob.S, 'R': prob.R, 'p': prob.p, 'q': prob.q, 'm': m, '2n': 2 * prob.n, 'm*m': m * m}


def _engine(model, prob=None):
    from occuspytial_amd._engine import Engine
    prob = prob or _problem(model)
    rng = np.random.default_rng(21)
    eng = Engine(prob, KEYS)
    for c in range(2):
        eta = rng.standard_normal(prob.n)
        spatial = eta - eta.mean() if model == 'icar' else rng.standard_normal(5)   # (with a basis the start holds theta)
        eng.set_start(c, rng.standard_normal(prob.q), rng.standard_normal(prob.p), 1.0 + c, spatial)
        if model == 'probit':
            eng.set('eps', rng.standard_normal(prob.n), c)
    return eng


def _readable(model):
    return [nm for nm, (_, read, _) in NAMES.items() if model in read]


def _state(eng, model):
    return {(nm, c): np.atleast_1d(eng.get(nm, c)) for nm in _readable(model) for c in range(2)}


def _same(a, b, but=()):
    assert a.keys() == b.keys()
    for key in a:
        if key not in but:
            assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key]), key


def _length_query(eng, name, chain):
    ln = C.c_int64(-1)
    eng._check(eng._lib.occ_get_state(eng._h, chain, name.encode(), None, 0, C.byref(ln)))
    return ln.value


def _other(name, value, prob):
    """A value of the same length that differs from ``value`` and that the model can hold."""
    new = np.array(np.atleast_1d(value), dtype=np.float64)
    if name == 'z':
        i = prob.not_surveyed[0]
        new[i] = 1.0 - new[i]
    elif name == 'iter':
        new += 4.0
    else:
        new += 0.125 * (1.0 + np.arange(new.size) % 3)
    return new


def test_the_sizes_are_pairwise_distinct_and_the_binding_says_the_same():
    from occuspytial_amd import _lib
    sizes = _sizes(_problem('probit'), 'probit')
    assert len(set(sizes.values())) == len(sizes) == 9, sizes
    prob = _problem('icar')
    assert prob.S < prob.n and prob.R % prob.S != 0 and prob.p != prob.q and 0 < len(prob.obs) < prob.S
    bit = dict(icar=_lib.ICAR, rsr=_lib.RSR, probit=_lib.PROBIT)
    assert set(_lib.STATE_NAMES) == set(NAMES)
    for nm, (unit, read, write) in NAMES.items():
        st = _lib.STATE_NAMES[nm]
        assert (st.unit, st.read, st.write) == (unit, sum(bit[k] for k in read), sum(bit[k] for k in write)), nm
        assert st.prologue == (nm in REDRAWS), nm


@pytest.mark.parametrize('model', MODELS)
def test_lengths_and_refusals(model):
    """A length query equals the name's length and the read's; a name the model lacks is unknown; one element too many, a
    read-only name and a name that is none earn their words."""
    eng = _engine(model)
    try:
        eng.run(3, 0)
        sizes = _sizes(eng.prob, model)
        for nm, (unit, read, write) in NAMES.items():
            want = sizes[unit]
            if model in read:
                for c in range(2):
                    assert _length_query(eng, nm, c) == want == eng.get(nm, c).size, (nm, c)
            else:
                with pytest.raises(ValueError, match=UNKNOWN):
                    eng.get(nm, 1)
                with pytest.raises(ValueError, match=UNKNOWN):
                    _length_query(eng, nm, 1)
            if model in write:
                with pytest.raises(ValueError, match=NOT_WRITABLE if nm in IN_THE_SCALARS else WRONG_LENGTH):
                    eng.set(nm, np.zeros(want + 1), 1)
            else:
                with pytest.raises(ValueError, match=NOT_WRITABLE):
                    eng.set(nm, np.zeros(want), 1)
        if model in LOGIT:
            with pytest.raises(ValueError, match=WRONG_LENGTH):      # (a negative limit is worded as a wrong length)
                eng.set('debug_maxiter', -1.0, 1)
        for nm in ('', 'nonesuch', 'Alpha', 'alpha '):
            with pytest.raises(ValueError, match=UNKNOWN):
                eng.get(nm, 0)
            with pytest.raises(ValueError, match=NOT_WRITABLE):
                eng.set(nm, 1.0, 0)
        for chain in (-1, 2):
            with pytest.raises(ValueError, match='bad chain index'):
                eng.get('alpha', chain)
    finally:
        eng.close()


@pytest.mark.parametrize('model', MODELS)
def test_a_write_reaches_its_name_on_its_chain_only(model):
    """Chain 1's own value written back leaves every readable name of both chains bit-equal.  One write cannot: the probit
    model's theta is read as G c and written as c = Phi' (K theta), so c, eta and theta come back through other sums; they
    agree to rounding (ROUNDING) and every other name is bit-equal.  Another value changes that name on chain 1 and nothing on
    chain 0."""
    eng = _engine(model)
    try:
        eng.run(3, 0)
        prob = eng.prob
        writable = [nm for nm, (_, _, write) in NAMES.items() if model in write and not nm.startswith('debug_')]
        for nm in writable:                                              # (first every write-back: the state is a chain's own)
            before = _state(eng, model)
            eng.set(nm, before[nm, 1], 1)
            after = _state(eng, model)
            follows = [('eta', 1), ('c', 1), ('theta', 1)] if nm == 'theta' and model == 'probit' else []
            for key in follows:
                print(model, 'theta written back:', key[0], 'moves by at most', np.abs(after[key] - before[key]).max(), 'of', np.abs(before[key]).max())
            _same(before, after, but=follows)
            for key in follows:
                assert np.allclose(after[key], before[key], rtol=0, atol=ROUNDING * max(1.0, np.abs(before[key]).max())), (nm, key)
        for nm in writable:
            before = _state(eng, model)
            new = _other(nm, before[nm, 1], prob)
            eng.set(nm, new, 1)
            changed = _state(eng, model)
            _same({k: v for k, v in before.items() if k[1] == 0}, {k: v for k, v in changed.items() if k[1] == 0})
            if nm == 'theta' and model == 'probit':                      # (read back as G c, c = G^-1 theta)
                assert np.allclose(changed[nm, 1], new, rtol=0, atol=ROUNDING * np.abs(new).max())
            else:
                assert np.array_equal(changed[nm, 1], new), nm
            assert not np.array_equal(changed[nm, 1], before[nm, 1]), nm
    finally:
        eng.close()


@pytest.mark.parametrize('model', MODELS)
def test_the_views_and_the_computed_names(model):
    """k is z - 1/2; exists is "detected, or z = 1" over the surveyed sites; xz is the two halves of the warm start, x then z;
    the probit model's theta is G c by the host's fma loop, to the last bit; link is 1."""
    eng = _engine(model)
    try:
        prob = eng.prob
        if model in LOGIT:
            assert not eng.get('xz', 0).any()                            # (a start has no warm start)
        eng.run(3, 0)
        for c in range(2):
            z = eng.get('z', c)
            assert set(np.unique(z)) <= {0.0, 1.0} and np.array_equal(eng.get('k', c), z - 0.5)
            exists = prob.obs_site.astype(bool) | (z[prob.site_id] == 1.0)
            assert np.array_equal(eng.get('exists', c), exists.astype(np.float64))
            assert int(eng.get('iter', c)) == 3
        if model == 'icar':
            assert eng.get('xz', 1).any()
        if model in LOGIT:
            x, zz = np.arange(1.0, prob.n + 1), -np.arange(1.0, prob.n + 1) / 3.0
            eng.set('xz', np.concatenate([x, zz]), 1)
            got = eng.get('xz', 1)
            assert np.array_equal(got[:prob.n], x) and np.array_equal(got[prob.n:], zz)
        if model == 'probit':
            G = np.asarray(prob.probit['G'], dtype=np.float64)
            for c in range(2):
                cc = np.atleast_1d(eng.get('c', c))
                want = []
                for i in range(G.shape[0]):
                    t = 0.0
                    for j in range(G.shape[1]):                          # fma: the exact product and sum, rounded once
                        t = float(Fraction(float(G[i, j])) * Fraction(float(cc[j])) + Fraction(t))
                    want.append(t)
                assert np.array_equal(eng.get('theta', c), np.array(want)), c
            assert np.atleast_1d(eng.get('link', 0)).tolist() == [1.0]
    finally:
        eng.close()


@pytest.mark.parametrize('model', MODELS)
def test_a_write_that_redraws_continues_like_a_restored_engine(model):
    """After a write of a name whose row has the prologue flag, run(2) equals run(2) of a second engine restored from a
    checkpoint taken before the write and given the same write (a restore always redraws).  The first engine has run since
    its last write, so only the write itself can ask for the redraw."""
    prob = _problem(model)
    one, two = _engine(model, prob), _engine(model, prob)
    try:
        one.run(3, 0)
        start = one.checkpoint()
        for nm in REDRAWS:
            if model not in NAMES[nm][2]:
                continue
            one.restore(start)
            one.run(1, 0)
            ckpt = one.checkpoint()
            value = np.zeros(1) if nm == 'debug_maxiter' else _other(nm, one.get(nm, 1), prob)
            one.set(nm, value, 1)
            two.restore(ckpt)
            two.set(nm, value, 1)
            for a, b in zip(one.run(2, 0), two.run(2, 0)):
                assert np.array_equal(a, b), nm
            # (omega_a is no part of a checkpoint: an iteration draws it where the site exists by the z it began with and leaves
            # the other rows as they were, which are never read)
            _same(_state(one, model), _state(two, model), but=[('omega_a', 0), ('omega_a', 1)])
    finally:
        one.close()
        two.close()
