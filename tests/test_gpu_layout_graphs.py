"""The kernels that walk a row of Q on the graphs of tests/_layout_graphs.py.  Needs an MI355X: ``-m gpu``.

What each graph reaches (true SELL-64 bases, rows of more than 16 off-diagonals, an ELL layout wider than 16, slices of width 0,
a site without neighbours, the general tile form) is pinned on the CPU by tests/test_layout_graphs_cpu.py, with the figures
that the bounds here rest on.  Three kinds of check:
  * lock step with the CPU oracle under test_gpu_parity's tolerances (its sensitivity rule is capped on the CPU at 1e-5),
    in every form of the eta solve that the planner's ladder holds for the graph;
  * a check that does not depend on the Krylov path: the relative residual of the engine's own xz on the engine's own
    system, in numpy, at most twice the oracle's for the same iteration;
  * the forms of the solve (one XCD per chain, any placement, tiles, launch per step; diagonal form or stored slots) against
    each other, bit for bit."""
import numpy as np
import pytest

from . import _layout_graphs as G
from .test_gpu_parity import KEY, TOL, _compare_iteration, _random_start, _rel

pytestmark = pytest.mark.gpu

KNOBS = ('OCC_NO_PERSISTENT', 'OCC_NO_XCD_LOCAL', 'OCC_NO_TILES', 'OCC_FORCE_TILES', 'OCC_NO_DIA')
FORMS = {'xcd_local': ({}, 2), 'any_placement': ({'OCC_NO_XCD_LOCAL': '1'}, 1), 'launch_per_step': ({'OCC_NO_PERSISTENT': '1'}, 0)}
LADDER = {name: list(FORMS) for name in ('sell8', 'sell16', 'one_isolated') + G.EMPTY}
LADDER.update(hub=['steps_only'], wide_ell=['steps_only'])  # rows of more than 16 off-diagonals: FORM_STEPS without any knob
RESIDUAL_FACTOR = 2.0  # (test_layout_graphs_cpu.py: one MINRES step less leaves less than twice the oracle's residual)


def _set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _engine(monkeypatch, prob, keys, form, env=None):
    """An engine in one form of the solve; the form it reports is asserted."""
    from occuspytial_amd._engine import Engine
    knobs, code = FORMS.get(form, ({}, 0))
    _set_env(monkeypatch, {**knobs, **(env or {})})
    eng = Engine(prob, keys)
    st = eng.stats()
    if form == 'tiles':
        assert st['persistent_solve'] == 3 and st['threads_per_block'] == 256, st
    else:
        assert st['persistent_solve'] == code, (form, st)
    return eng


def _residual_of(src, prob, chain=None):
    get = (lambda name: src.get(name, chain)) if chain is not None else src.get
    return G.residual(prob.Q, float(get('tau')), get('omega_b'), get('rhs'), get('xz'))


def _lockstep_graph(oracle, monkeypatch, prob, start, form, env=None, n_iter=3, empty=False):
    """Three iterations in lock step with the oracle, the engine re-seated on the oracle's state after each
    (test_gpu_parity._lockstep, plus the residual check).  ``empty``: the rule for graphs with a slice of 64 sites without
    neighbours, whose joint solve is sensitive to the summation order -- what does not depend on MINRES's path is held to the
    oracle (omega_b, tau, rhs at TOL; z and k equal), xz is held by its residual and, at the isolated sites, by the closed form
    within 10 x the oracle's own deviation from it."""
    eng = _engine(monkeypatch, prob, [KEY], form, env)
    orc = oracle.OracleSampler(prob, KEY)
    eng.set_start(0, **start)
    orc.set_start(**start)
    worst = {}
    for it in range(n_iter):
        x0 = orc.get('xz')
        eng.step()
        orc.step()
        if empty:
            got = {name: _rel(eng.get(name), orc.get(name)) for name in ('omega_b', 'tau', 'rhs')}
            for name, v in got.items():
                assert v < TOL[name], (it, name, v)
            assert np.array_equal(eng.get('z'), orc.get('z')) and np.array_equal(eng.get('k'), orc.get('k'))
            dev_o = G.closed_form_deviation(prob.Q, orc.get('omega_b'), orc.get('rhs'), orc.get('xz'))
            dev_e = G.closed_form_deviation(prob.Q, eng.get('omega_b'), eng.get('rhs'), eng.get('xz'))
            got.update(closed_form=dev_e, closed_form_oracle=dev_o, xz=_rel(eng.get('xz'), orc.get('xz')),
                       itn=abs(int(eng.get('minres_itn')) - int(orc.get('minres_itn'))))
            assert dev_e <= max(1e-4, 10.0 * dev_o), (it, dev_e, dev_o)
        else:
            got = _compare_iteration(eng, orc, prob, x0=x0)
        r_eng, r_orc = _residual_of(eng, prob), _residual_of(orc, prob)
        got.update(residual=r_eng, residual_ratio=r_eng / r_orc)
        assert r_eng <= RESIDUAL_FACTOR * r_orc, (it, r_eng, r_orc)
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), float(v))
        for name in ('alpha', 'beta', 'tau', 'eta', 'z', 'xz'):
            eng.set(name, orc.get(name))
    assert eng.stats()['fused_fallbacks'] == 0
    eng.close()
    print(form, env or '', 'worst over %d iterations:' % n_iter, {k: float('%.2e' % v) for k, v in worst.items()})
    return worst


@pytest.mark.parametrize('name, form', [(n, f) for n in ('sell8', 'sell16', 'hub', 'wide_ell', 'one_isolated') for f in LADDER[n]])
def test_lockstep_with_the_oracle_in_every_form(oracle, monkeypatch, name, form):
    """True SELL bases with the 8-wide and the 16-wide window of k_iter, rows of 46 off-diagonals (k_minres's tail loop past
    its prefetch window under SELL bases), an ELL layout of width 24 (the same loop under arithmetic bases) and a site without
    neighbours: every conditional of three iterations against the oracle, whose solve sensitivity on these cases is at most
    8e-8 (hub; 1e-10 and below on the others), and the engine's own residual within twice the oracle's (the oracle's shrinks
    by at most 1.95 in its last step).  Measured deviation of xz, the same in every form: sell8 7e-13, sell16 1e-10, wide_ell
    6e-14, one_isolated 2e-13, and hub 9e-8 -- the one case above the plain 5e-8, held by the sensitivity rule at 1.6e-7."""
    prob = G.survey(G.graph(name), G.SEEDS[name])
    _lockstep_graph(oracle, monkeypatch, prob, _random_start(prob, G.SEEDS[name]), form)


@pytest.mark.parametrize('name, form', [(n, f) for n in G.EMPTY for f in LADDER[n]])
def test_slices_of_width_zero_in_every_form(oracle, monkeypatch, name, form):
    """Sixty-four aligned sites without neighbours as the first, an inner and the last slice (under SELL bases the kernels
    then read the spare slots behind the arrays).  The oracle's own iterate lies 3e-2 to 1e-1 from the closed form
    x_i = rhs_i / omega_i, z_i = 1 / omega_i at these sites (the solve stops at a residual of 2e-3 to 4e-3 of ||b||), so the
    device is held to 10 x the oracle's deviation of the same iteration, not to 1e-4 (test_layout_graphs_cpu.py).  Measured:
    the device's deviation equals the oracle's to three digits, its xz lies 4e-4 (first), 7e-8 (middle), 5e-4 (last) from the
    oracle's with equal step counts, and its residual equals the oracle's."""
    prob = G.survey(G.graph(name), G.SEEDS[name])
    _lockstep_graph(oracle, monkeypatch, prob, _random_start(prob, G.SEEDS[name]), form, empty=True)


def _run_chains(monkeypatch, prob, keys, starts, form, env=None, iters=25, eager_step=False):
    eng = _engine(monkeypatch, prob, keys, form, env)
    for c, st in enumerate(starts):
        eng.set_start(c, **st)
    rec = eng.run(iters, 0)
    if eager_step:
        eng.step()                                         # eager stepping through the same kernel
    state = [tuple(eng.get(name, c) for name in ('eta', 'xz', 'z', 'minres_itn')) for c in range(len(keys))]
    st = eng.stats()
    eng.close()
    assert st['fused_fallbacks'] == 0, (form, env)
    return rec, state, st['krylov_mean']


def _assert_same_bits(got, ref):
    for u, v in zip(got[0], ref[0]):
        assert np.array_equal(u, v)
    for su, sv in zip(got[1], ref[1]):
        for u, v in zip(su, sv):
            assert np.array_equal(u, v)
    assert got[2] == ref[2]


@pytest.mark.parametrize('name', ['sell8', 'sell16', 'one_isolated'] + list(G.EMPTY))
def test_fused_forms_are_bit_identical_to_launch_per_step(monkeypatch, name):
    """Two chains, 25 iterations in one call, in each form of the ladder: records, eta, xz, z, every solve's iteration count
    and their mean equal those of the launch-per-step run, with no fallback (test_gpu_parity's
    test_persistent_solve_is_bit_identical_to_launch_per_step, on SELL bases)."""
    prob = G.survey(G.graph(name), G.SEEDS[name])
    keys = [KEY + 7 * c for c in range(2)]
    starts = [_random_start(prob, 11 + c) for c in range(2)]
    out = {form: _run_chains(monkeypatch, prob, keys, starts, form) for form in LADDER[name]}
    for form in ('xcd_local', 'any_placement'):
        _assert_same_bits(out[form], out['launch_per_step'])


def _queen(rows, cols, chains):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(rows, cols, visits=3, p=2, q=2, random_state=5)
    prob = FlatProblem(Q, W, X, y)
    return prob, [KEY + 7 * c for c in range(chains)], [_random_start(prob, 11 + c) for c in range(chains)]


@pytest.mark.parametrize('form', ['xcd_local', 'launch_per_step'])
def test_no_dia_gives_the_same_bits(monkeypatch, form):
    """OCC_NO_DIA=1 keeps a lattice's Q in stored slots where the default takes the diagonal form (k_iter, k_minres): the same
    neighbours in the same order with the same coefficients -- 30 x 40 queen lattice, 2 chains, 25 iterations, bit for bit."""
    prob, keys, starts = _queen(30, 40, 2)
    ref = _run_chains(monkeypatch, prob, keys, starts, form)
    alt = _run_chains(monkeypatch, prob, keys, starts, form, env={'OCC_NO_DIA': '1'})
    _assert_same_bits(alt, ref)


# ---- the general (non-diagonal) tile form k_tiles<8, T, 0> --------------------------------------------------------
def _tiles_against_steps(monkeypatch, prob, chains, T, iters=20):
    keys = [KEY + 7 * c for c in range(chains)]
    starts = [_random_start(prob, 11 + c) for c in range(chains)]
    tiles = _run_chains(monkeypatch, prob, keys, starts, 'tiles', {'OCC_FORCE_TILES': T}, iters, eager_step=True)
    eng_steps = _run_chains(monkeypatch, prob, keys, starts, 'launch_per_step', {'OCC_FORCE_TILES': T}, iters, eager_step=True)
    _assert_same_bits(tiles, eng_steps)


@pytest.mark.parametrize('T', ['1', '2', '4'])
def test_general_tile_form_on_a_weighted_lattice(monkeypatch, T):
    """61 x 67 queen lattice with random edge weights: ELL 8, no diagonal form, 16 tiles with a ragged last one; one, two and
    four tiles per workgroup, 2 chains, 20 iterations in one call and one eager step: bit for bit the launch-per-step
    kernels in the same layout (test_gpu_parity's test_tile_looping_persistent_solve_is_bit_identical_to_launch_per_step takes
    the diagonal form throughout)."""
    _tiles_against_steps(monkeypatch, G.survey(G.graph('weighted_queen'), G.SEEDS['weighted_queen']), 2, T)


@pytest.mark.parametrize('T', ['1', '3'])
def test_general_tile_form_on_sell_bases_with_neighbours_anywhere(monkeypatch, T):
    """4 400 sites (18 tiles, n no multiple of 256) on a ring, every site with a chord to a random site anywhere -- the
    workgroups that hold a workgroup's neighbours span all bands, most lines of the exchange buffer are stored
    write-through -- and an inner slice of 64 sites without neighbours: 1 chain, bit for bit launch-per-step."""
    _tiles_against_steps(monkeypatch, G.survey(G.graph('sell_tiles'), G.SEEDS['sell_tiles']), 1, T)


def test_general_tile_form_equals_the_diagonal_tile_form(monkeypatch):
    """The unweighted 61 x 67 lattice, two tiles per workgroup: k_tiles<8, 2, 0> (OCC_NO_DIA=1) against k_tiles<8, 2, 1>."""
    prob, keys, starts = _queen(61, 67, 2)
    ref = _run_chains(monkeypatch, prob, keys, starts, 'tiles', {'OCC_FORCE_TILES': '2'}, 20, eager_step=True)
    alt = _run_chains(monkeypatch, prob, keys, starts, 'tiles', {'OCC_FORCE_TILES': '2', 'OCC_NO_DIA': '1'}, 20, eager_step=True)
    _assert_same_bits(alt, ref)


@pytest.mark.parametrize('name, T', [('weighted_queen', '2'), ('sell_tiles', '1')])
def test_general_tile_form_lockstep_with_the_oracle(oracle, monkeypatch, name, T):
    """Three lock-step iterations of the tile kernel against the oracle: the weighted lattice under test_gpu_parity's
    tolerances (solve sensitivity 1e-13), the ring with its isolated slice under the rule for empty slices (there the
    oracle's iterate lies 2e-1 to 3e-1 from the closed form at the isolated sites)."""
    prob = G.survey(G.graph(name), G.SEEDS[name])
    _lockstep_graph(oracle, monkeypatch, prob, _random_start(prob, G.SEEDS[name]), 'tiles', {'OCC_FORCE_TILES': T}, empty=name == 'sell_tiles')
