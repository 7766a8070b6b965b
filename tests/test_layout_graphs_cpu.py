"""The graphs of tests/_layout_graphs.py on the CPU: which branch of the layout and which form of the planner each one
reaches (pinned: tests/test_gpu_layout_graphs.py relies on it), the oracle's joint solve against scipy's ``minres`` on graphs
with a site without neighbours and with two components, one engine lifecycle on the CPU build of the C ABI, and the
figures that the GPU tests' bounds rest on, from the oracle alone: the sensitivity of every compared solve (at or below 1e-5),
how much the residual shrinks in the oracle's last MINRES step (below 2), and how far the oracle's own iterate lies from the
closed form at a site without neighbours."""
import numpy as np
import pytest
from scipy import sparse

from . import _layout_graphs as G
from .test_cpu_abi import cpu_abi  # noqa: F401  (fixture)
from .test_gpu_parity import KEY, _random_start, _rel, _solve_sensitivity
from .test_layout_cpu import lib, layout, restate, ARRAYS  # noqa: F401  (lib: fixture)
from .test_plan_cpu import FORM_STEPS, FORM_TILES, FORM_XCD, planner  # noqa: F401  (planner: fixture)

# name: (ell_w, wmax, diagonals, smallest slice width), (form, window, ladder) of 2 chains
TABLE = {
    'sell8': ((0, 8, 0, 3), (FORM_XCD, 8, [2, 1, 0])),
    'sell16': ((0, 15, 0, 3), (FORM_XCD, 16, [2, 1, 0])),
    'hub': ((0, 46, 0, 7), (FORM_STEPS, 16, [0])),
    'wide_ell': ((24, 24, 0, 24), (FORM_STEPS, 16, [0])),
    'one_isolated': ((0, 8, 0, 3), (FORM_XCD, 8, [2, 1, 0])),
    'empty_last': ((0, 8, 0, 0), (FORM_XCD, 8, [2, 1, 0])),
    'empty_first': ((0, 8, 0, 0), (FORM_XCD, 8, [2, 1, 0])),
    'empty_middle': ((0, 8, 0, 0), (FORM_XCD, 8, [2, 1, 0])),
}
# the tile cases: layout facts, chains, {forced T: G}
TILES = {
    'weighted_queen': ((8, 8, 0, 8), 2, {1: 16, 2: 8, 4: 4}),
    'sell_tiles': ((0, 8, 0, 0), 1, {1: 18, 3: 6}),
}
LOCKSTEP = ('sell8', 'sell16', 'hub', 'wide_ell', 'one_isolated', 'weighted_queen')  # held to the oracle's xz: the sensitivity rule applies
SENSITIVITY_CAP = 1e-5


def _as_layout_problem(prob):
    Q = prob.Q
    return dict(indptr=Q.indptr, indices=Q.indices, data=Q.data, X=prob.X, W=prob.W, y=prob.y, site_id=prob.site_id, site_ptr=prob.site_ptr,
                a_mu=prob.a_mu, a_prec=prob.a_prec, b_mu=prob.b_mu, b_prec=prob.b_prec)


def _facts(lib, name):
    pr = _as_layout_problem(G.survey(G.graph(name), G.SEEDS[name]))
    got, want = layout(lib, pr), restate(pr)
    for a in ARRAYS:
        assert np.array_equal(got[a], np.asarray(want[a], dtype=float)), (name, a)
    width = np.diff(got['sell_ptr']) / 64
    return (int(got['ell_w'][0]), int(got['wmax'][0]), len(got['dia_off']), int(width.min())), len(width)


@pytest.mark.parametrize('name', list(TABLE))
def test_each_graph_reaches_its_branch(lib, planner, name):
    facts, nslice = _facts(lib, name)
    assert facts == TABLE[name][0]
    Q = G.graph(name)
    assert 640 <= Q.shape[0] <= 700 and nslice in (10, 11)
    form, window, ladder = TABLE[name][1]
    prob = G.survey(Q, G.SEEDS[name])
    pl = planner(prob.n, 2, rows=prob.R, wmax=facts[1], dia=facts[2] > 0)
    assert (pl.form, pl.iter_window, list(pl.ladder_form)[:pl.n_ladder]) == (form, window, ladder)
    iso = G.isolated_sites(Q)
    assert len(iso) == {'one_isolated': 1, 'empty_last': 64, 'empty_first': 64, 'empty_middle': 64}.get(name, 0)
    if name in G.EMPTY:
        assert iso[0] % 64 == 0 and np.array_equal(iso, iso[0] + np.arange(64))
        assert iso[0] // 64 == {'empty_first': 0, 'empty_middle': 4, 'empty_last': nslice - 1}[name]


@pytest.mark.parametrize('name', list(TILES))
def test_the_tile_graphs_take_the_general_tile_form(lib, planner, name):
    """Weighted 61 x 67 queen lattice: ELL 8 without a diagonal form, 16 tiles of 256 sites, the last one ragged; the
    4 400-site ring with chords anywhere: true SELL bases, one inner slice of width 0, 18 tiles, n no multiple of 256.  Forced
    tiles give form 3 with the stated T and G."""
    want, chains, forced = TILES[name]
    facts, nslice = _facts(lib, name)
    assert facts == want
    Q = G.graph(name)
    n = Q.shape[0]
    prob = G.survey(Q, G.SEEDS[name])
    assert n % 256 != 0 and -(-n // 256) == forced[1]
    for T, Gr in forced.items():
        pl = planner(n, chains, rows=prob.R, wmax=facts[1], dia=False, force_tiles=T)
        assert (pl.form, pl.tiles_T, pl.tiles_G, pl.tpb) == (FORM_TILES, T, Gr, 256)
        assert list(pl.ladder_form)[:pl.n_ladder] == [FORM_TILES, FORM_STEPS]
    if name == 'sell_tiles':
        iso = G.isolated_sites(Q)
        assert len(iso) == 64 and iso[0] % 64 == 0 and 0 < iso[0] // 64 < nslice - 1
        # most sites have a neighbour in another XCD's band of tiles (T = 1: bands of ceil(18 / 8) = 3 tiles)
        coo = Q.tocoo()
        far = (coo.row // 768) != (coo.col // 768)
        assert np.unique(coo.row[far]).size > 0.7 * n


def test_the_unweighted_queen_lattices_have_the_diagonal_form(lib):
    """What OCC_NO_DIA=1 switches off on the 30 x 40 and 61 x 67 lattices of the GPU tests: ELL 8 WITH the diagonal form."""
    from occuspytial_amd.utils import rand_precision_mat
    for shape in ((30, 40), (61, 67)):
        Q = rand_precision_mat(*shape, max_neighbors=8).astype(float).tocsr()
        n = Q.shape[0]
        one = np.ones((1, 1))
        got = layout(lib, dict(indptr=Q.indptr, indices=Q.indices, data=Q.data, X=np.zeros((n, 1)), W=np.zeros((0, 1)), y=np.zeros(0),
                               site_id=np.zeros(0), site_ptr=np.zeros(1), a_mu=one[0], a_prec=one, b_mu=one[0], b_prec=one))
        assert (int(got['ell_w'][0]), len(got['dia_off'])) == (8, 8)


# ---- the oracle's joint solve on rows without a stored diagonal --------------------------------------------------
def _scipy_solve(prob, orc, x0):
    from scipy.sparse.linalg import minres
    rhs, om, tau = orc.get('rhs'), orc.get('omega_b'), float(orc.get('tau'))
    A = sparse.block_diag([tau * prob.Q + sparse.diags(om)] * 2).tocsr()
    cnt = [0]
    x, info = minres(A, np.concatenate([rhs, np.ones(prob.n)]), x0=np.array(x0), rtol=1e-5, maxiter=10 * prob.n,
                     callback=lambda xk: cnt.__setitem__(0, cnt[0] + 1))
    assert info == 0
    return x, cnt[0]


@pytest.mark.parametrize('name', ['one_isolated', 'two_components'])
def test_oracle_solve_equals_scipy_minres(oracle, name):
    """Three oracle iterations from _random_start; after each, ``minres_joint`` on the system the oracle built against
    ``scipy.sparse.linalg.minres`` on blockdiag(tau Q + diag(omega))^2, right-hand side [rhs; 1], the same x0, rtol 1e-5:
    the same number of steps, and the solutions within 1e-12 relative (measured 2e-13 at worst).  Before the oracle added omega on a
    row WITHOUT a stored diagonal (a site without neighbours) it failed on one_isolated: 0.9 relative, 36 MINRES steps where scipy takes 21."""
    Q = G.graph(name)
    assert Q.nnz == Q.count_nonzero() and len(G.isolated_sites(Q)) == (1 if name == 'one_isolated' else 0)
    prob = G.survey(Q, G.SEEDS[name])
    orc = oracle.OracleSampler(prob, KEY)
    orc.set_start(**_random_start(prob, G.SEEDS[name]))
    for it in range(3):
        x0 = orc.get('xz')
        orc.step()
        mine, info, itn, _ = oracle.minres_joint(prob.Q, orc.get('omega_b'), float(orc.get('tau')), orc.get('rhs'), x0=x0)
        assert info == 0 and np.array_equal(mine, orc.get('xz')) and itn == int(orc.get('minres_itn'))
        ref, steps = _scipy_solve(prob, orc, x0)
        print(name, it, 'steps', itn, steps, 'relative difference %.1e' % _rel(mine, ref))
        assert itn == steps
        assert _rel(mine, ref) < 1e-12


def test_engine_lifecycle_on_the_cpu_abi_with_an_isolated_site(cpu_abi):
    from occuspytial_amd._engine import Engine
    prob = G.survey(G.graph('one_isolated'), G.SEEDS['one_isolated'])
    eng = Engine(prob, [KEY])
    eng.set_start(0, **_random_start(prob, 3))
    a, b, t = eng.run(5, 0)
    eta = eng.get('eta')
    for v in (a, b, t, eta, eng.get('xz'), eng.get('omega_b'), eng.get('rhs')):
        assert np.all(np.isfinite(v))
    assert a.shape == (1, 5, 2) and np.all(t > 0)
    assert abs(eta.sum()) <= 1e-8 * np.abs(eta).sum()
    eng.close()


# ---- what the GPU tests' bounds rest on, from the oracle alone ---------------------------------------------------
@pytest.fixture(scope='module')
def oracle_figures(oracle):
    """Per case: [(sensitivity, residual, residual one step earlier / residual, closed-form deviation)] of three iterations."""
    out = {}
    for name in list(TABLE) + list(TILES):
        prob = G.survey(G.graph(name), G.SEEDS[name])
        orc = oracle.OracleSampler(prob, KEY)
        orc.set_start(**_random_start(prob, G.SEEDS[name]))
        rows = []
        for it in range(3):
            x0 = orc.get('xz')
            orc.step()
            tau, om, rhs, xz, itn = float(orc.get('tau')), orc.get('omega_b'), orc.get('rhs'), orc.get('xz'), int(orc.get('minres_itn'))
            sens = _solve_sensitivity(orc, prob, x0) if name in LOCKSTEP else 0.0
            last = G.residual(prob.Q, tau, om, rhs, xz)
            before = G.residual(prob.Q, tau, om, rhs, oracle.minres_joint(prob.Q, om, tau, rhs, x0=x0, maxiter=itn - 1)[0])
            dev = G.closed_form_deviation(prob.Q, om, rhs, xz) if len(G.isolated_sites(prob.Q)) else 0.0
            rows.append((sens, last, before / last, dev))
        print('%-15s sensitivity %.1e  residual %.1e  one step earlier / last %.2f  closed form %.1e' % ((name,) + tuple(np.max(rows, axis=0))))
        out[name] = rows
    return out


def test_solve_sensitivity_of_the_lockstep_cases_stays_below_the_cap(oracle_figures):
    """test_gpu_parity's rule loosens xz, eta and beta to twice _solve_sensitivity: so that it cannot hide a wrong
    coefficient, the sensitivity of every compared iteration of every case that is held to the oracle's xz is computed here,
    from the oracle alone, and capped (measured at these seeds: sell8 8e-13, sell16 1e-10, hub 8e-8, wide_ell 1e-13,
    one_isolated 1e-12, weighted_queen 1e-13)."""
    for name in LOCKSTEP:
        for sens, *_ in oracle_figures[name]:
            assert sens <= SENSITIVITY_CAP, (name, sens)


def test_one_minres_step_less_leaves_less_than_twice_the_residual(oracle_figures):
    """The GPU tests hold the device's residual to 2 x the oracle's: the device may stop one MINRES step apart where the sums
    are ordered differently.  The oracle's residual one step before its last is below twice its last on every case
    (measured: 1.95 at worst, on wide_ell), so the factor stays 2."""
    for name, rows in oracle_figures.items():
        for _, last, ratio, _ in rows:
            assert 1.0 <= ratio < 2.0 and last < 1e-2, (name, ratio, last)


def test_the_oracle_itself_is_far_from_the_closed_form_at_isolated_sites(oracle_figures):
    """A site without neighbours has x_i = rhs_i / omega_i, z_i = 1 / omega_i exactly, but the solve stops on scipy's test
    ||r|| <= rtol ||A|| ||x||, which leaves a residual of 2e-3 to 5e-3 of ||b||: the oracle's own iterate lies 3e-2 to 1e-1
    (empty_*), 2e-1 to 3e-1 (sell_tiles) from the closed form there -- nowhere near a factor 10 inside 1e-4.  The GPU tests
    therefore hold the device to 10 x the ORACLE's deviation of the same iteration, not to 1e-4."""
    for name in G.EMPTY + ('sell_tiles',):
        for *_, dev in oracle_figures[name]:
            assert dev > 1e-5, (name, dev)
