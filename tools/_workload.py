"""The engine a timing tool measures: a lattice problem of make_lattice_problem, one chain per generator of
chain_generators(seed, chains), every chain at its default start."""


def lattice_engine(rows, cols, chains, edit=None, seed=10, **lattice_kw):
    """-> (prob, eng).  ``edit(W, y)``, if given, changes the visits before the problem is built (withholding sites)."""
    from occuspytial_amd._engine import Engine
    from occuspytial_amd._problem import FlatProblem, chain_generators, default_start
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(rows, cols, **lattice_kw)
    if edit is not None:
        edit(W, y)
    prob = FlatProblem(Q, W, X, y)
    gens = chain_generators(seed, chains)
    eng = Engine(prob, [int(g.bit_generator.random_raw()) for g in gens])
    for i, g in enumerate(gens):
        st = default_start(g, prob)
        eng.set_start(i, st['alpha'], st['beta'], st['tau'], st['eta'])
    return prob, eng
