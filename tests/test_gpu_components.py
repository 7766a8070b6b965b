"""Sum-to-zero per connected component on the device (``constraint='component'``; csrc/occ_comp.hpp).

The graphs are tests/_components_graphs.py's: 34 sites in five components (two of them single sites) and 360 sites in three,
whose components cross the solve's 64-site slices and 256-site tiles.  Nothing here is compared with the device itself: the
solve is held against scipy's MINRES on the same block system, the projection against numpy on the solve the engine
returned, the sampler as a whole against a dense numpy restatement (tests/_components_reference.py) whose draws are
stored in tests/golden/components34.npz.
"""
import os

import numpy as np
import pytest
from scipy import sparse
from scipy.sparse.linalg import minres

from . import _components_graphs as G

pytestmark = pytest.mark.gpu

KEY = 0x7C0FFEE5EEDC0DE5
FORM_KEYS = ('OCC_NO_PERSISTENT', 'OCC_FORCE_KRYLOV_CAP', 'OCC_FORCE_TILES', 'OCC_NO_TILES', 'OCC_NO_XCD_LOCAL', 'OCC_EAGER_ONLY', 'OCC_EVENT_SYNC',
             'OCC_STREAM_EVENTS', 'OCC_CU_SPLIT', 'OCC_NO_SIDE_STREAM')

# Measured worst case of the device's solve against scipy's MINRES (this file's test 1 on an MI355X): relative max-norm
# deviation of [x z], the iteration counts being equal.  The test asserts twice these, floor 2e-14 (tests/test_gpu_golden.py:
# _solve_bounds).  The 34-site system is solved in 23 steps, close to the number of its distinct eigenvalues: the Lanczos
# recurrence has all but exhausted the Krylov space there, and the device's scalar recurrence (one reciprocal square root per
# divisor) and scipy's then part by far more than on the 360-site one -- at a solve tolerance of 1e-5.
MEASURED_SOLVE = {'small': 4.2e-9, 'large': 4.8e-13, 'heavy': 1.1e-13}


def _problem(g, constraint):
    from occuspytial_amd._problem import FlatProblem
    return FlatProblem(g['Q'], g['W'], g['X'], g['y'], constraint=constraint)


def _start(prob, seed, labels=None):
    from occuspytial_amd.graph import centre
    rng = np.random.default_rng(seed)
    eta = rng.standard_normal(prob.n)
    eta = centre(eta, labels) if labels is not None else eta - eta.mean()
    return dict(alpha=rng.standard_normal(prob.q) * 0.5, beta=rng.standard_normal(prob.p) * 0.5, tau=0.9, eta=eta)


def _clear(monkeypatch):
    for k in FORM_KEYS:
        monkeypatch.delenv(k, raising=False)


def sum_bound(eta, sites):
    """|sum of eta over a component| <= 1e-12 n_c max(1, max |eta|): float64 rounding with a margin of a few thousand."""
    return 1e-12 * sites.size * max(1.0, float(np.abs(eta[sites]).max()))


def assert_centred(eta, labels):
    for c in np.unique(labels):
        sites = np.flatnonzero(labels == c)
        assert abs(float(eta[sites].sum())) <= sum_bound(eta, sites), (int(c), float(eta[sites].sum()))


def projection_ulps(xz, eta, labels, single):
    """The worst distance of eta from the numpy projection of [x z] (component sums in the documented order), in ulp of
    |x_i| + |a_c z_i|, away from the single sites."""
    n = labels.size
    x, z = xz[:n], xz[n:]
    sums = G.component_sums(xz, labels)
    a = np.array([-sums[int(c)][0] / sums[int(c)][1] for c in labels])
    ulp = np.spacing(np.abs(x) + np.abs(a * z))
    return float((np.abs(eta - (x + a * z)) / ulp)[~single].max())


GRAPHS = {'small': G.small, 'large': G.large, 'heavy': G.heavy}   # heavy: a component of more than 64 chunks (a wave's sum)


def _cond_eta(g, constraint, seed):
    """One injected eta conditional -> everything test 1 looks at."""
    from occuspytial_amd._engine import Engine
    prob = _problem(g, constraint)
    n = prob.n
    rng = np.random.default_rng(seed)
    st = _start(prob, seed + 1, g['labels'])
    om = rng.uniform(0.05, 0.25, n)
    eps1 = rng.standard_normal(n)
    prior = 0.5 * (g['Q'] @ rng.standard_normal(n))   # in the range of Q: zero at a site without neighbours
    x0 = 0.1 * rng.standard_normal(2 * n)
    eng = Engine(prob, [KEY])
    try:
        eng.set_start(0, st['alpha'], st['beta'], st['tau'], st['eta'])
        eng.set('z', prob.z0)
        eng.set('xz', x0)
        rhs, xz, eta, itn = eng.cond_eta(om, eps1, prior)
    finally:
        eng.close()
    return dict(prob=prob, st=st, om=om, eps1=eps1, prior=prior, x0=x0, rhs=rhs, xz=xz, eta=eta, itn=itn)


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_eta_conditional_under_component_constraints(name):
    """Test 1: right-hand side, solve and iteration count against scipy's MINRES with the reference's settings
    (logit.py:80-87: the 2n block system, the warm start, default tolerance); eta against the numpy projection of the engine's
    own [x z] with the component sums in the documented order; every component centred; the global constraint is not."""
    g = GRAPHS[name]()
    r = _cond_eta(g, 'component', 11)
    prob, st, n, labels = r['prob'], r['st'], g['n'], g['labels']
    tau = st['tau']
    rhs = (prob.z0 - 0.5) - r['om'] * (prob.X @ st['beta']) + np.sqrt(r['om']) * r['eps1'] + np.sqrt(tau) * r['prior']
    print(f'{name}: rhs deviation {np.abs(r["rhs"] - rhs).max() / np.abs(rhs).max():.3e}')
    assert np.abs(r['rhs'] - rhs).max() <= 1e-12 * np.abs(rhs).max()
    lam = (tau * g['Q'] + sparse.diags(r['om'])).tocsc()
    block = sparse.block_diag((lam, lam), format='csc')
    steps = []
    ref, fail = minres(block, np.concatenate([rhs, np.ones(n)]), x0=r['x0'], callback=lambda xk: steps.append(1))
    assert fail == 0
    dev = np.abs(r['xz'] - ref).max() / np.abs(ref).max()
    print(f'{name}: [x z] against scipy {dev:.3e}, iterations {r["itn"]} / {len(steps)}')
    assert r['itn'] == len(steps)
    assert dev <= max(2.0 * MEASURED_SOLVE[name], 2e-14)
    # the projection, from the engine's own [x z]
    eta = r['eta']
    single = np.isin(np.arange(n), g['singles'])
    worst = projection_ulps(r['xz'], eta, labels, single)
    print(f'{name}: eta against the numpy projection, worst {worst:.2f} ulp of |x| + |a z|')
    assert worst <= 4.0
    assert np.all(eta[single] == 0.0) and not np.any(np.signbit(eta[single]))
    assert_centred(eta, labels)
    # the same call under the global constraint: centred over all sites, not per component
    glob = _cond_eta(g, 'global', 11)['eta']
    excess = max(abs(float(glob[labels == c].sum())) / sum_bound(glob, np.flatnonzero(labels == c)) for c in np.unique(labels))
    print(f'{name}: under the global constraint the worst component sum is {excess:.3e} times the bound')
    assert excess > 1e6


def _run_form(monkeypatch, g, env, iters, eager):
    from occuspytial_amd._engine import Engine
    _clear(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    prob = _problem(g, 'component')
    eng = Engine(prob, [KEY, KEY + 7])
    try:
        for c in range(2):
            s = _start(prob, 21 + c, g['labels'])
            eng.set_start(c, s['alpha'], s['beta'], s['tau'], s['eta'])
            eng.set('z', prob.z0, c)
        if eager:
            for _ in range(iters):
                eng.step()
        else:
            eng.run(iters, 0)
        st = eng.stats()
        state = [tuple(np.atleast_1d(eng.get(nm, c)) for nm in ('eta', 'alpha', 'beta', 'tau', 'z', 'xz')) for c in range(2)]
    finally:
        eng.close()
    return state, st


def _same(a, b):
    return all(np.array_equal(u, v) for ca, cb in zip(a, b) for u, v in zip(ca, cb))


def test_every_form_gives_the_same_bits(monkeypatch):
    """Test 2: 12 iterations on the 360-site graph behind every form of the solve -- the default form (k_iter), one launch per
    MINRES step, forced k_tiles, an eager occ_step sequence.  The solve itself adds its MINRES sums per 64-site slice or, in
    the tile layout (OCC_FORCE_TILES), per group of 256-site tiles, and a layout's forms agree bit for bit with each other
    (tests/test_gpu_parity.py); the correction pass adds in ONE order whatever the form, so each layout's forms must still
    agree bit for bit, eager stepping included, and every component of every final eta is centred."""
    g = G.large()
    runs = {
        'default': _run_form(monkeypatch, g, {}, 12, False),
        'steps': _run_form(monkeypatch, g, {'OCC_NO_PERSISTENT': '1'}, 12, False),
        'eager': _run_form(monkeypatch, g, {}, 12, True),
        'tiles': _run_form(monkeypatch, g, {'OCC_FORCE_TILES': '1'}, 12, False),
        'tiles_steps': _run_form(monkeypatch, g, {'OCC_FORCE_TILES': '1', 'OCC_NO_PERSISTENT': '1'}, 12, False),
        'tiles_eager': _run_form(monkeypatch, g, {'OCC_FORCE_TILES': '1'}, 12, True),
        # captured graphs of too few Krylov launches: solves are carried into the next replay, whose pass must leave them alone
        'carry': _run_form(monkeypatch, g, {'OCC_NO_PERSISTENT': '1', 'OCC_FORCE_KRYLOV_CAP': '4'}, 12, False),
    }
    forms = {k: v[1]['persistent_solve'] for k, v in runs.items()}
    print('forms', forms, 'across the two layouts:', _same(runs['default'][0], runs['tiles'][0]))
    assert forms['default'] in (1, 2) and forms['steps'] == 0 and forms['tiles'] == 3 and forms['tiles_steps'] == 0, forms
    assert runs['tiles'][1]['threads_per_block'] == 256 and runs['tiles_steps'][1]['threads_per_block'] == 256
    for k in ('eager', 'tiles_eager'):
        assert runs[k][1]['eager_iterations'] == 12 and runs[k][1]['graph_launches'] == 0, runs[k][1]
    for k in ('default', 'steps', 'tiles', 'tiles_steps'):
        assert runs[k][1]['iterations'] == 12 and runs[k][1]['fused_fallbacks'] == 0, runs[k][1]
    assert _same(runs['default'][0], runs['steps'][0]) and _same(runs['default'][0], runs['eager'][0])
    assert runs['carry'][1]['persistent_solve'] == 0 and runs['carry'][1]['stalls'] > 0, runs['carry'][1]
    assert _same(runs['default'][0], runs['carry'][0])
    assert _same(runs['tiles'][0], runs['tiles_steps'][0]) and _same(runs['tiles'][0], runs['tiles_eager'][0])
    # what holds across the two layouts: every final eta is the projection of its own run's last [x z], the component sums
    # added in the one documented order, and every component is centred
    single = np.isin(np.arange(g['n']), g['singles'])
    for state, _ in runs.values():
        for eta, *_, xz in state:
            assert_centred(eta, g['labels'])
            assert eta[g['singles'][0]] == 0.0
            assert projection_ulps(xz, eta, g['labels'], single) <= 4.0


def test_component_of_more_than_64_chunks_in_captured_graphs_and_steps():
    """The wave branch of the second level (a mainland of 2 597 sites = 82 chunks) behind the fused solve in captured graphs
    and in eager steps: the same bits, every final eta the numpy projection of its own [x z] in the documented order -- lane l
    adds the chunks l, l + 64, ..., then the wave sum's tree -- and every component centred.  (Test 1 holds the same graph's
    injected conditional to scipy.)"""
    from occuspytial_amd._engine import Engine
    g = G.heavy()
    prob = _problem(g, 'component')
    single = np.isin(np.arange(g['n']), g['singles'])
    out = []
    for eager in (False, True):
        eng = Engine(prob, [KEY, KEY + 7])
        try:
            for c in range(2):
                s = _start(prob, 61 + c, g['labels'])
                eng.set_start(c, s['alpha'], s['beta'], s['tau'], s['eta'])
                eng.set('z', prob.z0, c)
            if eager:
                for _ in range(6):
                    eng.step()
            else:
                eng.run(6, 0)
                assert eng.stats()['graph_launches'] > 0
            out.append([(eng.get('eta', c), eng.get('xz', c), eng.get('tau', c)) for c in range(2)])
        finally:
            eng.close()
    for (eta, xz, tau), (eta2, xz2, tau2) in zip(*out):
        assert np.array_equal(eta, eta2) and np.array_equal(xz, xz2) and tau == tau2
        assert projection_ulps(xz, eta, g['labels'], single) <= 4.0
        assert_centred(eta, g['labels'])
        assert eta[g['singles'][0]] == 0.0


def test_one_component_is_the_global_path():
    """Test 3: on a connected lattice 'component' is 'global': the same recorded chains and state bit for bit, the same
    launches (no label reaches the library)."""
    from occuspytial_amd._engine import Engine
    g = G.connected()
    out = {}
    for constraint in ('component', 'global'):
        prob = _problem(g, constraint)
        assert prob.n_components == 1
        eng = Engine(prob, [KEY, KEY + 7])
        try:
            for c in range(2):
                s = _start(prob, 31 + c)
                eng.set_start(c, s['alpha'], s['beta'], s['tau'], s['eta'])
                eng.set('z', prob.z0, c)
            rec = eng.run(20, 0)
            state = [tuple(np.atleast_1d(eng.get(nm, c)) for nm in ('eta', 'alpha', 'beta', 'tau', 'z', 'xz')) for c in range(2)]
            st = eng.stats()
            if constraint == 'component':
                with pytest.raises(ValueError, match='has not been set'):
                    eng.get('component_id')
            prof = eng.profile(reps=3)
        finally:
            eng.close()
        out[constraint] = (rec, state, st, prof)
    a, b = out['component'], out['global']
    assert all(np.array_equal(u, v) for u, v in zip(a[0], b[0])) and _same(a[1], b[1])
    for f in ('iterations', 'graph_launches', 'eager_iterations', 'krylov_total', 'solves', 'persistent_solve', 'iter_kernel_launches',
              'n_blocks_sites', 'threads_per_block'):
        assert a[2][f] == b[2][f], f
    assert {k: v['launches'] for k, v in a[3].items()} == {k: v['launches'] for k, v in b[3].items()}


def _sampler(g, constraint='component', **kw):
    from occuspytial_amd import LogitICARGibbs
    return LogitICARGibbs(g['Q'], g['W'], g['X'], g['y'], random_state=5, constraint=constraint, **kw)


def test_resume_continues_bit_for_bit():
    """Test 4a: sample(40, burnin=10) then resume(20) equals one call of 60 under 'component'."""
    g = G.small()
    one = _sampler(g).sample(60, burnin=10, chains=2, progressbar=False)
    s = _sampler(g)
    head = s.sample(40, burnin=10, chains=2, progressbar=False)
    tail = s.resume(s.checkpoint(), 20, progressbar=False)
    for name in ('alpha', 'beta', 'tau'):
        assert np.array_equal(np.concatenate([head[name], tail[name]], axis=1), one[name]), name
    assert_centred(s.state.eta, g['labels'])


def test_group_of_two_devices_gives_each_chain_its_bits():
    """Test 4b: a two-handle EngineGroup sets the labels on every handle: each chain's bits are the single handle's."""
    from occuspytial_amd import _lib
    from occuspytial_amd._engine import Engine, EngineGroup
    if _lib.load().occ_device_count() < 2:
        pytest.skip('needs two devices')
    g = G.large()
    prob = _problem(g, 'component')
    keys = [KEY, KEY + 7]
    starts = [_start(prob, 41 + c, g['labels']) for c in range(2)]
    out = []
    for eng in (Engine(prob, keys), EngineGroup(prob, keys, [0, 1])):
        try:
            for c in range(2):
                eng.set_start(c, starts[c]['alpha'], starts[c]['beta'], starts[c]['tau'], starts[c]['eta'])
                eng.set('z', prob.z0, c)
            rec = eng.run(12, 0)
            out.append((rec, [eng.get('eta', c) for c in range(2)]))
            if isinstance(eng, EngineGroup):
                for e in eng.engines:
                    assert np.array_equal(e.get('component_id'), g['labels'])
        finally:
            eng.close()
    assert all(np.array_equal(u, v) for u, v in zip(out[0][0], out[1][0]))
    assert all(np.array_equal(u, v) for u, v in zip(out[0][1], out[1][1]))


def test_handle_state_name(monkeypatch):
    """The C ABI's name: read back as set; refused as a whole for a bad value, after the first iteration, and by a
    reduced-rank handle with a text of its own."""
    from occuspytial_amd._engine import Engine
    from occuspytial_amd._problem import FlatProblem
    g = G.small()
    prob = _problem(g, 'global')
    eng = Engine(prob, [KEY])
    try:
        with pytest.raises(ValueError, match='has not been set'):
            eng.get('component_id')
        bad = g['labels'].astype(float)
        bad[3] = 34.0
        with pytest.raises(ValueError, match='whole numbers from 0 to n - 1'):
            eng.set('component_id', bad)
        bad[3] = 0.5
        with pytest.raises(ValueError, match='whole numbers'):
            eng.set('component_id', bad)
        with pytest.raises(ValueError, match='has not been set'):
            eng.get('component_id')
        eng.set('component_id', g['comp'].astype(float) * 3)   # any numbering
        assert np.array_equal(eng.get('component_id'), g['comp'] * 3)
        s = _start(prob, 51, g['labels'])
        eng.set_start(0, s['alpha'], s['beta'], s['tau'], s['eta'])
        eng.set('z', prob.z0)
        eng.step()
        assert_centred(eng.get('eta'), g['labels'])
        with pytest.raises(ValueError, match="before the handle's first iteration"):
            eng.set('component_id', g['labels'].astype(float))
        prof = eng.profile(reps=3)   # (its real iterations run the pass too; what it leaves is mid-solve under either mode)
        assert prof['iter']['launches'] == 3
    finally:
        eng.close()
    c = G.connected()
    rsr = FlatProblem(c['Q'], c['W'], c['X'], c['y'])
    rsr.enable_rsr(q=6)
    eng = Engine(rsr, [KEY])
    try:
        with pytest.raises(ValueError, match='carries no sum-to-zero constraint'):
            eng.set('component_id', np.zeros(c['n']))
    finally:
        eng.close()


def test_outputs_ride_along():
    """Test 6: the optional outputs work unchanged; the posterior mean of eta is exactly 0 at the single sites, and the
    labels serve as regions."""
    g = G.small()
    s = _sampler(g)
    post = s.sample(60, burnin=20, chains=2, progressbar=False, site_summaries=True, regions=g['labels'])
    assert post.sites is not None and post.regions is not None
    assert post['occupied'].shape == (2, 40, g['k'])
    eta_mean = np.asarray(post.sites.eta_mean)
    assert eta_mean.shape == (g['n'],)
    assert np.all(eta_mean[list(g['singles'])] == 0.0)
    assert np.abs(eta_mean).max() > 0.0
    assert np.all(np.asarray(post.sites.eta_sd)[list(g['singles'])] == 0.0)


def test_sampler_agrees_with_the_dense_restatement():
    """Test 5: 2 chains of 3 000 iterations (500 dropped) on the 34-site graph against the stored draws of the dense numpy
    restatement (tests/_components_reference.py: Cholesky of Lambda, the k constraints by kriging): the posterior means of
    alpha, beta and log tau agree within 4 Monte-Carlo standard errors, the restatement's own by batch means (the rule of
    DESIGN 12).  The restatement under the GLOBAL constraint lies outside that band in log tau
    (tests/test_components_cpu.py checks the stored draws for it), and so does the device here."""
    from . import _components_reference as R
    g = G.small()
    ref = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'components34.npz'))
    # (tau ~ Gamma(5, 1): the stored draws' prior, tests/golden/make_components_golden.py says why)
    hparams = {'tau_shape': float(ref['tau_shape']), 'tau_rate': float(ref['tau_rate'])}
    post = _sampler(g, hparams=hparams).sample(int(ref['size']), burnin=int(ref['burnin']), chains=2, progressbar=False)
    pairs = [(f'{nm}[{j}]', post[nm][:, :, j], ref[nm][:, :, j]) for nm in ('alpha', 'beta') for j in range(2)]
    pairs.append(('log tau', np.log(post['tau']), np.log(ref['tau'])))
    rows = []
    for name, dev, cpu in pairs:
        rows.append((name, float(dev.mean()), float(cpu.mean()), 4 * R.batch_means_mcse(cpu)))
        print('%-8s device %.4f restatement %.4f band %.4f' % rows[-1])
    for name, d, c, band in rows:
        assert abs(d - c) <= band, (name, d, c, band)
    name, d, c, band = rows[-1]
    assert abs(d - float(np.log(ref['global_tau']).mean())) > band
