"""ProbitRSRGibbs on the MI355X: the truncated-normal draws, every conditional of ten iterations in lock step with the
numpy restatement (tests/_probit_reference.py) fed the device's own variates, determinism, the reference's sampler
contract for this class (all xfail in the reference, whose sampler does not run) and a long run from the dispersed
default start that sends the reference to NaN."""
import numpy as np
import pytest

from . import _probit_reference as pr
from .test_probit_cpu import restatement_problem

pytestmark = pytest.mark.gpu

LOCS = [0.0, 1.0, 5.0, 10.0, 38.0, 40.0, 100.0, 1e3, 1e6]
STREAMS = dict(u_ob=(1, 'uniform'), n_eps=(11, 'normal'), xi=(12, 'normal'), n_beta=(5, 'normal'), u_oa=(6, 'uniform'),
               n_alpha=(7, 'normal'), u_z=(8, 'uniform'))


def _data(n=150, seed=10, p=3, q=2):
    from occuspytial_amd.utils import make_data
    return make_data(n, min_v=2, max_v=4, ns=n // 2, p=p, q=q, random_state=seed)[:4]


def _lattice(rows, cols, seed=0):
    from occuspytial_amd.utils import make_lattice_problem
    return make_lattice_problem(rows, cols, visits=3, p=3, q=2, random_state=seed)[:4]


# ------------------------------------------------------------------ draws
@pytest.mark.parametrize('kind', ['truncnorm_pos', 'truncnorm_neg'])
def test_device_truncated_normal_equals_the_restatement(kind):
    from occuspytial_amd._engine import device_draw
    loc = np.repeat(np.array(LOCS + [-v for v in LOCS[1:]]), 4096)
    key, it, stream = 0x5EED1234, 3, 1
    U = device_draw('uniform', n=loc.size, key=key, it=it, stream=stream)
    got = device_draw(kind, loc, key=key, it=it, stream=stream)
    ref = pr.tn_pos(loc, U) if kind == 'truncnorm_pos' else pr.tn_neg(loc, U)
    assert np.all(np.isfinite(got))
    assert np.all(got > 0) if kind == 'truncnorm_pos' else np.all(got < 0)
    np.testing.assert_allclose(got, ref, rtol=1e-13, atol=0)


@pytest.mark.parametrize('loc', [-40.0, -5.0, 0.0, 3.0, 40.0])
def test_device_truncated_normal_ks(loc):
    from scipy import stats
    from occuspytial_amd._engine import device_draw
    n = 1_000_000
    for kind, (a, b) in (('truncnorm_pos', (-loc, np.inf)), ('truncnorm_neg', (-np.inf, -loc))):
        x = device_draw(kind, np.full(n, loc), key=77, it=1, stream=1)
        assert np.all(np.isfinite(x))
        d, pval = stats.kstest(x, stats.truncnorm(a, b, loc=loc).cdf)
        assert pval > 1e-4, (kind, loc, d, pval)


# ------------------------------------------------------------------ lock step
def _variates(eng, chain, it, n, m, p, q, R, tau_shape):
    from occuspytial_amd._engine import device_draw
    key = eng.keys[chain]
    sizes = dict(u_ob=n, n_eps=n, xi=m, n_beta=p, u_oa=R, n_alpha=q, u_z=n)
    var = {k: device_draw(kind, n=sizes[k], key=key, it=it, stream=st) for k, (st, kind) in STREAMS.items()}
    var['gamma'] = device_draw('std_gamma', np.array([tau_shape]), key=key, it=it, stream=2)[0]
    return var


def _device_state(eng, c):
    return {k: np.atleast_1d(eng.get(k, c)) for k in ('alpha', 'beta', 'tau', 'c', 'eta', 'eps', 'z')}


def _close(name, got, ref, tol=1e-10):
    got, ref = np.atleast_1d(np.asarray(got, float)), np.atleast_1d(np.asarray(ref, float))
    scale = max(np.abs(ref).max(), 1e-300)
    err = np.abs(got - ref).max() / scale
    assert err < tol, (name, err)


def _lockstep(Q, W, X, y, m, chains, iters):
    from occuspytial_amd import ProbitRSRGibbs
    from occuspytial_amd._engine import Engine
    s = ProbitRSRGibbs(Q, W, X, y, random_state=10, q=m)
    prob = restatement_problem(s)
    P = s._problem
    samplers = [s] + [s.copy() for _ in range(chains - 1)]
    keys = [0x1000 + 7919 * c for c in range(chains)]
    eng = Engine(P, keys, device=0)
    try:
        for c, t in enumerate(samplers):
            t.__dict__['state'] = type(s.state)(**s.state.__dict__)
            t._initialize_posterior_state(None)   # the dispersed default start (theta ~ N(0, 25))
            eng.set_start(c, t.state.alpha, t.state.beta, t.state.tau, t.state.eta)
            eng.set('eps', t.state.eps, c)
            eng.set('z', P.z0, c)
        for k in range(iters):
            before = [_device_state(eng, c) for c in range(chains)]
            eng.step()
            for c in range(chains):
                var = _variates(eng, c, k, P.n, m, P.p, P.q, P.R, P.tau_shape)
                st = dict(before[c], tau=float(before[c]['tau'][0]))
                out = pr.step(prob, st, var)
                _close('omega_b', eng.get('omega_b', c), out['omega_b'])
                _close('tau', eng.get('tau', c), out['tau'])
                _close('eps', eng.get('eps', c), out['eps'])
                _close('c', eng.get('c', c), out['c'])
                _close('theta', eng.get('theta', c), out['theta'])
                _close('eta', eng.get('eta', c), out['eta'])
                _close('beta', eng.get('beta', c), out['beta'])
                _close('omega_a', eng.get('omega_a', c), out['omega_a'])
                _close('alpha', eng.get('alpha', c), out['alpha'])
                assert np.array_equal(eng.get('z', c), out['z']), ('z', k, c)
                exists_now = P.obs_site.astype(bool) | (out['z'][P.site_id] == 1)   # (from the new z)
                assert np.array_equal(eng.get('exists', c).astype(bool), exists_now)
    finally:
        eng.close()


@pytest.mark.parametrize('chains', [1, 2, 4])
@pytest.mark.parametrize('m', [3, 10, 100])
def test_lock_step_small(m, chains):
    _lockstep(*_data(), m=m, chains=chains, iters=10)


_LATTICES = {}


def _lattice_cached(shape):
    if shape not in _LATTICES:
        _LATTICES[shape] = _lattice(*shape)
    return _LATTICES[shape]


@pytest.mark.parametrize('chains', [1, 2, 4])
@pytest.mark.parametrize('m,shape', [(1280, (40, 40)), (4096, (65, 65))])
def test_lock_step_large(m, shape, chains):
    _lockstep(*_lattice_cached(shape), m=m, chains=chains, iters=10)


# ------------------------------------------------------------------ determinism
def _engine_from(s, keys, start_from=None):
    from occuspytial_amd._engine import Engine
    P = s._problem
    eng = Engine(P, keys, device=0)
    for c in range(len(keys)):
        st = start_from[c]
        eng.set_start(c, st.alpha, st.beta, st.tau, st.eta)
        eng.set('eps', st.eps, c)
        eng.set('z', P.z0, c)
    return eng


def _starts(s, k):
    out = []
    for j in range(k):
        t = s.copy()
        t.__dict__['state'] = type(s.state)(**s.state.__dict__)
        t._initialize_posterior_state(None)
        out.append(t.state)
    return out


def test_runs_are_bit_identical_and_equal_steps_and_solo_chains():
    from occuspytial_amd import ProbitRSRGibbs
    s = ProbitRSRGibbs(*_data(), random_state=4, q=20)
    starts = _starts(s, 3)
    keys = [11, 22, 33]
    e1 = _engine_from(s, keys, starts)
    a1, b1, t1 = e1.run(21, 0)
    e2 = _engine_from(s, keys, starts)
    a2, b2, t2 = e2.run(21, 0)
    assert np.array_equal(a1, a2) and np.array_equal(b1, b2) and np.array_equal(t1, t2)
    e3 = _engine_from(s, keys, starts)   # run == a loop of step
    rows = []
    for _ in range(21):
        e3.step()
        rows.append([np.concatenate([e3.get('alpha', c), e3.get('beta', c), [e3.get('tau', c)]]) for c in range(3)])
    rows = np.array(rows)   # (iter, chain, q + p + 1)
    assert np.array_equal(rows[:, :, :2].transpose(1, 0, 2), a1)
    assert np.array_equal(rows[:, :, 2:5].transpose(1, 0, 2), b1)
    assert np.array_equal(rows[:, :, 5].T, t1)
    for c in (0, 2):   # batched == solo
        e4 = _engine_from(s, [keys[c]], [starts[c]])
        a4, b4, t4 = e4.run(21, 0)
        assert np.array_equal(a4[0], a1[c]) and np.array_equal(b4[0], b1[c]) and np.array_equal(t4[0], t1[c])
        assert np.array_equal(e4.get('eta', 0), e1.get('eta', c))
        e4.close()
    for e in (e1, e2, e3):
        e.close()


# ------------------------------------------------------------------ the sampler contract (reference test_samplers.py)
def test_sampler_contract():
    from occuspytial_amd import ProbitRSRGibbs
    data = _data()
    s = ProbitRSRGibbs(*data, random_state=10)
    out = s.sample(20, chains=1, progressbar=False)
    assert out['alpha'].shape == (1, 20, 2) and out['beta'].shape == (1, 20, 3) and out['tau'].shape == (1, 20)
    out2 = ProbitRSRGibbs(*data, random_state=10).sample(20, chains=1, progressbar=False)
    for k in ('alpha', 'beta', 'tau'):
        assert np.array_equal(out[k], out2[k])
    out = s.sample(20, burnin=5, chains=1, progressbar=False)
    assert out['alpha'].shape == (1, 15, 2)
    with pytest.raises(ValueError, match='burnin value cannot be larger than'):
        s.sample(10, burnin=11)
    out = s.sample(10, chains=3, progressbar=False)
    assert out['alpha'].shape == (3, 10, 2) and out['beta'].shape == (3, 10, 3) and out['tau'].shape == (3, 10)
    c = s.copy()
    assert isinstance(c, ProbitRSRGibbs) and c.rng is not s.rng
    st = dict(alpha=np.zeros(2), beta=np.zeros(3), tau=1.0, eta=np.zeros(s.fixed.q), eps=np.zeros(s.fixed.n))
    out = s.sample(10, chains=1, start=st, progressbar=False)
    assert np.all(np.isfinite(out['beta']))
    s.step()
    assert s.state.eps.shape == (s.fixed.n,) and s.state.eta.shape == (s.fixed.q,) and s.state.spatial.shape == (s.fixed.n,)
    assert np.isfinite(s.state.tau) and np.all(np.isfinite(s.state.omega_b))


def test_checkpoint_resume_is_bit_exact(tmp_path):
    from occuspytial_amd import ProbitRSRGibbs
    data = _data()
    s = ProbitRSRGibbs(*data, random_state=3, q=15)
    full = s.sample(30, chains=2, progressbar=False)
    s2 = ProbitRSRGibbs(*data, random_state=3, q=15)
    s2.sample(12, chains=2, progressbar=False)
    ck = s2.checkpoint(tmp_path / 'ck.npz')
    s3 = ProbitRSRGibbs(*data, random_state=99, q=15)
    tail = s3.resume(str(tmp_path / 'ck.npz'), 18, progressbar=False)
    assert int(ck['n_chains']) == 2
    for k in ('alpha', 'beta', 'tau'):
        assert np.array_equal(tail[k], full[k][:, 12:]), k


# ------------------------------------------------------------------ long run
def test_long_run_from_the_dispersed_start_stays_finite():
    from occuspytial_amd import ProbitRSRGibbs
    s = ProbitRSRGibbs(*_lattice(40, 50, seed=2), random_state=10, q=100)
    out = s.sample(10_000, chains=2, progressbar=False)
    for k in ('alpha', 'beta', 'tau'):
        assert np.all(np.isfinite(out[k])), k
    assert np.all(out['tau'] > 0)
    for name in ('eta', 'spatial', 'eps', 'omega_b', 'omega_a'):
        assert np.all(np.isfinite(getattr(s.state, name))), name


def test_more_chains_than_a_wave():
    """65 chains in one engine: every chain advances, records and equals the same chain run alone."""
    from occuspytial_amd import ProbitRSRGibbs
    s = ProbitRSRGibbs(*_data(), random_state=5, q=8)
    starts = _starts(s, 65)
    keys = [1000 + c for c in range(65)]
    eng = _engine_from(s, keys, starts)
    a, b, t = eng.run(12, 2)
    assert a.shape == (65, 10, 2) and np.all(np.isfinite(a)) and np.all(t > 0)
    assert all(int(eng.get('iter', c)) == 12 for c in range(65))
    for c in (0, 63, 64):
        e1 = _engine_from(s, [keys[c]], [starts[c]])
        a1, b1, t1 = e1.run(12, 2)
        assert np.array_equal(a1[0], a[c]) and np.array_equal(b1[0], b[c]) and np.array_equal(t1[0], t[c]), c
        e1.close()
    eng.close()


# ------------------------------------------------------------------ the posterior: device chains against the restatement on the CPU
def _probit_sim(seed=2):
    """Probit occupancy data at known parameters: 12 x 12 lattice, 100 surveyed sites, 4 visits, p = 3, q = 2."""
    from occuspytial_amd.utils import rand_precision_mat
    rng = np.random.default_rng(seed)
    n = 144
    Q = rand_precision_mat(12, 12).astype(float).tocsr()
    X = np.column_stack([np.ones(n), rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)])
    beta = np.array([0.3, -0.8, 0.6])
    r, c = np.divmod(np.arange(n), 12)
    eta = 0.6 * np.sin(r / 3.0) * np.cos(c / 4.0)
    z = (X @ beta + eta + rng.standard_normal(n) + rng.standard_normal(n) > 0).astype(float)
    alpha = np.array([0.2, 0.9])
    W, y = {}, {}
    for i in np.sort(rng.choice(n, 100, replace=False)):
        Wi = np.column_stack([np.ones(4), rng.uniform(-2, 2, 4)])
        W[int(i)] = Wi
        y[int(i)] = z[i] * (Wi @ alpha + rng.standard_normal(4) > 0)
    return Q, W, X, y


def _cpu_chain(s, start, size, seed):
    """The restatement with numpy's variates: `size` iterations of one chain, alpha and beta of each."""
    prob = restatement_problem(s)
    P = s._problem
    n, m, R = P.n, s.fixed.q, P.R
    st = dict(alpha=start['alpha'], beta=start['beta'], tau=start['tau'], c=prob['Phi'].T @ (prob['K'] @ start['eta']),
              eta=prob['K'] @ start['eta'], eps=start['eps'], z=P.z0.copy())
    rng = np.random.default_rng(seed)
    out = np.empty((size, P.q + P.p))
    for k in range(size):
        var = dict(u_ob=rng.random(n), n_eps=rng.standard_normal(n), gamma=rng.standard_gamma(P.tau_shape),
                   xi=rng.standard_normal(m), n_beta=rng.standard_normal(P.p), u_oa=rng.random(R),
                   n_alpha=rng.standard_normal(P.q), u_z=rng.random(n))
        st = pr.step(prob, st, var)['state']
        out[k] = np.concatenate([st['alpha'], st['beta']])
    return out


def test_posterior_agrees_with_the_restatement_on_the_cpu():
    """4 device chains x 3 000 iterations against 2 CPU chains of the restatement on the same simulated probit data: the
    posterior means of alpha and beta agree within 4 Monte Carlo standard errors, and R-hat of the device chains is
    below 1.05."""
    from occuspytial_amd import ProbitRSRGibbs
    from occuspytial_amd.diagnostics import mcse_mean, rhat
    data = _probit_sim()
    s = ProbitRSRGibbs(*data, random_state=7, q=10)
    start = dict(alpha=np.zeros(2), beta=np.zeros(3), tau=1.0, eta=np.zeros(10), eps=np.zeros(s.fixed.n))
    size, burnin = 3000, 1000
    dev = s.sample(size, burnin=burnin, chains=4, start=start, progressbar=False)
    d = np.concatenate([dev['alpha'], dev['beta']], axis=2)            # (4, 2000, 5)
    cpu = np.stack([_cpu_chain(s, start, size, seed)[burnin:] for seed in (1, 2)])   # (2, 2000, 5)
    for j in range(5):
        assert rhat(d[:, :, j]) < 1.05, (j, rhat(d[:, :, j]))
        se = np.hypot(mcse_mean(d[:, :, j]), mcse_mean(cpu[:, :, j]))
        diff = d[:, :, j].mean() - cpu[:, :, j].mean()
        assert abs(diff) < 4 * se, (j, d[:, :, j].mean(), cpu[:, :, j].mean(), se)

