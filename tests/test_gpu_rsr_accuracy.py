"""Accuracy of the reduced-rank theta update (LogitRSRGibbs: k_rsr_gram / k_rsr_solve up to 128 columns, k_rsr_gram32 and
k_rsrb_* beyond) against a high-precision reference of the same operation (tests/_rsr_reference.py), not against another
float64 code: basis sizes at every block and panel edge up to the cap of 4 096 columns, condition numbers of Lam up to 1e10,
and the regimes the sampler reaches by itself.  Needs an MI355X: ``-m gpu``.

Every comparison feeds the reference the device's own inputs -- beta and z before the step, omega_b and tau after it, eps1
and eps2 drawn by the device's generators on the theta update's streams -- so what is tested is the Gram, K'u, assembly and
solve kernels, not the generators.  With err(x) = ||x - theta_hp|| / ||theta_hp||, the worst over chains and iterations:

  (1) err(theta_dev) <= 10 err(numpy_theta) + 64 u      (as accurate as the reference's own float64 arithmetic)
  (2) err(theta_dev) <= 2 m u kappa(Lam) + F             (no accuracy lost as kappa grows)

F is what forming Lam and r in float64 may cost before any solve (first order, Higham 2002, 3.1 and 7.1): every entry of
Lam is an n-term sum, |dLam| <= g(n + p + 4) |K|'Omega|K| + g(m + 2) tau |Qr|, every entry of r one too,
|dr| <= g(n + p + 4) |K|'(|b| + sqrt(omega) |eps1|) + g(m + 2) sqrt(tau) |E||eps2| (g(k) = k u / (1 - k u)), and
theta moves by Lam^-1 (dr - dLam theta): F = || |dr| + |dLam||theta| || / (lambda_min ||theta||).  Without it (2) would
demand of a one-column basis an r more accurate than n-term float64 sums give.
"""
from types import SimpleNamespace

import numpy as np
import pytest
from scipy import linalg

from . import _rsr_reference as R

pytestmark = pytest.mark.gpu

KEY = 0x9E3779B97F4A7C15
U = R.U
STREAM_TAU, STREAM_ETA_SITE, STREAM_RSR = 2, 3, 9


def _g(k):
    return k * U / (1 - k * U)


def _lattice(rows, cols, seed=5, visits=3):
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q, W, X, y, *_ = make_lattice_problem(rows, cols, visits=visits, p=2, q=2, random_state=seed)
    return FlatProblem(Q, W, X, y)


def _set_basis(prob, K, Qr, E):
    m = K.shape[1]
    prob.rsr = {'K': np.ascontiguousarray(K), 'Q': np.ascontiguousarray(Qr), 'E': np.ascontiguousarray(E), 'dim': m}
    prob.tau_shape = 0.5 + 0.5 * m      # as enable_rsr sets it


def _engine(prob, starts):
    from occuspytial_amd._engine import Engine
    keys = [KEY + 7 * c for c in range(len(starts))]
    eng = Engine(prob, keys)
    for c, st in enumerate(starts):
        eng.set_start(c, **st)
    return eng


def _starts(prob, C, seed, eta_scale=0.3, theta=None):
    rng = np.random.default_rng(seed)
    m = prob.rsr['dim']
    return [dict(alpha=rng.standard_normal(prob.q), beta=rng.standard_normal(prob.p), tau=1.0 + c,
                 eta=eta_scale * rng.standard_normal(m) if theta is None else theta[c]) for c in range(C)]


def _step(eng, prob, gram=False, reseat=None):
    """One eng.step(); per chain the inputs of its theta update and what the device made of them."""
    from occuspytial_amd._engine import device_draw
    if reseat is not None:
        for c in range(eng.n_chains):
            for name, v in reseat.items():
                eng.set(name, v, c)
    m = prob.rsr['dim']
    out = []
    for c in range(eng.n_chains):
        out.append(dict(beta=eng.get('beta', c), z=eng.get('z', c), it=int(np.atleast_1d(eng.get('iter', c))[0]),
                        theta_prev=eng.get('theta', c), key=eng.keys[c]))
    eng.step()
    for c, d in enumerate(out):
        d.update(omega=eng.get('omega_b', c), tau=float(np.atleast_1d(eng.get('tau', c))[0]), theta=eng.get('theta', c),
                 eta=eng.get('eta', c))
        d['eps1'] = device_draw('normal', n=prob.n, key=d['key'], it=d['it'], stream=STREAM_ETA_SITE)
        d['eps2'] = device_draw('normal', n=m, key=d['key'], it=d['it'], stream=STREAM_RSR)
        if gram:
            d['gram'] = eng.get('rsr_gram', c).reshape(m, m)
    return out


def _forming_bound(prob, d, theta, lam_min):
    """F of the module docstring."""
    K, Qr, E = prob.rsr['K'], prob.rsr['Q'], prob.rsr['E']
    n, m = K.shape
    om, tau = d['omega'], d['tau']
    b = np.abs(np.asarray(R.b_hp(d['z'], om, prob.X, d['beta']), dtype=np.float64))
    aK, at = np.abs(K), np.abs(theta)
    gn, gm = _g(n + prob.p + 4), _g(m + 2)
    v = gn * (aK.T @ (om * (aK @ at)) + aK.T @ (b + np.sqrt(om) * np.abs(d['eps1'])))
    v += gm * (tau * (np.abs(Qr) @ at) + np.sqrt(tau) * (np.abs(E) @ np.abs(d['eps2'])))
    return float(np.linalg.norm(v) / (lam_min * np.linalg.norm(theta)))


def _reference(prob, d):
    """theta_hp, Lam_hp, r_hp of one chain's update; numpy_theta on the same inputs."""
    K, Qr, E = prob.rsr['K'], prob.rsr['Q'], prob.rsr['E']
    Lam = R.lam_hp(K, Qr, d['omega'], d['tau'])
    bl = R.b_hp(d['z'], d['omega'], prob.X, d['beta'])
    r = R.rhs_hp(K, bl, d['omega'], d['eps1'], E, d['eps2'], d['tau'])
    th = R.theta_hp(Lam, r)
    th_np = R.numpy_theta(K, Qr, E, bl.astype(np.float64), d['omega'], d['tau'], d['eps1'], d['eps2'])
    return th, th_np, Lam


def _check_theta(prob, d, label):
    """Criteria (1) and (2) for one chain's update; returns (err_dev, err_np, kappa, theta_hp)."""
    m = prob.rsr['dim']
    th, th_np, Lam = _reference(prob, d)
    w = linalg.eigvalsh(Lam.astype(np.float64), check_finite=False)
    kap = float(w[-1] / w[0])
    err_dev, err_np = R.rel_err(d['theta'], th), R.rel_err(th_np, th)
    F = _forming_bound(prob, d, th.astype(np.float64), w[0])
    print(f'  {label:<34s} m={m:<5d} kappa={kap:9.2e} err_dev={err_dev:9.2e} err_np={err_np:9.2e} '
          f'bound2={2 * m * U * kap:9.2e}+{F:8.2e}')
    assert err_dev <= 10 * err_np + 64 * U, (label, err_dev, err_np)
    assert err_dev <= 2 * m * U * kap + F, (label, err_dev, kap, F)
    return err_dev, err_np, kap, th, Lam


def _check_eta(prob, d):
    """eta = K theta_dev entry by entry within 4 m u (|K||theta|)."""
    K = prob.rsr['K']
    m = K.shape[1]
    ref = R._ld_matvec(K, d['theta'])
    diff = np.abs((np.asarray(d['eta'], dtype=R.LD) - ref).astype(np.float64))
    assert np.all(diff <= 4 * m * U * (np.abs(K) @ np.abs(d['theta'])) + 1e-300), diff.max()


def _check_tau(prob, d):
    """tau = g / (theta_prev'Qr theta_prev / 2 + b) with g the device's own gamma variate: the quadratic form is
    (2m + 1)-term sums, |d quad| <= g(2m + 1) |theta|'|Qr||theta|, and rate, 1 / rate and the product round once each."""
    from occuspytial_amd._engine import device_draw
    Qr = prob.rsr['Q']
    m = Qr.shape[0]
    g = device_draw('std_gamma', param=[prob.tau_shape], key=d['key'], it=d['it'], stream=STREAM_TAU)[0]
    tp = d['theta_prev']
    quad = np.dot(np.asarray(tp, dtype=R.LD), R._ld_matvec(Qr, tp))
    rate = quad / 2 + R.LD(prob.tau_rate)
    tau_hp = R.LD(g) / rate
    A = np.abs(tp) @ (np.abs(Qr) @ np.abs(tp))
    bound = (_g(2 * m + 1) * A / 2 + 4 * U * float(rate)) / float(rate)
    rel = abs(float((R.LD(d['tau']) - tau_hp) / tau_hp))
    assert rel <= bound, (rel, bound, d['tau'])


def _report(rows):
    kap = max(r[2] for r in rows)
    return max(r[0] for r in rows), max(r[1] for r in rows), kap


def test_reference_is_fed_the_devices_own_inputs():
    """The wiring first, at kappa ~ 10 (16 Moran columns, tau 1.5): with beta and z read before the step, omega_b and tau
    after it, and eps1 / eps2 drawn by device_draw on the theta update's streams (3 and STREAM_RSR) at the iteration
    counter before the step, the device's theta IS theta_hp to ~1e-14 -- a wrong stream, counter or state read would be
    O(1)."""
    prob = _lattice(20, 25)
    prob.enable_rsr(q=16)
    eng = _engine(prob, _starts(prob, 1, 16))
    print()
    try:
        for it in range(2):
            d = _step(eng, prob)[0]
            err_dev, err_np, kap, _, _ = _check_theta(prob, d, f'wiring it={it}')
            assert kap < 1e3 and err_dev < 1e-13, (kap, err_dev)
    finally:
        eng.close()


# ---- a. sizes: the small path's block edges, the large path's panel edges, the old and the new cap ---------------------
@pytest.mark.parametrize('m, C', [(1, 1), (3, 2), (16, 3), (17, 1), (127, 2), (128, 3), (129, 3)])
def test_theta_accuracy_at_block_and_panel_edges(m, C):
    """A 20 x 25 lattice's Moran basis of m columns, C chains (m = 129: k_rsr_gram32's full pair and its half-empty one),
    two iterations; every chain's theta against theta_hp, eta against K theta, tau against its conditional from the
    previous theta.  Up to 128 columns also the Gram matrix the update used (rsr_gram, upper triangle) against gram_hp
    entry by entry within g(n + 1) |K|'Omega|K| (n-term sums of products of two roundings)."""
    prob = _lattice(20, 25)
    prob.enable_rsr(q=m)
    eng = _engine(prob, _starts(prob, C, m))
    rows = []
    print()
    try:
        for it in range(2):
            for c, d in enumerate(_step(eng, prob, gram=m <= 128)):
                rows.append(_check_theta(prob, d, f'sizes it={it} chain={c}')[:3])
                _check_eta(prob, d)
                _check_tau(prob, d)
                if m <= 128:
                    K = prob.rsr['K']
                    G = R.gram_hp(K, d['omega'])
                    A = np.abs(K).T @ (d['omega'][:, None] * np.abs(K))
                    iu = np.triu_indices(m)
                    diff = np.abs((np.asarray(d['gram'][iu], dtype=R.LD) - G[iu]).astype(np.float64))
                    assert np.all(diff <= _g(prob.n + 1) * A[iu]), (c, float((diff / A[iu]).max()))
    finally:
        eng.close()
    print('  worst err_dev={:.2e} err_np={:.2e} kappa={:.2e}'.format(*_report(rows)))


@pytest.fixture(scope='module')
def cap_basis():
    """A 65 x 64 lattice (4 160 sites) with a random orthonormal basis of 4 096 columns (np.linalg.qr: cheaper than the
    Moran eigenproblem); every size below the cap takes its first m columns."""
    prob = _lattice(65, 64, seed=9, visits=2)
    K = np.linalg.qr(np.random.default_rng(4096).standard_normal((prob.n, 4096)))[0]
    return prob, K


@pytest.mark.parametrize('m', [2048, 2049, 4095, 4096])
def test_theta_accuracy_up_to_the_basis_cap(cap_basis, m):
    """m = 2 048 / 2 049 (the old cap, a ragged last panel of one row) and 4 095 / 4 096 (the cap): three chains for one
    iteration.  Chains 0 and 2 -- the first member of k_rsr_gram32's full pair and its half-empty one -- against theta_hp;
    chain 1 against float64 numpy on the same inputs, within the sum of the two's bounds (2) (both lie within it of the
    true theta); every chain's eta and tau as above.  Qr = K'QK and E from eigh(Qr), as enable_rsr forms them."""
    prob, Kfull = cap_basis
    K = np.ascontiguousarray(Kfull[:, :m])
    Qr = K.T @ (prob.Q @ K)
    Qr = 0.5 * (Qr + Qr.T)
    s, u = np.linalg.eigh(Qr)
    _set_basis(prob, K, Qr, u * np.sqrt(np.clip(s, 0.0, None)))
    eng = _engine(prob, _starts(prob, 3, m, eta_scale=0.1))
    rows = []
    print()
    try:
        for c, d in enumerate(_step(eng, prob)):
            _check_eta(prob, d)
            _check_tau(prob, d)
            if c != 1:
                rows.append(_check_theta(prob, d, f'cap chain={c}')[:3])
                continue
            lam = K.T @ (d['omega'][:, None] * K) + d['tau'] * Qr
            bl = R.b_hp(d['z'], d['omega'], prob.X, d['beta']).astype(np.float64)
            th_np = R.numpy_theta(K, Qr, prob.rsr['E'], bl, d['omega'], d['tau'], d['eps1'], d['eps2'])
            w = linalg.eigvalsh(lam, check_finite=False)
            kap = float(w[-1] / w[0])
            bound = 2 * (2 * m * U * kap + _forming_bound(prob, d, th_np, w[0]))
            diff = R.rel_err(d['theta'], th_np)
            print(f'  cap chain=1 (against numpy)          m={m:<5d} kappa={kap:9.2e} diff={diff:9.2e} bound={bound:9.2e}')
            assert diff <= bound, (diff, bound)
    finally:
        eng.close()
    print('  worst err_dev={:.2e} err_np={:.2e} kappa={:.2e}'.format(*_report(rows)))


# ---- b. conditioning sweep: the same model in a worse basis -------------------------------------------------------------
@pytest.mark.parametrize('kap', [1e2, 1e5, 1e8, 1e10])
@pytest.mark.parametrize('m, lattice', [(100, (20, 25)), (1280, (40, 40))])
def test_theta_accuracy_as_kappa_grows(m, lattice, kap):
    """The Moran basis of m columns (100: the small path; 1 280: the large one, the reference's default size at 100 x 100,
    here on a 40 x 40 lattice) rewritten in the basis K M (tests/_rsr_reference.reparam) so that kappa(Lam) ~ kap; the
    starting theta is mapped by M^-1, so eta and tau's rate start where they would.  Two chains, two iterations, criteria
    (1) and (2); and eta against K theta_hp of the ORIGINAL basis on the same inputs within 2 m u kappa ||eta||: a backward
    stable solve in the basis K M moves eta by Lam^-1 M^-T dLam' M^-1 theta, ||dLam'|| ~ m u ||Lam||, i.e. by ~ m u kappa(Lam')."""
    prob = _lattice(*lattice)
    prob.enable_rsr(q=m)
    K0, Q0, E0 = prob.rsr['K'], prob.rsr['Q'], prob.rsr['E']
    rng = np.random.default_rng(int(np.log10(kap)) + m)
    _, M = R.spread_for(K0, Q0, np.full(prob.n, 0.2), 1.5, kap, rng)
    _set_basis(prob, *R.reparam(K0, Q0, E0, M))
    th0 = [0.3 * rng.standard_normal(m) for _ in range(2)]
    eng = _engine(prob, _starts(prob, 2, m, theta=[np.linalg.solve(M, t) for t in th0]))
    orig = SimpleNamespace(rsr={'K': K0, 'Q': Q0, 'E': E0, 'dim': m}, X=prob.X, p=prob.p)     # same eps2: r' = M'r
    rows = []
    print()
    try:
        for it in range(2):
            for c, d in enumerate(_step(eng, prob)):
                err_dev, err_np, k, _, _ = _check_theta(prob, d, f'kappa~{kap:.0e} it={it} chain={c}')
                rows.append((err_dev, err_np, k))
                _check_eta(prob, d)
                th_o = _reference(orig, d)[0]
                eta_hp = R._ld_matvec(K0, th_o)
                rel = R.rel_err(d['eta'], eta_hp)
                assert rel <= 2 * m * U * k, (rel, 2 * m * U * k)
    finally:
        eng.close()
    e, n_, k = _report(rows)
    print(f'  worst err_dev={e:.2e} err_np={n_:.2e} kappa={k:.2e}')
    assert 0.01 * kap < k < 100 * kap


# ---- c. regimes the sampler reaches by itself ----------------------------------------------------------------------------
@pytest.mark.parametrize('regime', ['large_tau', 'small_tau', 'large_predictors'])
def test_theta_accuracy_in_extreme_regimes(regime):
    """The Moran basis at m = 160 (large path).  large_tau: a tiny starting theta and tau_rate = 1e-8, so that tau ~ 1e9 and
    Lam ~ tau Qr; small_tau: a starting theta of scale 1e3, so that theta'Qr theta is large, tau tiny, Lam ~ K'Omega K,
    and |x'beta + eta| in the thousands makes omega tiny; large_predictors: beta and alpha re-seated before every iteration
    so that |x'beta| reaches a few hundred (test_gpu_parity._large_predictors).  Two chains, two iterations, criteria (1)
    and (2), eta and tau."""
    from .test_gpu_parity import _large_predictors
    prob = _lattice(20, 25)
    prob.enable_rsr(q=160)
    reseat = None
    scale = {'large_tau': 1e-6, 'small_tau': 1e3, 'large_predictors': 0.3}[regime]
    if regime == 'large_tau':
        prob.tau_rate = 1e-8
    if regime == 'large_predictors':
        reseat = _large_predictors(prob, 5)
    eng = _engine(prob, _starts(prob, 2, 160, eta_scale=scale))
    rows, taus, omegas = [], [], []
    print()
    try:
        for it in range(2):
            for c, d in enumerate(_step(eng, prob, reseat=reseat(it) if reseat else None)):
                rows.append(_check_theta(prob, d, f'{regime} it={it} chain={c}')[:3])
                _check_eta(prob, d)
                _check_tau(prob, d)
                taus.append(d['tau'])
                omegas.append(d['omega'].min())
    finally:
        eng.close()
    print('  worst err_dev={:.2e} err_np={:.2e} kappa={:.2e}'.format(*_report(rows)), f'tau {min(taus):.1e}..{max(taus):.1e}',
          f'min omega {min(omegas):.1e}')
    if regime == 'large_tau':
        assert min(taus[:2]) > 1e6
    if regime == 'small_tau':
        assert max(taus[:2]) < 1e-3 and min(omegas[:2]) < 1e-3


# ---- d. what rsr_gram holds on the large path: the factor U outside the diagonal blocks ---------------------------------
@pytest.mark.parametrize('m', [160, 333])
def test_large_path_factor_rows_against_long_double_cholesky(m):
    """Beyond 128 columns rsr_gram holds, after an update, the upper Cholesky factor U of Lam in the rows of each 32-row
    panel right of its diagonal block -- what k_rsrb_step's panel triangular solves (rsrb_apply, X = U_kk^-T P on the matrix
    cores) wrote.  Those entries against the long-double factor of Lam_hp, within 10 x the error of scipy's float64
    cholesky of the same Lam: a wrong panel solve shows here, where it is made.  Two chains, one iteration."""
    prob = _lattice(20, 25)
    prob.enable_rsr(q=m)
    eng = _engine(prob, _starts(prob, 2, m))
    print()
    try:
        steps = _step(eng, prob, gram=True)
    finally:
        eng.close()
    P = 32
    mask = np.zeros((m, m), dtype=bool)
    for k0 in range(0, m, P):
        mask[k0:k0 + P, k0 + P:] = True
    for c, d in enumerate(steps):
        _, _, kap, _, Lam = _check_theta(prob, d, f'factor chain={c}')
        Uhp = R.cholesky_hp(Lam)
        Usp = linalg.cholesky(Lam.astype(np.float64), lower=False)
        ref = Uhp[mask]
        nrm = np.linalg.norm(ref.astype(np.float64))
        e_dev = np.linalg.norm((np.asarray(d['gram'][mask], dtype=R.LD) - ref).astype(np.float64)) / nrm
        e_sp = np.linalg.norm((np.asarray(Usp[mask], dtype=R.LD) - ref).astype(np.float64)) / nrm
        print(f'  factor chain={c} m={m} kappa={kap:.2e} err_U_dev={e_dev:.2e} err_U_scipy={e_sp:.2e}')
        assert e_dev <= 10 * e_sp, (c, e_dev, e_sp)
