"""The logit z update over the whole range of its occupancy predictor a0 = x_i beta + eta_i, psi = expit(a0) rounding to 1
included, against the log-space reference of tests/_z_theory.py (which tests/test_z_theory_cpu.py holds to mpmath).  The
tolerances are those of _z_theory's docstring -- derived there, none measured, and none grows with 1 / (1 - psi):

    pr: 1e-12 b min(pr, q) + 4 u      l: 1e-12 (b + |l|)      D: the tolerance of l, times D      (u = 2^-53)

Two kinds of test.  Injected uniforms (occ_cond_z; k_cond_beta_z, z_update_site and z_update_site_g): every point of the
reference's grid sits at a site of one lattice, and the uniforms pr -+ tol must give z = 1 and z = 0.  The accumulating
variants (k_z_ob_stats, k_z_ob_ll, k_z_ob_ppc, k_holdout_sites and the generic kernels): a workload whose pinned coefficients
carry it into the regime by itself, the sums of eight iterations against the reference evaluated at the states read back, and
-- a condition on the inputs -- enough sites in every iteration at which the form that subtracts psi from 1 misses the
tolerances.  Every test prints its worst found / bound before it asserts."""
import numpy as np
import pytest

from . import _z_theory as zt
from ._outputs_gpu import engine_with, time_limit as _time_limit  # noqa: F401 (autouse in this module)
from .test_gpu_holdout import CNT, LIK, LOG, LOG2, PD, holdout_terms
from .test_gpu_parity import KEY
from .test_gpu_waic import _ll_terms

pytestmark = pytest.mark.gpu
U = zt.U


# ------------------------------------------------------------------ 1: injected uniforms at every point of the grid
def grid_problem(p):
    """The 24 x 30 lattice, one grid point per site in site order: 672 surveyed sites without a detection, then 24 sites that
    were not surveyed (the a0 of the grid and three more of it) and 24 with a detection.  X = [1, a0, ...], W = [1, -t_r, ...];
    with beta = alpha = (0, 1, 0, ...) and eta = 0, a0 and t_r reach the update exactly (products with 0 add +-0).
    -> (prob, a0 of every site, the reference of the 672 points as arrays)."""
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q = make_lattice_problem(24, 30, visits=1, p=2, q=2, random_state=1)[0]
    pts = zt.grid()
    n, G = 720, len(pts)
    rng = np.random.default_rng(5)
    a0 = np.concatenate([[pt[0] for pt in pts], (zt.A0_GRID + zt.A0_GRID[9:12]), rng.uniform(-40.0, 40.0, 24)])
    assert a0.size == n and G == 672
    X = rng.standard_normal((n, p))
    X[:, 0], X[:, 1] = 1.0, a0
    W, y = {}, {}
    for i in list(range(G)) + list(range(G + 24, n)):
        t = pts[i][1] if i < G else -rng.uniform(-3.0, 6.0, 1 + i % 5)
        w = rng.standard_normal((t.size, p))
        w[:, 0], w[:, 1] = 1.0, -t
        W[i], y[i] = w, np.zeros(t.size)
        if i >= G:
            y[i][i % t.size] = 1.0
    prob = FlatProblem(Q, W, X, y)
    assert prob.not_surveyed == list(range(G, G + 24)) and prob.obs == list(range(G + 24, n))
    refs = [zt.site(a, t) for a, t in pts]
    return prob, a0, {k: np.array([float(r[k]) for r in refs]) for k in ('pr', 'q', 'l', 'D', 'b')}


@pytest.mark.parametrize('p', [2, 9])
def test_injected_uniforms_decide_as_the_reference_over_the_whole_range(p):
    """p = q = 2: z_update_site; p = q = 9, the further coefficients 0: z_update_site_g.  Two passes: a0 through x_i beta
    (beta = (0, 1), eta = 0) and through eta (beta = 0, eta_i = a0).  u = pr - tol must give z = 1 and u = pr + tol must give
    z = 0 at every surveyed site without a detection -- one side only where the other would leave (0, 1); an unsurveyed site is
    held to expit(a0) in the same way (b = 1 + |a0|); a site with a detection stays 1 whatever u."""
    prob, a0, ref = grid_problem(p)
    G, n = 672, prob.n
    uns = np.arange(G, G + 24)
    pr = np.concatenate([ref['pr'], np.exp(zt.lsig(a0[uns]))])
    q = np.concatenate([ref['q'], np.exp(zt.lsig(-a0[uns]))])
    tol = 1e-12 * np.concatenate([ref['b'], 1.0 + np.abs(a0[uns])]) * np.minimum(pr, q) + 4.0 * U
    lo, hi = pr - tol, pr + tol
    lo_ok, hi_ok = lo > 0.0, hi < 1.0
    print('grid of %d points and %d unsurveyed sites: u = pr - tol tested at %d, u = pr + tol at %d' % (G, uns.size, lo_ok.sum(), hi_ok.sum()))
    assert lo_ok.sum() >= 450 and hi_ok.sum() >= 450 and np.all(lo_ok | hi_ok)
    coef = np.zeros(p)
    coef[1] = 1.0
    eng = engine_with(prob, [KEY], [dict(alpha=coef, beta=coef, tau=1.0, eta=np.zeros(n))])
    for through_eta in (False, True):
        if through_eta:
            eng.set('beta', np.zeros(p))
            eng.set('eta', a0)
        u_lo = np.concatenate([np.where(lo_ok, lo, 0.5), np.full(24, 0.999)])
        u_hi = np.concatenate([np.where(hi_ok, hi, 0.5), np.full(24, 0.999)])
        z_lo, z_hi = eng.cond_z(u_lo), eng.cond_z(u_hi)
        bad_lo = np.flatnonzero(lo_ok & (z_lo[:G + 24] != 1.0))
        bad_hi = np.flatnonzero(hi_ok & (z_hi[:G + 24] != 0.0))
        print('a0 through %s: %d sites decide 0 at pr - tol, %d decide 1 at pr + tol' % ('eta' if through_eta else 'x beta', bad_lo.size, bad_hi.size))
        for a, b in ((-701.0, 0.0), (0.0, 10.0), (10.0, 20.0), (20.0, 30.0), (30.0, 36.5), (36.5, 701.0)):
            band = (a0[:G + 24] >= a) & (a0[:G + 24] < b)
            print('    a0 in [%g, %g): decisions tested %d, as the reference %d' % (a, b, (lo_ok & band).sum() + (hi_ok & band).sum(),
                  (lo_ok & band & (z_lo[:G + 24] == 1.0)).sum() + (hi_ok & band & (z_hi[:G + 24] == 0.0)).sum()))
        assert bad_lo.size == 0, [(i, a0[i], pr[i]) for i in bad_lo[:8]]
        assert bad_hi.size == 0, [(i, a0[i], pr[i]) for i in bad_hi[:8]]
        assert np.all(z_lo[G + 24:] == 1.0) and np.all(z_hi[G + 24:] == 1.0)
    eng.close()


# ------------------------------------------------------------------ 2: the accumulating variants, in the regime by themselves
def probe_problem(p):
    """The 13 x 17 queen lattice.  Every second site is a probe: x_2 = linspace(-5, 60) over the probes, 1 to 40 visits, no
    detection; the others have 1 to 6 visits and y ~ Bernoulli(0.4).  Every seventh site is not surveyed; of those the probes and
    every second other one are held out, with withheld visits of the site's kind.  The priors pin beta to (0, 1, 0, ...) and alpha
    to (1, 1, 0, ...), so a0 = x_2 + eta_i reaches 60 and the visits' detection probability is expit(1 + w_2).
    -> (prob, keys, starts, Wt, yt)."""
    from occuspytial_amd._problem import FlatProblem
    from occuspytial_amd.utils import make_lattice_problem
    Q = make_lattice_problem(13, 17, visits=1, p=2, q=2, random_state=6)[0]
    n = 13 * 17
    rng = np.random.default_rng(31)
    probes = np.arange(0, n, 2)
    X = 0.5 * rng.standard_normal((n, p))
    X[:, 0] = 1.0
    X[:, 1] = rng.uniform(-2.0, 2.0, n)
    X[probes, 1] = np.linspace(-5.0, 60.0, probes.size)
    W, y, Wt, yt = {}, {}, {}, {}
    for i in range(n):
        probe = i % 2 == 0
        v = 1 + (7 * (i // 2)) % 40 if probe else int(rng.integers(1, 7))
        w = 0.5 * rng.standard_normal((v, p))
        w[:, 0] = 1.0
        w[:, 1] = rng.uniform(-2.0, 2.0, v)
        yy = np.zeros(v) if probe else rng.binomial(1, 0.4, v).astype(float)
        if i % 7 == 0:
            if probe or i % 4 == 1:
                Wt[i], yt[i] = w, yy
        else:
            W[i], y[i] = w, yy
    b_mu, a_mu = np.zeros(p), np.zeros(p)
    b_mu[1], a_mu[0], a_mu[1] = 1.0, 1.0, 1.0
    hp = dict(b_mu=b_mu, a_mu=a_mu, b_prec=1e10 * np.eye(p), a_prec=1e10 * np.eye(p))
    prob = FlatProblem(Q, W, X, y, hp)
    eta = 0.5 * rng.standard_normal(n)
    return prob, [KEY + 5], [dict(alpha=a_mu.copy(), beta=b_mu.copy(), tau=1.0, eta=eta - eta.mean())], Wt, yt


def _sum_bound(tols, terms, N):
    """The bound of a sum of N terms: the sum of the terms' tolerances plus 2 N u sum |terms|."""
    return tols + 2.0 * N * U * terms


def _accumulate(p, ppc):
    """Eight iterations (occ_step; with ``ppc`` run(1, 0), whose one kept draw replicates the detections) with the site sums, the
    log-likelihood sums and the held-out sums on; after each, alpha, beta and eta are read back, the reference evaluated and
    its terms and their tolerances accumulated.  Then site_occ, the three log-likelihood sums and the held-out sums are
    compared, each sum's bound being the sum of its terms' tolerances plus 2 N u sum |terms|:
      pr at a surveyed site without a detection, and expit(a0) at an unsurveyed one (b = 1 + sum |products_0|): tol_pr; a site
        with a detection adds exactly 1;
      l, no detection: 1e-12 (b + |l|); a detection: 1e-12 sum_terms (sum |products| + |term| + 1), the bound
        tests/test_gpu_waic.py derives;   L: the tolerance of l times L, and one ulp of exp;   l^2: 2 |l| times the tolerance of l;
      held out: the same over the withheld rows; pd keeps the absolute bound 1e-12 sum ((sum |products_0| + 1) + sum_r (sum |products_r| + 1))
        of tests/test_gpu_holdout.py.
    Power: in every iteration the form num / ((1 - psi) + num), evaluated in float64 at the states read back, misses the
    tolerance of pr at 15 surveyed sites without a detection or more, that of l at 15 or more, and that of l at 5 held-out
    entries or more; otherwise the test fails for lack of power."""
    from occuspytial_amd.holdout import holdout_arg, unpack
    prob, keys, starts, Wt, yt = probe_problem(p)
    data = unpack(holdout_arg((Wt, yt), prob), prob.q)
    h_seen = np.add.reduceat(data[2], data[1][:-1]) > 0
    n, H, N = prob.n, data[0].size, 8
    und = np.asarray(prob.obs_site) == 0
    und_sites = prob.site_id[und]
    uns = np.asarray(prob.not_surveyed)
    assert und.sum() >= 100 and (~und).sum() >= 50 and uns.size >= 30 and (~h_seen).sum() >= 14 and h_seen.sum() >= 3
    eng = engine_with(prob, keys, starts, site=True, ll=True, ppc=ppc, holdout=(Wt, yt))
    acc = {k: np.zeros(n) for k in ('occ', 'occ_tol', 'lik', 'lik_tol', 'log', 'log_abs', 'log_tol', 'log2', 'log2_tol')}
    hac = {k: np.zeros(H) for k in ('lik', 'lik_tol', 'log', 'log_abs', 'log_tol', 'log2', 'log2_tol', 'pd', 'pd_tol')}
    power = []
    for _ in range(N):
        if ppc:
            eng.run(1, 0)
        else:
            eng.step()
        alpha, beta, eta = (eng.get(name) for name in ('alpha', 'beta', 'eta'))
        ref = zt.problem_terms(prob.X, eta, beta, prob.W, alpha, prob.site_ptr, prob.site_id)
        a0 = prob.X @ beta + eta
        pr, pr_tol = np.ones(n), np.zeros(n)
        pr[und_sites], pr_tol[und_sites] = ref['pr'][und], zt.tol_pr(ref)[und]
        pr[uns] = np.exp(zt.lsig(a0[uns]))
        b_uns = 1.0 + np.abs(prob.X[uns] * beta).sum(axis=1) + np.abs(eta[uns])
        pr_tol[uns] = 1e-12 * b_uns * np.minimum(pr[uns], np.exp(zt.lsig(-a0[uns]))) + 4.0 * U
        acc['occ'] += pr
        acc['occ_tol'] += pr_tol
        ll, lik, b = _ll_terms(prob, alpha, beta, eta)
        _add(acc, ll, lik, 1e-12 * b)
        hl, hlik, hpd, hb, hbp = holdout_terms(prob.X, data, alpha, beta, eta)
        _add(hac, hl, hlik, 1e-12 * hb)
        hac['pd'] += hpd
        hac['pd_tol'] += 1e-12 * hbp
        # power: the subtracting form at these states
        s_pr, s_D = zt.subtracting_terms(prob.X, eta, beta, prob.W, alpha, prob.site_ptr, prob.site_id)
        with np.errstate(divide='ignore'):
            m_pr = ~(np.abs(s_pr - ref['pr']) <= zt.tol_pr(ref)) & und
            m_l = ~(np.abs(np.log(s_D) - ref['l']) <= zt.tol_l(ref)) & und
            href = zt.problem_terms(prob.X, eta, beta, data[3], alpha, data[1], data[0])
            h_D = zt.subtracting_terms(prob.X, eta, beta, data[3], alpha, data[1], data[0])[1]
            m_h = ~(np.abs(np.log(h_D) - href['l']) <= zt.tol_l(href)) & ~h_seen
        power.append((int(m_pr.sum()), int(m_l.sum()), int(m_h.sum())))
        assert np.max(np.abs(beta - starts[0]['beta'])) < 1e-3 and np.max(np.abs(alpha - starts[0]['alpha'])) < 1e-3   # the priors pin them
    print('p = %d, ppc %s: sites per iteration where the subtracting form misses (pr, l, held-out l): %s; a0 up to %.1f'
          % (p, ppc, power, np.max(a0)))
    site = eng.site_sums()
    lls = eng.loglik_sums()
    hold = eng.holdout_sums()
    eng.close()
    sv = np.zeros(n, dtype=bool)
    sv[prob.site_id] = True
    fig = dict(
        occ=np.max(np.abs(site['occ'] - acc['occ']) / _sum_bound(acc['occ_tol'], acc['occ'], N)),
        lik=np.max(np.abs(lls['lik'] - acc['lik'])[sv] / _sum_bound(acc['lik_tol'], acc['lik'], N)[sv]),
        log=np.max(np.abs(lls['log'] - acc['log'])[sv] / _sum_bound(acc['log_tol'], acc['log_abs'], N)[sv]),
        log2=np.max(np.abs(lls['log2'] - acc['log2'])[sv] / _sum_bound(acc['log2_tol'], acc['log2'], N)[sv]))
    g = hold['sums']
    hfig = dict(
        lik=np.max(np.abs(g[LIK] - hac['lik']) / _sum_bound(hac['lik_tol'], hac['lik'], N)),
        log=np.max(np.abs(g[LOG] - hac['log']) / _sum_bound(hac['log_tol'], hac['log_abs'], N)),
        log2=np.max(np.abs(g[LOG2] - hac['log2']) / _sum_bound(hac['log2_tol'], hac['log2'], N)),
        pd=np.max(np.abs(g[PD] - hac['pd']) / _sum_bound(hac['pd_tol'], hac['pd'], N)))
    print('p = %d, ppc %s: worst found / bound: site and log-likelihood sums %s; held-out sums %s' % (p, ppc, fig, hfig))
    assert site['count'] == N and lls['count'] == N and hold['count'] == N and np.all(g[CNT] == N)
    assert all(a >= 15 and b >= 15 and c >= 5 for a, b, c in power), power
    assert not lls['log'][~sv].any() and not lls['lik'][~sv].any()
    assert all(v <= 1.0 for v in fig.values()), fig
    assert all(v <= 1.0 for v in hfig.values()), hfig


def _add(a, ll, lik, tol_l):
    """One iteration's l, L and l^2 with their tolerances into the running sums."""
    a['lik'] += lik
    a['lik_tol'] += (tol_l + 4.0 * U) * lik
    a['log'] += ll
    a['log_abs'] += np.abs(ll)
    a['log_tol'] += tol_l
    a['log2'] += ll * ll
    a['log2_tol'] += 2.0 * np.abs(ll) * tol_l


def test_site_and_loglik_and_heldout_sums_in_the_regime():
    """k_z_ob_stats's site_occ rides k_z_ob_ll here (both switches on); k_holdout_sites behind it."""
    _accumulate(2, ppc=False)


def test_site_sums_alone_in_the_regime():
    """k_z_ob_stats itself (the log-likelihood sums off): site_occ of eight iterations."""
    prob, keys, starts, _, _ = probe_problem(2)
    und = np.asarray(prob.obs_site) == 0
    n, N = prob.n, 8
    eng = engine_with(prob, keys, starts, site=True)
    occ, tol, power = np.zeros(n), np.zeros(n), []
    uns = np.asarray(prob.not_surveyed)
    for _ in range(N):
        eng.step()
        alpha, beta, eta = (eng.get(name) for name in ('alpha', 'beta', 'eta'))
        ref = zt.problem_terms(prob.X, eta, beta, prob.W, alpha, prob.site_ptr, prob.site_id)
        a0 = prob.X @ beta + eta
        pr, pr_tol = np.ones(n), np.zeros(n)
        pr[prob.site_id[und]], pr_tol[prob.site_id[und]] = ref['pr'][und], zt.tol_pr(ref)[und]
        pr[uns] = np.exp(zt.lsig(a0[uns]))
        pr_tol[uns] = 1e-12 * (1.0 + np.abs(prob.X[uns] * beta).sum(axis=1) + np.abs(eta[uns])) * np.minimum(pr[uns], np.exp(zt.lsig(-a0[uns]))) + 4.0 * U
        occ += pr
        tol += pr_tol
        s_pr = zt.subtracting_terms(prob.X, eta, beta, prob.W, alpha, prob.site_ptr, prob.site_id)[0]
        power.append(int((~(np.abs(s_pr - ref['pr']) <= zt.tol_pr(ref)) & und).sum()))
    site = eng.site_sums()
    eng.close()
    worst = np.max(np.abs(site['occ'] - occ) / _sum_bound(tol, occ, N))
    print('site_occ alone: worst found / bound %.3g; sites per iteration where the subtracting form misses pr: %s' % (worst, power))
    assert site['count'] == N and min(power) >= 15, power
    assert worst <= 1.0


def test_sums_with_the_predictive_check_on_in_the_regime():
    """k_z_ob_ppc with the site and the log-likelihood sums on: every iteration is the one kept draw of a run(1, 0)."""
    _accumulate(2, ppc=True)


def test_generic_kernels_sums_in_the_regime():
    """p = q = 9: the generic kernels (z_update_site_g, z_update_site_ll through it)."""
    _accumulate(9, ppc=False)
