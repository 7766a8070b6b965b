"""``ProbitRSRGibbs`` on the MI355X engine (API of reference ``occuspytial/gibbs/probit.py``).

The reference's class is importable but does not run: its beta update passes the fixed precision ``X'X + b_prec`` to
``precision_mvnorm``, which overwrites it with its Cholesky factor, so from the second iteration on beta is drawn from a
corrupted precision and diverges; and its truncated-normal inverse CDF overflows to +-inf past |loc| ~ 38.  This class is
the same model with both fixed (DESIGN.md "ProbitRSRGibbs").
"""
import numpy as np

from .._engine import Engine
from .logit import LogitICARGibbs
from .base import GibbsBase

MAX_BASIS = 4096


class ProbitRSRGibbs(GibbsBase):
    r"""Gibbs sampler, probit link, reduced-rank (RSR) spatial random effects -- computed on an AMD MI355X.

    Drop-in for the reference class of the same name: ``ProbitRSRGibbs(Q, W, X, y, hparams=None, random_state=None,
    r=0.5, q=None)``.  The basis ``K`` (eigenvectors of the Moran operator with eigenvalues of at least ``r``, or the ``q``
    leading ones), ``fixed.Q`` (= :math:`K^\top QK`), ``fixed.KTK``, ``fixed.q``, ``fixed.XTX_plus_bprec`` and the default
    ``tau_shape = 0.5 + 0.5 q`` are the reference's.  ``state.eta`` holds :math:`\theta`, ``state.spatial`` :math:`K\theta`,
    ``state.eps`` the site-level noise.  One iteration is the reference's eight conditional updates in its order
    (:math:`\omega_b, \tau, \epsilon, \theta, \beta, \omega_a, \alpha, z`); the beta precision is never overwritten and the
    truncated normals are drawn stably for any location.  Per iteration the device makes two passes over one n x m matrix
    and no factorisation (``csrc/occ_probit.hpp``).  ``device`` selects the HIP device; the chains of one ``sample`` call run
    batched on it.  At most 4 096 basis columns and 8 covariates of each kind.  ``basis='device'`` builds K on the device
    without any n x n array (``occuspytial_amd.basis.moran_basis``; the same span, columns defined up to sign and up to a
    rotation inside a cluster of near-equal eigenvalues); any value but ``'host'`` and ``'device'`` is refused.
    """

    def __init__(self, Q, W, X, y, hparams=None, random_state=None, r=0.5, q=None, device=0, basis='host', constraint='global'):
        if basis not in ('host', 'device'):
            raise ValueError("basis must be 'host' or 'device'")
        self._check_constraint(constraint, 'its spatial effect K theta carries no sum-to-zero constraint')
        super().__init__(Q, W, X, y, hparams, random_state)
        self.devices = None
        self.device = device
        self._configure(Q, hparams, q, r, basis)

    def _configure(self, Q, hparams, q, r, basis='host'):
        super()._configure(Q, hparams, prior_draw='edge')
        prob = self._problem
        if prob.p > 8 or prob.q > 8:
            raise ValueError('the probit model takes at most 8 occupancy and 8 detection covariates')
        pb = prob.enable_probit(r=r, q=q, default_tau_shape=not hparams, basis=basis, device=self.device)
        m = pb['dim']
        if m > MAX_BASIS:
            raise ValueError(f'{m} basis columns selected; the device path supports at most {MAX_BASIS} '
                             '(raise the threshold `r` or pass `q`)')
        fixed = self.fixed
        fixed.XTX_plus_bprec = self._problem.X.T @ self._problem.X + prob.b_prec
        fixed.eps_chol_factor = np.ones(prob.n) / np.sqrt(2)
        fixed.q = m
        fixed.KTK = pb['KTK']
        del fixed.Q
        fixed.Q = pb['Q']
        fixed.K = pb['K']
        if not hparams:
            del fixed.tau_shape
            fixed.tau_shape = prob.tau_shape
        self.state.omega_b = np.zeros(prob.n)

    # ------------------------------------------------------------------ start values (reference probit.py)
    def _initialize_default_start(self, state):
        state = super()._initialize_default_start(state)
        state.eta = self.rng.normal(scale=5, size=self.fixed.q)
        state.spatial = self.fixed.K @ state.eta
        state.eps = self.rng.standard_normal(self.fixed.n)
        return state

    def _initialize_posterior_state(self, start=None):
        if start is None:
            self._initialize_default_start(self.state)
        else:
            self.state.alpha = start['alpha']
            self.state.beta = start['beta']
            self.state.tau = start['tau']
            self.state.eta = start['eta']
            self.state.eps = start['eps']
            self.state.spatial = self.fixed.K @ np.asarray(self.state.eta, dtype=float)

    # ------------------------------------------------------------------ engine management: LogitICARGibbs's, on one device
    def _get_engine(self, keys):
        eng = self.__dict__.get('_engine')
        if eng is None or eng.n_chains != len(keys):
            if eng is not None:
                eng.close()
            eng = Engine(self._problem, keys, device=self.device)
            self.__dict__['_engine'] = eng
        else:
            eng.set_keys(keys)
        return eng

    def _push_start(self, eng, chain, state):
        LogitICARGibbs._push_start(self, eng, chain, state)
        eng.set('eps', np.asarray(state.eps, dtype=float), chain)

    def _pull_state(self, eng, chain=0):
        LogitICARGibbs._pull_state(self, eng, chain)
        st = self.state
        st.eps = eng.get('eps', chain)

    def _refusal(self, option):
        return option.probit   # (None where this model allows the option: the rows of gibbs/options.py say which and why)

    step = LogitICARGibbs.step
    checkpoint = LogitICARGibbs.checkpoint
    resume = LogitICARGibbs.resume
    _run_chains = LogitICARGibbs._run_chains
