"""Sampler base class: the public API of the reference's ``occuspytial/gibbs/base.py``.

``GibbsBase`` keeps the reference's constructor, attributes (``state``, ``fixed``, ``dists``, ``rng``,
``chain``), ``sample`` / ``copy`` / ``step`` contract and error messages.  What changes is where the
work happens: a subclass that provides ``_run_chains`` (as :class:`LogitICARGibbs` does) hands all
chains to the HIP engine in one batch instead of forking one process per chain
(reference ``gibbs/parallel.py:38-41``).
"""
import numpy as np
from scipy.sparse import csc_matrix, isspmatrix_csc

from .._problem import FlatProblem, default_start
from ..chain import Chain
from ..data import Data
from ..graph import CONSTRAINTS
from ..posterior import PosteriorParameter
from ..utils import get_generator
from . import options
from .parallel import sample_parallel
from .state import FixedState, State


class _GibbsState(State):
    """Sampler state whose ``posteriors`` are the recorded parameters (reference base.py:15-27)."""

    _posterior_names = ('alpha', 'beta', 'tau')

    @property
    def posteriors(self):
        return {name: self.__dict__[name] for name in self._posterior_names}


class GibbsBase:
    """Base class of the Gibbs samplers for spatial occupancy models.

    Parameters follow the reference (``base.py:30-82``): ``Q`` spatial precision (sparse or dense),
    ``W`` / ``y`` dictionaries keyed by surveyed site, ``X`` the ``n x p`` occupancy design,
    ``hparams`` optional hyper-parameter dict, ``random_state`` None | int | SeedSequence.
    """

    def __init__(self, Q, W, X, y, hparams=None, random_state=None):
        self.W = Data(W)
        self.X = X
        self.y = Data(y)
        self.rng = get_generator(random_state)

    def step(self):
        raise NotImplementedError(f'{self.__class__.__name__} must implement a `step` method.')

    # ------------------------------------------------------------------ configuration (base.py:107-186)
    def _check_constraint(self, constraint, carries_none=None):
        """Refuse a ``constraint`` this sampler cannot honour, before a problem or an engine exists: any value but
        ``'global'`` and ``'component'``; ``'component'`` for a sampler whose spatial effect carries no sum-to-zero constraint
        (``carries_none`` says why) or that steps in Python (the per-component projection is the engine's)."""
        if constraint not in CONSTRAINTS:
            raise ValueError("constraint must be 'global' or 'component'")
        if constraint == 'component' and carries_none:
            raise ValueError(f"{self.__class__.__name__} has no constraint='component': {carries_none}")
        if constraint == 'component' and not hasattr(self, '_run_chains'):
            raise ValueError(f"{self.__class__.__name__} steps in Python: constraint='component' is applied by the engine's "
                             'correction pass behind the eta solve')

    def _configure(self, Q, hparams, verify_precision=True, prior_draw='auto', constraint='global', **kwargs):
        self._check_constraint(constraint)
        prob = FlatProblem(Q, self.W._data, self.X, self.y._data, hparams, check_singular=verify_precision, prior_draw=prior_draw,
                           constraint=constraint)
        self._problem = prob

        self.state = _GibbsState()
        self.state.z = prob.z0.copy()
        self.state.k = self.state.z - 0.5

        fixed = FixedState()
        fixed.Q = Q if isspmatrix_csc(Q) else csc_matrix(Q)
        fixed.n = prob.n
        fixed.ones = np.ones(prob.n)
        fixed.not_surveyed = prob.not_surveyed
        fixed.not_obs = prob.not_obs
        fixed.obs = prob.obs
        fixed.n_no = len(prob.not_obs)
        fixed.n_ns = len(prob.not_surveyed)
        fixed.W_not_obs = self.W[prob.not_obs] if prob.not_obs else np.zeros((0, prob.q))
        fixed.visits_not_obs = self.W.visits(prob.not_obs)
        sections = np.cumsum(fixed.visits_not_obs, dtype=np.int64)
        fixed.stacked_w_indices = np.concatenate([[0], sections])[:-1].astype(np.int64)
        if hparams:
            # user keys are set verbatim first, like base.py:172-175 (tests read them back unchanged)
            for key, value in hparams.items():
                setattr(fixed, key, value)
        for key in ('tau_rate', 'tau_shape', 'a_mu', 'a_prec', 'b_mu', 'b_prec'):
            if key not in fixed.__dict__:
                setattr(fixed, key, prob.hparams[key])
        fixed.a_prec_by_mu = prob.a_prec @ prob.a_mu
        fixed.b_prec_by_mu = prob.b_prec @ prob.b_mu
        self.fixed = fixed
        self.dists = FixedState()

    # ------------------------------------------------------------------ start values (base.py:188-212)
    def _initialize_posterior_state(self, start=None):
        if start is None:
            self._initialize_default_start(self.state)
        else:
            self.state.alpha = start['alpha']
            self.state.beta = start['beta']
            self.state.tau = start['tau']
            self.state.eta = start['eta']
            self.state.spatial = self.state.eta

    def _initialize_default_start(self, state):
        """Default start, drawn from ``self.rng`` in the reference's order (base.py:199-212):
        gamma for tau, n normals for eta (centred), then alpha and beta from
        ``multivariate_normal(mu, 100 * prec, method='cholesky')`` -- ``100 * prec`` used as a
        covariance, as the reference does."""
        st = default_start(self.rng, self._problem)
        state.tau, state.eta, state.spatial = st['tau'], st['eta'], st['eta']
        state.alpha, state.beta = st['alpha'], st['beta']
        return state

    # ------------------------------------------------------------------ generic single-chain loop (base.py:214-241)
    def _run(self, size, burnin=0, start=None, chains=2, progressbar=True, pos=0):
        from tqdm.auto import tqdm

        self._initialize_posterior_state(start)
        dims = {'alpha': np.size(self.state.alpha), 'beta': np.size(self.state.beta), 'tau': 1}
        self.chain = Chain(dims, size - burnin)
        for i in tqdm(range(size), total=size, disable=not progressbar, position=pos):
            self.step()
            if i >= burnin:
                self.chain.append(self.state.posteriors)
        return self.chain

    def sample(self, size, burnin=0, start=None, chains=2, progressbar=True, site_summaries=False, waic=False, regions=None,
               ppc=False, spatial_check=False, site_intervals=False, site_diagnostics=False, holdout=None):
        """Draw ``size`` iterations per chain and return the kept ``alpha``, ``beta``, ``tau`` draws.

        Same contract as the reference (``base.py:243-291``): ``burnin < size`` else ``ValueError``;
        ``chains >= 1`` else ``ValueError``; ``start`` may give ``alpha``, ``beta``, ``tau``, ``eta``;
        the result indexes as ``out['alpha'] -> (chains, size - burnin, q)`` etc.

        ``site_summaries=True`` (samplers that run on the engine; logit link) additionally accumulates the per-site
        posterior map on the device over the kept iterations -- occupancy probability, P(z = 1 | data), the spatial effect
        and its sd -- and returns it as ``out.sites``, a :class:`~occuspytial_amd.sites.SiteSummary` (``None`` otherwise).

        ``waic=True`` (the same samplers) accumulates, over the same iterations, every surveyed site's marginal likelihood
        and log-likelihood (z integrated out) on the device and returns ``out.waic``, a :class:`~occuspytial_amd.waic.WAIC`
        (``None`` otherwise): compare two fits with :func:`occuspytial_amd.waic.compare`.

        ``regions`` (every sampler that runs on the engine, the probit one included): ``True`` -- the whole lattice as one
        region -- or an integer array with the region of every site, ``-1`` for none.  The device then counts, per kept
        draw, the occupied sites of every region: ``out['occupied']`` is ``(chains, size - burnin, G)``, it appears in
        ``out.summary`` (mean, sd, HDI, ESS, R-hat of the finite-sample occupancy), and ``out.regions`` is a
        :class:`~occuspytial_amd.regions.RegionOccupancy` (sizes, detected sites, proportion of area occupied).

        ``ppc=True`` (samplers that run on the engine; logit link): per kept draw the device replicates every surveyed
        site's detections from the draw's z and alpha and records the Freeman-Tukey discrepancy of the observed and of the
        replicated data; ``out.ppc`` is a :class:`~occuspytial_amd.ppc.PredictiveCheck` (Bayesian p-value, lack-of-fit
        ratio; ``None`` otherwise).  ``out.summary`` and the chains are unchanged.

        ``spatial_check=True`` (likewise): per kept draw the device forms Moran's I of the occupancy residuals
        ``z - psi`` and of one replicate of them; ``out.spatial_check`` is a
        :class:`~occuspytial_amd.spatial.SpatialCheck` (tail probability, excess autocorrelation; ``None`` otherwise).

        ``site_intervals=True`` (likewise; or a number of bins from 4 to 1024, ``True`` is 64): over the kept iterations
        the device keeps, per site, a histogram of the occupancy probability psi; ``out.site_intervals`` is a
        :class:`~occuspytial_amd.intervals.SiteIntervals` (credible intervals, quantiles and exceedance probabilities of
        psi per site, to within one bin; ``None`` otherwise).

        ``site_diagnostics=True`` (likewise; or a batch length from 1 to 2^30, ``True`` is ``floor(sqrt(size - burnin))``):
        over the kept iterations the device keeps, per site, batch-means sums of psi and of the spatial effect eta;
        ``out.site_diagnostics`` is a :class:`~occuspytial_amd.convergence.SiteDiagnostics` (R-hat across chains, effective
        sample size and Monte-Carlo standard error per site, and the worst sites; ``None`` otherwise).

        ``holdout=(W_test, y_test)`` (likewise): the withheld visits of sites this sampler does NOT survey, as dicts keyed
        by site like the constructor's ``W`` and ``y``.  Over the kept iterations the device adds, per held-out site, the
        predictive density of its withheld detection history; ``out.holdout`` is a
        :class:`~occuspytial_amd.holdout.HoldoutScore` (expected log predictive density with its standard error, Brier
        score and AUC of the predicted detections; ``None`` otherwise).  :func:`occuspytial_amd.holdout.split` makes the
        folds of a K-fold run and :func:`occuspytial_amd.holdout.combine` joins their scores.
        """
        given = dict(locals())
        first = options.parse_first(given, self._problem, size - burnin)
        if burnin >= size:
            raise ValueError('burnin value cannot be larger than sample size')
        if chains < 1:
            raise ValueError('chains must a positive integer.')
        asked = options.ask(self, given, size - burnin, first)
        extra = {'asked': asked} if asked else {}   # (with the defaults, no keyword about them goes on)
        samples = sample_parallel(self, size=size, burnin=burnin, chains=chains, start=start, progressbar=progressbar, **extra)
        out = PosteriorParameter(*samples)
        for result, value in self.__dict__.pop('_outputs', {}).items():   # (what _run_chains made of the options asked)
            setattr(out, result, value)
        return out

    def _refusal(self, option):
        """Why this sampler refuses an optional output (a row of ``options.OPTIONS``), or None.  Every one of them is formed on
        the device behind the engine's z update: a sampler with a Python ``step`` has none."""
        return None if hasattr(self, '_run_chains') else f'{self.__class__.__name__} {option.python_step}'

    def copy(self):
        """A shallow copy with its own generator spawned from this one's seed sequence
        (reference ``base.py:293-306``: child ``spawn_key=(j,)``, the counter persists across calls)."""
        out = type(self).__new__(self.__class__)
        out.__dict__.update(self.__dict__)
        seed_seq = self.rng.bit_generator.seed_seq.spawn(1)[0]
        out.__dict__['rng'] = get_generator(seed_seq)
        # per-object caches must not be shared with the copy
        out.__dict__.pop('_engine', None)
        return out
