"""``LogitICARGibbs`` on the MI355X engine (API of reference ``occuspytial/gibbs/logit.py:102-266``)."""
import numpy as np

from .. import _lib
from .._engine import Engine, EngineGroup
from ..chain import Chain
from ..convergence import SiteDiagnostics, diagnostics_batch
from ..holdout import HoldoutScore, holdout_arg
from ..intervals import SiteIntervals, interval_bins
from ..ppc import PredictiveCheck, ppc_flag
from ..regions import region_ids
from ..sites import SiteSummary
from ..spatial import SpatialCheck, spatial_flag
from ..waic import WAIC
from .base import GibbsBase

SUMS_RESULT = {'site': SiteSummary, 'll': WAIC}   # kind of per-site sums (_lib.SUMS_KINDS) -> what a result holds of them


def _philox_key(rng):
    """64-bit key of a chain's device streams: the next raw word of the chain's own SFC64 stream,
    taken AFTER its start values were drawn, so chains and repeated runs never share a key."""
    return int(rng.bit_generator.random_raw())


class LogitICARGibbs(GibbsBase):
    r"""Gibbs sampler, logit link, ICAR spatial random effects -- computed on an AMD MI355X.

    Drop-in for the reference class of the same name (``logit.py:102-174``): same constructor
    ``(Q, W, X, y, hparams=None, random_state=None)``, same ``sample`` / ``step`` / ``copy``, same
    ``state`` / ``fixed`` attributes and error behaviour.  One iteration performs the reference's seven
    conditional updates in its order (``logit.py:254-266``): :math:`\omega_b`, :math:`\tau`,
    :math:`\eta`, :math:`\beta`, :math:`\omega_a`, :math:`\alpha`, :math:`z`.

    Differences that are visible to a user, all documented in DESIGN.md:

    * variates come from counter-based Philox streams keyed per chain, not from one sequential SFC64
      stream, so draws are equal to the reference's in distribution, not value for value;
    * the prior term of the :math:`\eta` conditional uses the edge factorisation
      :math:`Q = B^\top B` instead of a dense eigenfactor (``logit.py:66-67``): no O(n^2) memory, no
      O(n^3) set-up, for any ICAR precision (zero row sums, non-positive off-diagonals).  ``prior_draw='dense'``
      selects the reference's own form instead (dense ``eigh`` on the host, one dense matrix-vector product per
      iteration on the device); ``'auto'`` takes it by itself for a singular positive semi-definite ``Q`` that is
      not an ICAR precision, which the edge form cannot represent;
    * ``device`` selects the HIP device; all chains of one ``sample`` call run batched on it.  ``devices=[...]``
      instead fans the chains of ``sample(chains=N)`` out over several GPUs from this process, chain ``c`` on
      ``devices[c % len(devices)]`` -- the reference's one-process-per-chain fan-out (``gibbs/parallel.py:20-41``) with
      GPUs for processes: the problem is uploaded once and broadcast device to device over RCCL, every GPU is driven by
      its own host thread, and chain ``k`` still owns the generator the reference would give it, so the draws do not
      depend on how many devices share the work.
    """

    def __init__(self, Q, W, X, y, hparams=None, random_state=None, device=0, devices=None, prior_draw='auto'):
        super().__init__(Q, W, X, y, hparams, random_state)
        self.devices = [int(d) for d in devices] if devices is not None else None
        self.device = self.devices[0] if self.devices else device
        self._configure(Q, hparams, prior_draw=prior_draw)

    def _configure(self, Q, hparams, prior_draw='auto'):
        super()._configure(Q, hparams, prior_draw=prior_draw)

    # ------------------------------------------------------------------ engine management
    def _get_engine(self, keys):
        eng = self.__dict__.get('_engine')
        if eng is None or eng.n_chains != len(keys):
            if eng is not None:
                eng.close()
            if self.devices and len(self.devices) > 1 and len(keys) > 1:   # chains sharded over the GPUs of this process
                eng = EngineGroup(self._problem, keys, self.devices)
            else:
                eng = Engine(self._problem, keys, device=self.device)
            self.__dict__['_engine'] = eng
        else:
            eng.set_keys(keys)
        return eng

    def _push_start(self, eng, chain, state):
        eng.set_start(chain, np.atleast_1d(np.asarray(state.alpha, dtype=float)),
                      np.atleast_1d(np.asarray(state.beta, dtype=float)), float(state.tau),
                      np.asarray(state.eta, dtype=float))

    def _pull_state(self, eng, chain=0):
        """Mirror the device state of one chain into ``self.state`` (reference attribute names)."""
        st = self.state
        st.alpha = eng.get('alpha', chain)
        st.beta = eng.get('beta', chain)
        st.tau = float(eng.get('tau', chain))
        if self._problem.rsr is None:
            st.eta = eng.get('eta', chain)
            st.spatial = st.eta
        else:   # reduced-rank model: eta holds the basis coefficients, spatial = K eta (logit.py:484-485)
            st.eta = eng.get('theta', chain)
            st.spatial = eng.get('eta', chain)
        st.z = eng.get('z', chain)
        st.k = st.z - 0.5
        st.omega_b = eng.get('omega_b', chain)
        prob = self._problem
        exists_flag = eng.get('exists', chain).astype(bool)
        # reference order (logit.py:187-188): sites with a detection first, then newly occupied ones
        obs = prob.obs_site.astype(bool)
        order = np.concatenate([np.flatnonzero(obs), np.flatnonzero(exists_flag & ~obs)])
        st.exists = [prob.surveyed[i] for i in order]
        rows = [np.arange(prob.site_ptr[i], prob.site_ptr[i + 1]) for i in order]
        rows = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
        st.omega_a = eng.get('omega_a', chain)[rows]
        st.W = prob.W[rows]

    # ------------------------------------------------------------------ public stepping (logit.py:254-266)
    def step(self):
        """One Gibbs iteration of this sampler's own chain (its state must have start values:
        ``sample`` sets them, or call ``_initialize_posterior_state`` first, as ``_run`` does)."""
        if 'alpha' not in self.state.__dict__:
            self._initialize_posterior_state(None)
        eng = self.__dict__.get('_engine')
        if eng is None or eng.n_chains != 1 or not self.__dict__.get('_stepping'):
            eng = self._get_engine([_philox_key(self.rng)])
            self._push_start(eng, 0, self.state)
            eng.set('z', self.state.z, 0)
            self.__dict__['_stepping'] = True
        eng.step()
        self._pull_state(eng, 0)

    # ------------------------------------------------------------------ checkpoint / resume
    def checkpoint(self, path=None):
        """State of every chain of the last :meth:`sample` call, sufficient to continue each of them exactly
        (``Engine.checkpoint``).  Returns a dict of arrays; ``path`` additionally writes it as ``.npz``."""
        eng = self.__dict__.get('_engine')
        if eng is None:
            raise RuntimeError('nothing to checkpoint: call sample() first')
        ckpt = eng.checkpoint()
        if path is not None:
            np.savez(path, **ckpt)
        return ckpt

    def _sums_switch(self, eng, kind, on):
        try:
            eng.sums_switch(kind, on)
        except ValueError as exc:   # a stale build, or a stand-in library that does not know the state names
            raise ValueError(f'the loaded engine library has no {_lib.SUMS_KINDS[kind].what} ({exc}): rebuild it') from None

    def _regions_call(self, call):
        try:
            return call()
        except ValueError as exc:   # a stale build, or a stand-in library that does not know the state names
            raise ValueError(f'the loaded engine library does not count the occupied sites per region ({exc}): rebuild it') from None

    def _ppc_switch(self, eng, on):
        try:
            eng.ppc_stats(on)
        except ValueError as exc:   # a stale build, or a stand-in library that does not know the state names
            raise ValueError(f'the loaded engine library has no posterior predictive check ({exc}): rebuild it') from None

    def _moran_switch(self, eng, on):
        try:
            eng.moran_stats(on)
        except ValueError as exc:   # a stale build, or a stand-in library that does not know the state names
            raise ValueError(f'the loaded engine library has no spatial residual check ({exc}): rebuild it') from None

    def _hist_switch(self, eng, bins):
        try:
            eng.hist_stats(bins)
        except ValueError as exc:   # a stale build, or a stand-in library that does not know the state names
            raise ValueError(f'the loaded engine library has no site intervals ({exc}): rebuild it') from None

    def _conv_switch(self, eng, batch):
        try:
            eng.conv_stats(batch)
        except ValueError as exc:   # a stale build, or a stand-in library that does not know the state names
            raise ValueError(f'the loaded engine library has no site diagnostics ({exc}): rebuild it') from None

    def _holdout_call(self, call):
        try:
            return call()
        except ValueError as exc:   # a stale build, or a stand-in library that does not know the state names
            raise ValueError(f'the loaded engine library has no held-out scoring ({exc}): rebuild it') from None

    def resume(self, checkpoint, size, progressbar=True, site_summaries=False, waic=False, regions=None, ppc=False,
               spatial_check=False, site_intervals=False, site_diagnostics=False, holdout=None):
        """Continue the chains of ``checkpoint`` (a dict from :meth:`checkpoint` or the path of its ``.npz``)
        for ``size`` more iterations on this sampler's problem.  Returns a ``PosteriorParameter`` of the new
        draws; every chain's ``Chain`` is the continuation (use ``Chain.expand`` / ``append`` to join them to
        earlier draws).  The result equals the tail of an uninterrupted run bit for bit.  ``site_summaries=True``: the
        per-site sums go on from those the checkpoint holds (from zero if it holds none); the result's ``sites`` covers
        every iteration accumulated so far, those before the checkpoint included.  ``waic=True``: the same for the
        log-likelihood sums and the result's ``waic``.  ``regions`` (as in :meth:`sample`): the occupied sites per region of
        the new draws, ``out['occupied']`` and ``out.regions``; the draws belong to a call, so nothing of them is carried.
        ``ppc=True``: the posterior predictive check of the new draws, ``out.ppc``; likewise nothing of it is carried.
        ``spatial_check=True``: the spatial residual check of the new draws, ``out.spatial_check``; likewise.
        ``site_intervals`` (as in :meth:`sample`): the per-site histograms of psi go on from those the checkpoint holds
        (from zero if it holds none, or holds another number of bins); ``out.site_intervals`` covers every iteration
        accumulated so far.
        ``site_diagnostics`` (as in :meth:`sample`): the per-site batch-means sums go on from those the checkpoint holds,
        with the checkpoint's batch length whatever is asked for here (from zero if it holds none: ``True`` is then
        ``floor(sqrt(size))``); ``out.site_diagnostics`` covers every iteration accumulated so far.
        ``holdout`` (as in :meth:`sample`): the held-out sums go on from those the checkpoint holds if it holds them for
        the same withheld data (from zero otherwise); ``out.holdout`` covers every iteration accumulated so far."""
        from ..posterior import PosteriorParameter
        from tqdm.auto import tqdm
        bins = interval_bins(site_intervals)
        batch = diagnostics_batch(site_diagnostics, size)
        if isinstance(checkpoint, (str, bytes)) or hasattr(checkpoint, '__fspath__'):
            with np.load(checkpoint) as f:
                checkpoint = {k: f[k] for k in f.files}
        if size < 1:
            raise ValueError('size must be a positive integer')
        ids = region_ids(regions, self._problem.n)
        if ids is not None:
            self._refuse_regions()
        ppc = ppc_flag(ppc)
        if ppc:
            self._refuse_ppc()
        spatial_check = spatial_flag(spatial_check)
        if spatial_check:
            self._refuse_spatial_check()
        if bins:
            self._refuse_site_intervals()
        if batch:
            self._refuse_site_diagnostics()
        if holdout is not None:
            self._refuse_holdout()
            holdout = holdout_arg(holdout, self._problem)
        C = int(checkpoint['n_chains'])
        self.__dict__['_stepping'] = False
        eng = self._get_engine([int(k) for k in np.asarray(checkpoint['keys'])])
        eng.restore(checkpoint)
        kinds = self._sums_asked(site_summaries=site_summaries, waic=waic)
        for kind in kinds:
            self._refuse_sums(kind)
            if _lib.SUMS_KINDS[kind].fields[0] not in checkpoint:
                self._sums_switch(eng, kind, True)
        if ids is not None:
            self._regions_call(lambda: (eng.regions(ids), eng.region_stats(True)))
            occupied = np.zeros((C, size, max(int(ids.max()) + 1, 1)))
        if ppc:
            self._ppc_switch(eng, True)
            ppc_rows = np.zeros((C, size, 4))
        elif getattr(eng, '_ppc_on', False):   # (the checkpoint's switch was on: this call did not ask)
            eng.ppc_stats(False)
        if spatial_check:
            self._moran_switch(eng, True)
            moran_rows = np.zeros((C, size, 8))
        elif getattr(eng, '_moran_on', False):   # (the checkpoint's switch was on: this call did not ask)
            eng.moran_stats(False)
        if bins:
            if getattr(eng, '_hist_bins', 0) != bins:   # (the checkpoint holds none, or of another number of bins: from zero)
                self._hist_switch(eng, bins)
        elif getattr(eng, '_hist_bins', 0):   # (the checkpoint's switch was on: this call did not ask)
            eng.hist_stats(0)
        if batch:
            if not getattr(eng, '_conv_batch', 0):   # (the checkpoint holds none: from zero; otherwise its batch length stays)
                self._conv_switch(eng, batch)
        elif getattr(eng, '_conv_batch', 0):   # (the checkpoint's switch was on: this call did not ask)
            eng.conv_stats(0)
        if holdout is not None:
            if not (getattr(eng, '_holdout_on', False) and np.array_equal(eng._holdout, holdout)):   # (none, or of other data: from zero)
                self._holdout_call(lambda: (eng.holdout_data(holdout), eng.holdout_stats(True)))
        elif getattr(eng, '_holdout_on', False):   # (the checkpoint's switch was on: this call did not ask)
            eng.holdout_stats(False)
        alpha = np.zeros((C, size, self._problem.q))
        beta = np.zeros((C, size, self._problem.p))
        tau = np.zeros((C, size))
        bar = tqdm(total=size, disable=not progressbar)
        chunk = size if not progressbar else max(1, min(size, max(16, size // 25)))
        done = 0
        while done < size:
            step = min(chunk, size - done)
            alpha[:, done:done + step], beta[:, done:done + step], tau[:, done:done + step] = eng.run(step, 0)
            if ids is not None:
                occupied[:, done:done + step] = [eng.region_draws(c) for c in range(C)]
            if ppc:
                ppc_rows[:, done:done + step] = [eng.ppc_draws(c) for c in range(C)]
            if spatial_check:
                moran_rows[:, done:done + step] = [eng.moran_draws(c) for c in range(C)]
            done += step
            bar.update(step)
        bar.close()
        extra = {'occupied': occupied} if ids is not None else {}
        chains = [Chain._from_arrays({'alpha': alpha[c], 'beta': beta[c], 'tau': tau[c], **{k: v[c] for k, v in extra.items()}},
                                     vectors=tuple(extra)) for c in range(C)]
        self.chain = chains[0]
        self._pull_state(eng, 0)
        out = PosteriorParameter(*chains)
        for kind in kinds:
            setattr(out, _lib.SUMS_KINDS[kind].result, SUMS_RESULT[kind].from_engine(eng))
        if ids is not None:
            out.regions = self._region_result(ids, out)
        if ppc:
            out.ppc = PredictiveCheck.from_problem(self._problem, ppc_rows)
        if spatial_check:
            out.spatial_check = SpatialCheck.from_problem(self._problem, moran_rows)
        if bins:
            out.site_intervals = SiteIntervals.from_engine(eng)
        if batch:
            out.site_diagnostics = SiteDiagnostics.from_engine(eng)
        if holdout is not None:
            out.holdout = HoldoutScore.from_engine(eng)
        return out

    # ------------------------------------------------------------------ batched chains
    def _run_chains(self, samplers, size, burnin=0, start=None, progressbar=True, site_summaries=False, waic=False, regions=None,
                    ppc=False, spatial_check=False, site_intervals=False, site_diagnostics=False, holdout=None):
        """All chains of one ``sample`` call as one device batch.

        Mirrors ``GibbsBase._run`` (base.py:214-241) per chain: start values from the chain's own
        generator (or the ``start`` dict), then ``size`` iterations keeping those ``>= burnin``.
        ``site_summaries``: burn-in chunks run with the engine's per-site sums switched off; the switch goes on (which
        zeroes them) right before the first chunk that keeps a draw, and inside that chunk the engine itself counts
        only the iterations past the chunk's burn-in.  With the default no call about them reaches the engine.
        ``waic``: the log-likelihood sums, switched in exactly the same way.
        ``regions`` (an array of region ids, or None): the count of occupied sites per region, switched in the same way; every
        chunk's rows are appended to the chains' ``occupied``.  With the default no call about it reaches the engine.
        ``ppc``: the posterior predictive check, switched in the same way; every chunk's rows are appended and the
        :class:`~occuspytial_amd.ppc.PredictiveCheck` made of them is left for ``sample``.  With the default no call about
        it reaches the engine.
        ``spatial_check``: the spatial residual check, switched in the same way; every chunk's rows are appended and the
        :class:`~occuspytial_amd.spatial.SpatialCheck` made of them is left for ``sample``.  With the default no call about
        it reaches the engine.
        ``site_intervals`` (a number of bins, or False): the per-site histograms of psi, switched as the site sums are -- off
        during burn-in chunks, on (which zeroes them) before the first chunk that keeps a draw; they accumulate on the
        device and the :class:`~occuspytial_amd.intervals.SiteIntervals` read from the engine at the end is left for
        ``sample``.  With the default no call about them reaches the engine.
        ``site_diagnostics`` (a batch length, or False): the per-site batch-means sums of psi and eta, switched in the same
        way; the :class:`~occuspytial_amd.convergence.SiteDiagnostics` read from the engine at the end is left for ``sample``.
        With the default no call about them reaches the engine.
        ``holdout`` (the packed withheld data, or None): the held-out sums, switched in the same way -- the data are set with
        every chain off before the first chunk; the :class:`~occuspytial_amd.holdout.HoldoutScore` read from the engine at
        the end is left for ``sample``.  With the default no call about them reaches the engine.
        """
        from tqdm.auto import tqdm

        for s in samplers:
            if s is not self:  # copies share `state` by reference in the reference too; give each its own
                s.__dict__['state'] = type(self.state)(**self.state.__dict__)
            s._initialize_posterior_state(start)
        keys = [_philox_key(s.rng) for s in samplers]
        self.__dict__['_stepping'] = False
        eng = self._get_engine(keys)
        z0 = self._problem.z0
        for c, s in enumerate(samplers):
            self._push_start(eng, c, s.state)
            eng.set('z', z0, c)
        kinds = self._sums_asked(site_summaries=site_summaries, waic=waic)
        for kind in _lib.SUMS_KINDS:
            if kind in kinds or getattr(eng, '_sums_on', {}).get(kind):   # (a reused engine that an earlier call left switched on)
                self._sums_switch(eng, kind, False)   # (also the early answer of a library that does not know the kind)
        if regions is not None:   # (sets the map with every chain's switch off)
            self._regions_call(lambda: eng.regions(regions))
        elif getattr(eng, '_region_on', False):   # (a reused engine that an earlier call left counting)
            eng.region_stats(False)
        if ppc or getattr(eng, '_ppc_on', False):   # (off during burn-in; a reused engine that an earlier call left on)
            self._ppc_switch(eng, False)
        if spatial_check or getattr(eng, '_moran_on', False):   # (likewise)
            self._moran_switch(eng, False)
        if site_intervals or getattr(eng, '_hist_bins', 0):   # (likewise)
            self._hist_switch(eng, 0)
        if site_diagnostics or getattr(eng, '_conv_batch', 0):   # (likewise)
            self._conv_switch(eng, 0)
        if holdout is not None:   # (sets the data with every chain's switch off)
            self._holdout_call(lambda: eng.holdout_data(holdout))
        elif getattr(eng, '_holdout_on', False):   # (a reused engine that an earlier call left on)
            eng.holdout_stats(False)
        sums_on = False

        C = len(samplers)
        keep = size - burnin
        extra = {'occupied': np.zeros((C, keep, max(int(regions.max()) + 1, 1)))} if regions is not None else {}
        ppc_rows = np.zeros((C, keep, 4)) if ppc else None
        moran_rows = np.zeros((C, keep, 8)) if spatial_check else None
        alpha = np.zeros((C, keep, self._problem.q))
        beta = np.zeros((C, keep, self._problem.p))
        tau = np.zeros((C, keep))
        bars = [tqdm(total=size, disable=not progressbar, position=pos) for pos in range(C)]
        chunk = size if not progressbar else max(1, min(size, max(16, size // 25)))
        done = kept = 0
        while done < size:
            step = min(chunk, size - done)
            b = min(max(burnin - done, 0), step)
            if b == step:  # the whole chunk is burn-in: run it, keep only its last draw, drop it
                eng.run(step, step - 1)
            else:
                if not sums_on:
                    for kind in kinds:
                        self._sums_switch(eng, kind, True)
                    if regions is not None:
                        eng.region_stats(True)
                    if ppc:
                        eng.ppc_stats(True)
                    if spatial_check:
                        eng.moran_stats(True)
                    if site_intervals:
                        eng.hist_stats(site_intervals)
                    if site_diagnostics:
                        eng.conv_stats(site_diagnostics)
                    if holdout is not None:
                        eng.holdout_stats(True)
                    sums_on = True
                a_, b_, t_ = eng.run(step, b)
                m = step - b
                alpha[:, kept:kept + m], beta[:, kept:kept + m], tau[:, kept:kept + m] = a_, b_, t_
                if regions is not None:
                    extra['occupied'][:, kept:kept + m] = [eng.region_draws(c) for c in range(C)]
                if ppc:
                    ppc_rows[:, kept:kept + m] = [eng.ppc_draws(c) for c in range(C)]
                if spatial_check:
                    moran_rows[:, kept:kept + m] = [eng.moran_draws(c) for c in range(C)]
                kept += m
            done += step
            for bar in bars:
                bar.update(step)
        for bar in bars:
            bar.close()

        chains = []
        for c, s in enumerate(samplers):
            ch = Chain._from_arrays({'alpha': alpha[c], 'beta': beta[c], 'tau': tau[c], **{k: v[c] for k, v in extra.items()}},
                                    vectors=tuple(extra))
            s.chain = ch
            chains.append(ch)
        self._pull_state(eng, 0)
        for kind in kinds:
            self.__dict__['_' + _lib.SUMS_KINDS[kind].result] = SUMS_RESULT[kind].from_engine(eng)
        if ppc:
            self.__dict__['_ppc'] = PredictiveCheck.from_problem(self._problem, ppc_rows)
        if spatial_check:
            self.__dict__['_spatial_check'] = SpatialCheck.from_problem(self._problem, moran_rows)
        if site_intervals:
            self.__dict__['_site_intervals'] = SiteIntervals.from_engine(eng)
        if site_diagnostics:
            self.__dict__['_site_diagnostics'] = SiteDiagnostics.from_engine(eng)
        if holdout is not None:
            self.__dict__['_holdout'] = HoldoutScore.from_engine(eng)
        return chains


class LogitRSRGibbs(LogitICARGibbs):
    r"""Gibbs sampler, logit link, reduced-rank (RSR) spatial random effects -- computed on an AMD MI355X.

    Drop-in for the reference class of the same name (``logit.py:340-485``): ``LogitRSRGibbs(Q, W, X, y,
    hparams=None, random_state=None, r=0.5, q=None)``.  The spatial effects are :math:`K\theta` with
    :math:`K` the eigenvectors of the Moran operator whose eigenvalues are at least ``r`` (or the ``q`` leading
    ones); ``state.eta`` holds :math:`\theta`, ``state.spatial`` holds :math:`K\theta`, ``fixed.Q`` is
    :math:`K^\top Q K`, ``fixed.K`` is :math:`K`, ``fixed.q`` its number of columns, and the default
    ``tau_shape`` becomes ``0.5 + 0.5 q`` -- all as in the reference.  The basis is computed on the host with dense
    n x n linear algebra, once (as the reference does); per iteration the device forms
    :math:`K^\top\Omega K + \tau K^\top QK` and solves the q x q system (``csrc/occ_rsr.hpp``: in LDS and registers up to
    128 basis columns, panel by panel in device memory up to 4096 -- the reference's default threshold keeps about 13 % of a
    lattice's sites: 1 280 columns at 100x100).  ``device`` selects the HIP device.  ``basis='device'`` builds the basis on
    that device too, without any n x n array (``occuspytial_amd.basis.moran_basis``): the same span, columns defined up to sign
    and up to a rotation inside a cluster of near-equal eigenvalues; any value but ``'host'`` and ``'device'`` is refused.
    """

    def __init__(self, Q, W, X, y, hparams=None, random_state=None, r=0.5, q=None, device=0, devices=None, basis='host'):
        if basis not in ('host', 'device'):
            raise ValueError("basis must be 'host' or 'device'")
        super().__init__(Q, W, X, y, hparams, random_state, device=device, devices=devices, prior_draw='edge')
        self._configure_rsr(r, q, hparams, basis)

    def _configure_rsr(self, r, q, hparams, basis='host'):
        rsr = self._problem.enable_rsr(r=r, q=q, default_tau_shape=not hparams, basis=basis, device=self.device)
        if rsr['dim'] > 4096:
            raise ValueError(f'{rsr["dim"]} basis columns selected; the device path supports at most 4096 '
                             '(raise the threshold `r` or pass `q`)')
        fixed = self.fixed
        fixed.q = rsr['dim']
        del fixed.Q
        fixed.Q = rsr['Q']
        fixed.K = rsr['K']
        if not hparams:
            del fixed.tau_shape
            fixed.tau_shape = self._problem.tau_shape

    def _initialize_default_start(self, state):
        state = super()._initialize_default_start(state)
        state.eta = self.rng.normal(scale=5, size=self.fixed.q)           # logit.py:453-455
        state.spatial = self.fixed.K @ state.eta
        return state

    def _initialize_posterior_state(self, start=None):
        if start is None:
            self._initialize_default_start(self.state)
        else:
            self.state.alpha = start['alpha']
            self.state.beta = start['beta']
            self.state.tau = start['tau']
            self.state.eta = start['eta']
            self.state.spatial = self.fixed.K @ np.asarray(self.state.eta, dtype=float)
