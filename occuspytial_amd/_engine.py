"""Thin object wrapper over the C ABI: one ``Engine`` = one device-resident batch of chains."""
import atexit
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._native import ptr as _ptr


def _keys_array(keys):
    return (C.c_uint64 * len(keys))(*[int(v) & (2 ** 64 - 1) for v in keys])


def problem_struct(prob):
    """``occ_problem`` of a :class:`FlatProblem` plus the arrays that must outlive the call."""
    Q = prob.Q
    k = dict(
        indptr=np.ascontiguousarray(Q.indptr, dtype=np.int32),
        indices=np.ascontiguousarray(Q.indices, dtype=np.int32),
        data=np.ascontiguousarray(Q.data, dtype=np.float64),
        site_id=np.ascontiguousarray(prob.site_id, dtype=np.int32),
        site_ptr=np.ascontiguousarray(prob.site_ptr, dtype=np.int32),
    )
    pb = _lib.OccProblem(
        n=prob.n, n_surveyed=prob.S, n_rows=prob.R, p=prob.p, q=prob.q,
        q_indptr=_ptr(k['indptr']), q_indices=_ptr(k['indices']), q_data=_ptr(k['data']),
        X=_ptr(prob.X), site_id=_ptr(k['site_id']), site_ptr=_ptr(k['site_ptr']),
        W=_ptr(prob.W), y=_ptr(prob.y), a_mu=_ptr(prob.a_mu), a_prec=_ptr(prob.a_prec),
        b_mu=_ptr(prob.b_mu), b_prec=_ptr(prob.b_prec), tau_rate=prob.tau_rate, tau_shape=prob.tau_shape)
    rsr = getattr(prob, 'rsr', None)
    if rsr is not None:   # LogitRSRGibbs: eta = K theta
        pb.rsr_dim = int(rsr['dim'])
        pb.rsr_K, pb.rsr_Q, pb.rsr_E = _ptr(rsr['K']), _ptr(rsr['Q']), _ptr(rsr['E'])
        probit = getattr(prob, 'probit', None)
        if probit is not None:   # ProbitRSRGibbs: the same basis, plus the eigenvectors of the factor-free theta update
            pb.link = 1
            pb.pb_Phi, pb.pb_G, pb.pb_lam = _ptr(probit['Phi']), _ptr(probit['G']), _ptr(probit['lam'])
    elif getattr(prob, 'prior_factor', None) is not None:   # the reference's form of the prior draw: u = E eps
        k['prior_factor'] = np.ascontiguousarray(prob.prior_factor, dtype=np.float64)
        pb.prior_factor = _ptr(k['prior_factor'])
        pb.prior_factor_cols = k['prior_factor'].shape[1]
    return pb, k


class ProblemMeta:
    """Sizes and hyper-parameters of a problem -- all a rank of a distributed group needs on the HOST when the design
    arrays themselves arrive on its device by broadcast (start values, output shapes)."""

    FIELDS = ('n', 'p', 'q', 'S', 'R', 'tau_rate', 'tau_shape', 'a_mu', 'a_prec', 'b_mu', 'b_prec')
    OPTIONAL = ('constraint', 'n_components', 'component_labels')   # absent: the global constraint
    rsr = None
    constraint, n_components, component_labels = 'global', 1, None

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])
        for f in self.OPTIONAL:
            if f in kw:
                setattr(self, f, kw[f])

    @classmethod
    def of(cls, prob):
        return cls(**{f: getattr(prob, f) for f in cls.FIELDS + cls.OPTIONAL if hasattr(prob, f)})

    def to_dict(self):
        d = {f: getattr(self, f) for f in self.FIELDS}
        if self.constraint != 'global':
            d.update({f: getattr(self, f) for f in self.OPTIONAL})
        return d


_LIVE = weakref.WeakSet()   # engines not yet closed: closed at interpreter exit, before the library's own exit hook runs


@atexit.register
def _close_live_engines():
    """An engine some object still holds when the interpreter exits (an uncollected sampler, an exception path) would keep its
    CU-masked streams alive into the HIP runtime's -- and a profiler's -- finalisers (a rocprofv3 crash seen in round 3)."""
    for eng in list(_LIVE):
        try:
            eng.close()
        except Exception:
            pass


class Engine:
    """Device-resident sampler state for ``n_chains`` chains of one :class:`FlatProblem`.

    ``keys`` are the 64-bit Philox keys of the chains.  ``device`` is the HIP device ordinal.
    """

    def __init__(self, prob, keys, device=0):
        lib = _lib.load()
        pb, keep = problem_struct(prob)
        karr = _keys_array(keys)
        h = C.c_void_p()
        code = lib.occ_create(C.byref(pb), len(keys), karr, int(device), C.byref(h))
        _lib.raise_for(code, None)
        self._adopt(lib, h, prob, keys, device)
        del keep
        if self.probit is not None:
            # a library that does not know the probit model (an older build, or the CPU oracle's C ABI, which ignores
            # `link`) would run the logit model on this problem without a word: it must say that it runs the probit one
            ln = C.c_int64(0)
            out = np.zeros(1)
            code = lib.occ_get_state(h, 0, b'link', _ptr(out), 1, C.byref(ln))
            if code != _lib.OCC_OK or ln.value != 1 or out[0] != 1.0:
                self.close()
                raise _lib.EngineUnavailable(f'{_lib.LIB_PATH} does not implement the probit model')

    def _adopt(self, lib, handle, prob, keys, device):
        self._h = handle
        self._lib = lib
        self.prob = prob
        self.rsr = getattr(prob, 'rsr', None)
        self.probit = getattr(prob, 'probit', None)
        self.n_chains = len(keys)
        self.device = int(device)
        self.keys = [int(v) & (2 ** 64 - 1) for v in keys]
        # kind of per-site sums (_lib.SUMS_KINDS) -> switched on (sums_switch); off: no call about them reaches the library
        self._sums_on = dict.fromkeys(_lib.SUMS_KINDS, False)
        # the draws of a call (_lib.DRAWS_KINDS): each kind's switch, and the regions' map (None: never set); until a switch or
        # the map is first set, no call about the kind reaches the library
        self._regions = None
        for k in _lib.DRAWS_KINDS.values():
            setattr(self, k.on, False)
        # per-site intervals: the number of bins while switched on, 0 while off; until it is first set, no call about them
        # reaches the library
        self._hist_bins = 0
        # per-site convergence diagnostics: the batch length while switched on, 0 while off; likewise
        self._conv_batch = 0
        self._conv_last = 0   # (the batch length of the sums that stay readable after switching off)
        # held-out predictive scoring: the withheld data as packed for the library (None: never set) and the switch; until the
        # data are set, no call about it reaches the library
        self._holdout = None
        self._holdout_on = False
        _LIVE.add(self)
        # constraint='component' on a graph of more than one connected component: the handle gets the labels before its first
        # iteration (with one component, or under 'global', no call about them reaches the library)
        if getattr(prob, 'constraint', 'global') == 'component' and getattr(prob, 'n_components', 1) > 1:
            try:
                self.set('component_id', np.asarray(prob.component_labels, dtype=np.float64), 0)
            except Exception as exc:
                self.close()   # (whatever the refusal: no half-made engine is left open)
                if isinstance(exc, ValueError) and 'unknown state name' in str(exc):
                    # a stale build, or a stand-in library that does not know the state name
                    raise ValueError(f"the loaded engine library has no constraint='component' ({exc}): rebuild it") from None
                raise   # (a library that knows the name and refuses: its own words, e.g. for a reduced-rank problem)
        return self

    @classmethod
    def group(cls, prob, keys_per_device, devices):
        """One engine per entry of ``devices`` (``occ_create_group``): the problem is laid out once, uploaded to
        ``devices[0]`` and broadcast to the others device-to-device (RCCL).  ``keys_per_device[g]`` are the Philox keys
        of the chains that live on ``devices[g]``.  Each engine is then driven by its own host thread."""
        lib = _lib.load()
        pb, keep = problem_struct(prob)
        G = len(devices)
        if G < 1 or len(keys_per_device) != G or any(len(k) < 1 for k in keys_per_device):
            raise ValueError('every device of a group needs at least one chain')
        dev = (C.c_int32 * G)(*[int(d) for d in devices])
        cnt = (C.c_int32 * G)(*[len(k) for k in keys_per_device])
        karr = _keys_array([k for ks in keys_per_device for k in ks])
        hs = (C.c_void_p * G)()
        code = lib.occ_create_group(C.byref(pb), G, dev, cnt, karr, hs)
        _lib.raise_for(code, None)
        del keep
        engines = []
        try:
            for g in range(G):
                engines.append(cls.__new__(cls)._adopt(lib, C.c_void_p(hs[g]), prob, keys_per_device[g], devices[g]))
        except Exception:   # (a handle refused the problem's mode: none of the group's handles stays open)
            for e in engines:
                e.close()
            for g in range(len(engines) + 1, G):
                lib.occ_destroy(C.c_void_p(hs[g]))
            raise
        return engines

    @classmethod
    def distributed(cls, prob, comm, keys, root=0):
        """This process's engine of a one-process-per-GPU group (``occ_create_distributed``): ``prob`` is the full
        :class:`FlatProblem` on rank ``root`` and a :class:`ProblemMeta` (sizes and hyper-parameters only) elsewhere;
        the design arrays reach the other ranks' devices by RCCL broadcast, never their hosts.  ``comm``: an
        ``occuspytial_amd.distributed.RcclComm``."""
        lib = _lib.load()
        h = C.c_void_p()
        if comm.rank == root:
            pb, keep = problem_struct(prob)
            code = lib.occ_create_distributed(C.byref(pb), comm.handle, root, len(keys), _keys_array(keys), C.byref(h))
            del keep
        else:
            code = lib.occ_create_distributed(None, comm.handle, root, len(keys), _keys_array(keys), C.byref(h))
        _lib.raise_for(code, None)
        return cls.__new__(cls)._adopt(lib, h, prob, keys, comm.device)

    @property
    def transport(self):
        """How this engine's fixed arrays reached its device (``occ_group_transport``)."""
        return self._lib.occ_group_transport(self._h).decode()

    def synchronize(self):
        self._check(self._lib.occ_synchronize(self._h))

    def close(self):
        if getattr(self, '_h', None):
            self._lib.occ_destroy(self._h)
            self._h = None
            _LIVE.discard(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, code):
        _lib.raise_for(code, self._h)

    def set_keys(self, keys):
        if len(keys) != self.n_chains:
            raise ValueError('one key per chain is required')
        karr = (C.c_uint64 * self.n_chains)(*[int(v) & (2 ** 64 - 1) for v in keys])
        self._check(self._lib.occ_set_keys(self._h, karr))
        self.keys = [int(v) & (2 ** 64 - 1) for v in keys]

    # ---- checkpoint / resume (the reference has none) -------------------------------------
    @property
    def model(self):
        """This engine's bit of the masks of ``_lib.STATE_NAMES``."""
        return _lib.PROBIT if self.probit is not None else _lib.RSR if self.rsr is not None else _lib.ICAR

    def checkpoint(self):
        """Everything a chain needs to continue exactly where it is: the state the next iteration reads
        (alpha, beta, tau, eta, z, the MINRES warm start xz), its iteration number and its Philox key.
        Variates are functions of (key, iteration, index), so a restored chain reproduces the
        uninterrupted one bit for bit; omega_b and the noise of the coming iteration are recomputed."""
        out = {'n_chains': np.int64(self.n_chains), 'keys': np.array(self.keys, dtype=np.uint64),
               'iter': np.array([int(self.get('iter', c)) for c in range(self.n_chains)], dtype=np.int64),
               'shape': np.array([self.prob.n, self.prob.p, self.prob.q, self.prob.R], dtype=np.int64)}
        # (the probit model: also the engine's own coordinates c and the eta it computed from them, bit-exact continuation)
        for name in (nm for nm, st in _lib.STATE_NAMES.items() if st.ckpt & self.model):
            out[name] = np.stack([np.atleast_1d(self.get(name, c)) for c in range(self.n_chains)])
        for kind, on in self._sums_on.items():
            if on:   # switch, count and the kind's per-site sums: a resumed run ends with the sums of the uninterrupted one
                switch, *rest = _lib.SUMS_KINDS[kind].fields
                out[switch] = np.ones(self.n_chains)
                for name in rest:
                    out[name] = np.stack([np.atleast_1d(self.get(name, c)) for c in range(self.n_chains)])
        for k in _lib.DRAWS_KINDS.values():   # (the handle's input, one row per chain, as every entry,) and the switch; the draws belong to a call
            on = getattr(self, k.on)
            if k.input and self._regions is not None:
                out[k.input] = np.tile(self._regions, (self.n_chains, 1))
            if k.input in out or (on and not k.input):
                out[k.fields[-2]] = np.full(self.n_chains, float(on))
        for kind, k in _lib.ACCUM_KINDS.items():
            on = getattr(self, k.on)
            if on:   # (the handle's input, one row per chain, as every entry,) the switch's value, the counts and the data
                switch, count, data = k.fields[-3:]
                parts = [self._accum(kind, c) for c in range(self.n_chains)]
                if k.input:
                    out[k.input] = np.tile(self._holdout, (self.n_chains, 1))
                out[switch] = np.full(self.n_chains, float(on))
                out[count] = np.array([p[0] for p in parts], dtype=np.int64)
                out[data] = np.stack([p[1] for p in parts])
        return out

    def restore(self, ckpt):
        """Inverse of :meth:`checkpoint` (same problem, same number of chains)."""
        if int(ckpt['n_chains']) != self.n_chains:
            raise ValueError('checkpoint holds %d chains, this engine %d' % (int(ckpt['n_chains']), self.n_chains))
        if list(np.asarray(ckpt['shape'])) != [self.prob.n, self.prob.p, self.prob.q, self.prob.R]:
            raise ValueError('checkpoint belongs to a problem of different size')
        self.set_keys([int(k) for k in np.asarray(ckpt['keys'])])
        spatial = 'eta' if self.rsr is None else 'theta'   # reduced-rank model: the coefficients; eta = K theta follows
        for c in range(self.n_chains):
            self.set_start(c, ckpt['alpha'][c], ckpt['beta'][c], float(np.asarray(ckpt['tau'][c]).ravel()[0]), ckpt[spatial][c])
            self.set('z', ckpt['z'][c], c)
            if self.probit is not None:
                for name in ('c', 'eta', 'eps'):
                    self.set(name, ckpt[name][c], c)
            if self.rsr is None:
                self.set('xz', ckpt['xz'][c], c)
            self.set('iter', float(ckpt['iter'][c]), c)
        for kind, k in _lib.SUMS_KINDS.items():
            switch, *rest = k.fields
            if switch in ckpt and np.all(np.asarray(ckpt[switch]) != 0):
                self.sums_switch(kind, True)
                for c in range(self.n_chains):
                    for name in rest:
                        self.set(name, ckpt[name][c], c)
            elif self._sums_on[kind]:
                self.sums_switch(kind, False)
        for k in _lib.DRAWS_KINDS.values():   # (the methods bear the names of the switches)
            switch = k.fields[-2]
            on = switch in ckpt and bool(np.all(np.asarray(ckpt[switch]) != 0))
            if k.input in ckpt:   # (a kind with an input is switched as the checkpoint says, off too)
                self.regions(np.asarray(ckpt[k.input])[0])
            if k.input in ckpt or on or getattr(self, k.on):
                getattr(self, switch)(on)
        for k in _lib.ACCUM_KINDS.values():   # (the methods bear the names of the input and of the switch)
            switch, count, data = k.fields[-3:]
            if switch in ckpt and np.all(np.asarray(ckpt[switch]) != 0):
                if k.input:
                    getattr(self, k.input)(np.asarray(ckpt[k.input], dtype=np.float64)[0])
                getattr(self, switch)(int(np.asarray(ckpt[switch]).ravel()[0]))
                for c in range(self.n_chains):
                    self.set(count, float(np.asarray(ckpt[count])[c]), c)
                    self.set(data, np.asarray(ckpt[data], dtype=np.float64)[c].ravel(), c)
            elif getattr(self, k.on):
                getattr(self, switch)(0)

    def _accum(self, kind, chain):
        """``(iterations accumulated, the data in their shape and dtype)`` of one accumulator (``_lib.ACCUM_KINDS``) and chain."""
        k = _lib.ACCUM_KINDS[kind]
        shape = tuple(self.prob.n if d == 'n' else d for d in k.shape)
        return int(self.get(k.fields[-2], chain)[0]), self.get(k.fields[-1], chain).reshape(shape).astype(k.dtype, copy=False)

    # ---- held-out predictive scoring (state names holdout_*, include/occ_gibbs.h) ----
    def holdout_data(self, W, y=None):
        """Set the handle's withheld data: ``W`` and ``y`` dicts keyed by site, as the constructor takes them, of sites this
        engine's problem does NOT survey (or ``W`` the array :func:`occuspytial_amd.holdout.holdout_arg` packs and no
        ``y``).  The switches of all chains go off first (the library sets the data only then); setting them zeroes every
        chain's sums."""
        from .holdout import holdout_arg
        packed = holdout_arg((W, y), self.prob) if y is not None else np.ascontiguousarray(W, dtype=np.float64).ravel()
        if self._holdout_on:
            self.holdout_stats(False)
        self.set('holdout_data', packed, 0)
        self._holdout = packed.copy()

    def holdout_stats(self, on):
        """Switch the held-out sums of every chain on (which ZEROES them and their counts) or off (they stay readable).
        While on, every iteration past a call's burn-in adds, per held-out site, the predictive density of its withheld
        detection history under the iteration's alpha, beta and eta (:meth:`holdout_sums`)."""
        for c in range(self.n_chains):
            self.set('holdout_stats', 1.0 if on else 0.0, c)
        self._holdout_on = bool(on)

    def holdout_sums(self, chain=0):
        """``{'count': iterations accumulated, 'sums': (5, H) float64}`` of one chain: per held-out entry ``cnt``, the sum of
        the likelihood L, of l = log L, of l^2, and of pd, the predictive probability of at least one detection."""
        count, sums = self._accum('holdout', chain)
        return {'count': count, 'sums': sums}

    # ---- per-site convergence diagnostics (state names conv_*, include/occ_gibbs.h) ----
    def conv_stats(self, batch):
        """Switch the per-site batch-means sums of every chain: ``batch`` from 1 to 2^30 is on with that batch length (which
        ZEROES them and their counts), 0 or False is off (they stay readable).  While on, every iteration past a call's
        burn-in updates the sums of psi and of eta at every site (:meth:`conv_sums`).  The batch length belongs to the
        handle: for another one every chain is switched off first."""
        batch = int(batch)
        if batch and self._conv_batch and batch != self._conv_batch:
            self.conv_stats(0)
        for c in range(self.n_chains):
            self.set('conv_stats', float(batch), c)
        self._conv_batch = batch
        self._conv_last = batch or self._conv_last

    def conv_sums(self, chain=0):
        """``{'batch': L, 'count': iterations accumulated, 'sums': (11, n) float64}`` of one chain: per site ``cnt``, then
        ``ref, s1, s2, run, bsq`` of psi, then the same five of eta."""
        batch = self._conv_batch or self._conv_last   # (neither is set when the switch was set by name: ask the handle)
        batch = batch or int(max(self.get('conv_stats', c)[0] for c in range(self.n_chains)))
        count, sums = self._accum('conv', chain)
        return {'batch': batch, 'count': count, 'sums': sums}

    # ---- per-site intervals (state names hist_*, include/occ_gibbs.h) ----
    def hist_stats(self, bins):
        """Switch the per-site histograms of every chain: ``bins`` from 4 to 1024 is on with that many equal bins on (0, 1)
        (which ZEROES them and their counts), 0 or False is off (they stay readable).  While on, every iteration past a
        call's burn-in adds one count per site, in the bin of the iteration's psi (:meth:`hist_counts`).  The number of bins
        belongs to the handle: for another one every chain is switched off first."""
        bins = 64 if bins is True else bins
        if bins and self._hist_bins and bins != self._hist_bins:
            self.hist_stats(0)
        for c in range(self.n_chains):
            self.set('hist_stats', float(bins), c)
        self._hist_bins = int(bins)

    def hist_counts(self, chain=0):
        """``{'bins': B, 'count': iterations accumulated, 'counts': (B, n) uint32}`` of one chain."""
        count, counts = self._accum('hist', chain)
        return {'bins': counts.shape[0], 'count': count, 'counts': counts}

    # ---- the draws of a call (state names moran_*, ppc_* and region_*, include/occ_gibbs.h), by kind (_lib.DRAWS_KINDS) ----
    def _draws_switch(self, kind, on):
        k = _lib.DRAWS_KINDS[kind]
        for c in range(self.n_chains):
            self.set(k.fields[-2], 1.0 if on else 0.0, c)
        setattr(self, k.on, bool(on))

    def _draws_rows(self, kind, chain):
        k = _lib.DRAWS_KINDS[kind]
        width = k.width or (max(int(self._regions.max()) + 1, 1) if self._regions is not None else 1)
        return self.get(k.fields[-1], chain).reshape(-1, width)

    def moran_stats(self, on):
        """Switch the spatial residual check of every chain.  While on, every kept draw of ``run`` records the sums of
        Moran's I of the occupancy residuals z - psi and of one replicate of them (:meth:`moran_draws`)."""
        self._draws_switch('moran', on)

    def moran_draws(self, chain=0):
        """``(keep, 8)`` rows of one chain from the last ``run`` -- A, B, C, D of the residuals, then of their replicate
        (``occuspytial_amd.spatial``) -- ``(0, 8)`` if its switch was off during that call."""
        return self._draws_rows('moran', chain)

    def ppc_stats(self, on):
        """Switch the posterior predictive check of every chain.  While on, every kept draw of ``run`` replicates the
        detections of every surveyed site from the draw's z and alpha and records four sums (:meth:`ppc_draws`)."""
        self._draws_switch('ppc', on)

    def ppc_draws(self, chain=0):
        """``(keep, 4)`` rows of one chain from the last ``run`` -- the Freeman-Tukey discrepancy of the observed and of the
        replicated detections, the replicated detections, the replicated sites with a detection -- ``(0, 4)`` if its
        switch was off during that call."""
        return self._draws_rows('ppc', chain)

    def regions(self, ids):
        """Set the handle's map: the region of every site, whole numbers in [-1, 256), -1 for none.  The switches of all
        chains go off first (the library sets a map only then)."""
        ids = np.asarray(ids, dtype=np.int64).ravel()
        if self._region_on:
            self.region_stats(False)
        self.set('region_id', ids.astype(np.float64), 0)
        self._regions = ids.copy()

    def region_stats(self, on):
        """Switch the count of occupied sites per region of every chain.  While on, every kept draw of ``run`` records, per
        region, the number of its sites with z = 1 (:meth:`region_draws`)."""
        self._draws_switch('region', on)

    def region_draws(self, chain=0):
        """``(keep, G)`` counts of one chain from the last ``run``; ``(0, G)`` if its switch was off during that call."""
        return self._draws_rows('region', chain)

    # ---- per-site sums accumulated on the device (state names site_* and ll_*, include/occ_gibbs.h), by kind ----
    def sums_switch(self, kind, on):
        """Switch one kind of per-site sums of every chain on (which ZEROES them and their counts) or off (they stay
        readable).  The kinds are independent of each other."""
        for c in range(self.n_chains):
            self.set(_lib.SUMS_KINDS[kind].fields[0], 1.0 if on else 0.0, c)
        self._sums_on[kind] = bool(on)

    def sums(self, kind, chain=0):
        """``{'count': iterations accumulated, short name: sum (n), ...}`` of one kind and one chain."""
        _, count, *names = _lib.SUMS_KINDS[kind].fields
        out = {'count': int(self.get(count, chain)[0])}
        for name in names:
            out[name[len(kind) + 1:]] = self.get(name, chain)
        return out

    def site_stats(self, on):
        """Switch the per-site posterior sums (:meth:`sums_switch`).  While on, the z update of every kept iteration adds
        psi, P(z = 1 | rest), z, eta and eta^2 of every site."""
        self.sums_switch('site', on)

    def site_sums(self, chain=0):
        """``{'count', 'psi', 'occ', 'z', 'eta', 'eta2'}`` of one chain: the iterations accumulated and the five sums (n)."""
        return self.sums('site', chain)

    def loglik_stats(self, on):
        """Switch the log-likelihood sums of streaming WAIC (:meth:`sums_switch`).  While on, the z update of every kept
        iteration adds, at every surveyed site, the site's marginal likelihood L (z integrated out), log L and (log L)^2."""
        self.sums_switch('ll', on)

    def loglik_sums(self, chain=0):
        """``{'count', 'lik', 'log', 'log2'}`` of one chain: the iterations accumulated and the three sums (n; exactly 0
        at a site that was not surveyed)."""
        return self.sums('ll', chain)

    def set_start(self, chain, alpha, beta, tau, eta):
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        b = np.ascontiguousarray(beta, dtype=np.float64)
        e = np.ascontiguousarray(eta, dtype=np.float64)
        n_eta = self.prob.n if self.rsr is None else int(self.rsr['dim'])   # reduced-rank model: eta is theta
        if a.shape != (self.prob.q,) or b.shape != (self.prob.p,) or e.shape != (n_eta,):
            raise ValueError('start values have the wrong shape')
        self._check(self._lib.occ_set_start(self._h, chain, _ptr(a), _ptr(b), float(tau), _ptr(e)))

    def step(self):
        self._check(self._lib.occ_step(self._h))

    def run(self, n_iter, burnin=0):
        keep = n_iter - burnin
        C_ = self.n_chains
        a = np.zeros((C_, max(keep, 0), self.prob.q))
        b = np.zeros((C_, max(keep, 0), self.prob.p))
        t = np.zeros((C_, max(keep, 0)))
        self._check(self._lib.occ_run(self._h, n_iter, burnin, _ptr(a), _ptr(b), _ptr(t)))
        return a, b, t

    def get(self, name, chain=0):
        ln = C.c_int64(0)
        self._check(self._lib.occ_get_state(self._h, chain, name.encode(), None, 0, C.byref(ln)))
        out = np.empty(ln.value)
        self._check(self._lib.occ_get_state(self._h, chain, name.encode(), _ptr(out), out.size, C.byref(ln)))
        return out[0] if name in ('tau', 'minres_itn', 'iter') else out

    def set(self, name, value, chain=0):
        v = np.ascontiguousarray(np.atleast_1d(value), dtype=np.float64)
        self._check(self._lib.occ_set_state(self._h, chain, name.encode(), _ptr(v), v.size))

    # ---- per-conditional updates with injected variates (C ABI occ_cond_*; parity tests against the reference's fixtures)
    @staticmethod
    def _vec(a, size):
        v = np.ascontiguousarray(a, dtype=np.float64).ravel()
        if v.size != size:
            raise ValueError('wrong length: %d, expected %d' % (v.size, size))
        return v

    def cond_tau(self, gamma_variate, chain=0):
        out = C.c_double(0.0)
        self._check(self._lib.occ_cond_tau(self._h, chain, float(gamma_variate), C.byref(out)))
        return out.value

    def cond_eta(self, omega_b, eps_site, prior_term, chain=0):
        """-> (rhs, xz, eta, minres iterations) from the chain's beta, z, tau and warm start."""
        n = self.prob.n
        ob, e1, pt = self._vec(omega_b, n), self._vec(eps_site, n), self._vec(prior_term, n)
        rhs, xz, eta, itn = np.empty(n), np.empty(2 * n), np.empty(n), C.c_int32(0)
        self._check(self._lib.occ_cond_eta(self._h, chain, _ptr(ob), _ptr(e1), _ptr(pt), _ptr(rhs), _ptr(xz), _ptr(eta), C.byref(itn)))
        return rhs, xz, eta, itn.value

    def cond_beta(self, omega_b, eps, chain=0):
        ob, ep, out = self._vec(omega_b, self.prob.n), self._vec(eps, self.prob.p), np.empty(self.prob.p)
        self._check(self._lib.occ_cond_beta(self._h, chain, _ptr(ob), _ptr(ep), _ptr(out)))
        return out

    def cond_alpha(self, omega_a, eps, chain=0):
        oa, ep, out = self._vec(omega_a, self.prob.R), self._vec(eps, self.prob.q), np.empty(self.prob.q)
        self._check(self._lib.occ_cond_alpha(self._h, chain, _ptr(oa), _ptr(ep), _ptr(out)))
        return out

    def cond_z(self, u, chain=0):
        uu, out = self._vec(u, self.prob.n), np.empty(self.prob.n)
        self._check(self._lib.occ_cond_z(self._h, chain, _ptr(uu), _ptr(out)))
        return out

    def stats(self):
        st = _lib.OccStats()
        self._check(self._lib.occ_get_stats(self._h, C.byref(st)))
        return {f: getattr(st, f) for f, _ in st._fields_}

    def profile(self, reps=200):
        """Average in-graph launch time per kernel kind (leaves the chains mid-solve: re-start them)."""
        counts = (C.c_int64 * _lib.N_KERNEL_KINDS)()
        total = (C.c_double * _lib.N_KERNEL_KINDS)()
        self._check(self._lib.occ_profile(self._h, reps, counts, total))
        return {k: {'launches': int(counts[i]), 'total_us': float(total[i]),
                    'avg_us': float(total[i]) / counts[i] if counts[i] else 0.0}
                for i, k in enumerate(_lib.KERNEL_KINDS)}


DRAW_KINDS = {'pg1': 0, 'std_gamma': 1, 'normal': 2, 'uniform': 3, 'wave_sum_check': 4, 'truncnorm_pos': 5, 'truncnorm_neg': 6}


def device_draw(kind, param=None, n=None, key=1, it=0, stream=1, device=0):
    """Variates of the engine's own generators drawn on the device (``occ_draw``): element ``i`` comes from the
    sub-stream ``(key, i, it, stream)`` exactly as the kernels draw it.  ``kind``: ``'pg1'`` (``param`` = z),
    ``'std_gamma'`` (``param`` = shape), ``'normal'``, ``'uniform'`` (``n`` draws), ``'truncnorm_pos'`` / ``'truncnorm_neg'``
    (``param`` = loc: N(loc, 1) truncated to (0, inf) / (-inf, 0) at the uniform of ``'uniform'``); ``'wave_sum_check'``: a device self-test
    (tests/test_gpu_rng.py), NaN where the forms of the engine's wave sum disagree."""
    lib = _lib.load()
    par = None
    if kind in ('pg1', 'std_gamma', 'wave_sum_check', 'truncnorm_pos', 'truncnorm_neg'):
        par = np.ascontiguousarray(param, dtype=np.float64).ravel()
        n = par.size
    out = np.empty(int(n))
    code = lib.occ_draw(int(device), DRAW_KINDS[kind], int(key) & (2 ** 64 - 1), int(it), int(stream), int(n),
                        _ptr(par) if par is not None else None, _ptr(out))
    _lib.raise_for(code, None)
    return out


class EngineGroup:
    """Several :class:`Engine` s -- one per GPU of this process -- behind the interface of one: chain ``c`` lives on
    ``devices[c % G]`` (the reference's ``gibbs/parallel.py:20-41`` gives every chain a process of its
    own).  The problem is uploaded once and broadcast device to device (``Engine.group``); ``run`` drives every device
    from its own host thread (the C ABI holds no global state and ctypes releases the GIL)."""

    def __init__(self, prob, keys, devices, engine_factory=None):
        devices = [int(d) for d in devices]
        G = min(len(devices), len(keys))
        self.devices = devices[:G]
        self.prob = prob
        self.rsr = getattr(prob, 'rsr', None)
        self.n_chains = len(keys)
        self.where = [(c % G, c // G) for c in range(self.n_chains)]        # chain -> (engine, local index)
        per_dev = [[keys[c] for c in range(self.n_chains) if c % G == g] for g in range(G)]
        if engine_factory is None:
            self.engines = Engine.group(prob, per_dev, self.devices)
        else:   # tests: any object with the Engine interface
            self.engines = [engine_factory(prob, per_dev[g], self.devices[g]) for g in range(G)]
        self.keys = [int(k) & (2 ** 64 - 1) for k in keys]
        self.device = self.devices[0]

    @property
    def transport(self):
        return getattr(self.engines[0], 'transport', 'n/a')

    def _each(self, fn):
        """``fn(engine)`` on every engine, one host thread per engine; results in engine order."""
        if len(self.engines) == 1:
            return [fn(self.engines[0])]
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=len(self.engines)) as pool:
            return list(pool.map(fn, self.engines))

    def close(self):
        for e in self.engines:
            e.close()

    def set_keys(self, keys):
        if len(keys) != self.n_chains:
            raise ValueError('one key per chain is required')
        G = len(self.engines)
        for g, e in enumerate(self.engines):
            e.set_keys([keys[c] for c in range(self.n_chains) if c % G == g])
        self.keys = [int(k) & (2 ** 64 - 1) for k in keys]

    def set_start(self, chain, alpha, beta, tau, eta):
        g, i = self.where[chain]
        self.engines[g].set_start(i, alpha, beta, tau, eta)

    def get(self, name, chain=0):
        g, i = self.where[chain]
        return self.engines[g].get(name, i)

    def set(self, name, value, chain=0):
        g, i = self.where[chain]
        self.engines[g].set(name, value, i)

    @property
    def _sums_on(self):   # (a stand-in engine of the tests need not know the sums: it has none switched on)
        return {kind: any(getattr(e, '_sums_on', {}).get(kind, False) for e in self.engines) for kind in _lib.SUMS_KINDS}

    # What every feature of Engine needs of a group -- the sums, the regions, ppc, moran, hist, conv, holdout: its switches and
    # inputs are set on every engine, its results are read from the engine of the chain (the last argument, 0 if left out,
    # after `lead` others), and what Engine remembers of it is any engine's, the largest, or the first engine's.  A stand-in
    # engine of the tests need not know a feature: it has it switched off.
    _DRAWS = tuple(_lib.DRAWS_KINDS.values())   # (their methods bear the names of the switch and of the rows)
    ON_EVERY = ('sums_switch', 'regions') + tuple(k.fields[-2] for k in _DRAWS) + ('hist_stats', 'conv_stats', 'holdout_data', 'holdout_stats')
    BY_CHAIN = {'sums': 1, **{k.fields[-1]: 0 for k in _DRAWS}, 'hist_counts': 0, 'conv_sums': 0, 'holdout_sums': 0}
    REMEMBERED = {'_regions': None, **{k.on: any for k in _DRAWS}, '_hist_bins': max, '_conv_batch': max, '_holdout': None, '_holdout_on': any}

    # (the entry points by name are Engine's own: each only names its kind)
    site_stats, site_sums, loglik_stats, loglik_sums = Engine.site_stats, Engine.site_sums, Engine.loglik_stats, Engine.loglik_sums

    def step(self):
        self._each(lambda e: e.step())

    def synchronize(self):
        for e in self.engines:
            e.synchronize()

    def run(self, n_iter, burnin=0):
        parts = self._each(lambda e: e.run(n_iter, burnin))
        keep = max(n_iter - burnin, 0)
        a = np.zeros((self.n_chains, keep, self.prob.q))
        b = np.zeros((self.n_chains, keep, self.prob.p))
        t = np.zeros((self.n_chains, keep))
        for c, (g, i) in enumerate(self.where):
            a[c], b[c], t[c] = parts[g][0][i], parts[g][1][i], parts[g][2][i]
        return a, b, t

    def stats(self):
        per = [e.stats() for e in self.engines]
        out = dict(per[0])
        out['n_chains'] = self.n_chains
        out['devices'] = list(self.devices)
        out['per_device'] = per
        return out

    def checkpoint(self):
        parts = [e.checkpoint() for e in self.engines]
        out = {'n_chains': np.int64(self.n_chains), 'shape': parts[0]['shape']}
        for name in parts[0]:
            if name in ('n_chains', 'shape'):
                continue
            out[name] = np.stack([np.asarray(parts[g][name])[i] for g, i in self.where])
        return out

    def restore(self, ckpt):
        if int(ckpt['n_chains']) != self.n_chains:
            raise ValueError('checkpoint holds %d chains, this engine %d' % (int(ckpt['n_chains']), self.n_chains))
        G = len(self.engines)
        for g, e in enumerate(self.engines):
            idx = [c for c in range(self.n_chains) if c % G == g]
            part = {k: (np.asarray(v)[idx] if k not in ('n_chains', 'shape') else v) for k, v in ckpt.items()}
            part['n_chains'] = np.int64(len(idx))
            e.restore(part)
        self.keys = [int(k) for k in np.asarray(ckpt['keys'])]


def _on_every(name):
    def call(self, *args, **kw):
        for e in self.engines:
            getattr(e, name)(*args, **kw)
    return call


def _by_chain(name, lead):
    def call(self, *args, chain=0):
        g, i = self.where[args[lead] if len(args) > lead else chain]
        return getattr(self.engines[g], name)(*args[:lead], i)
    return call


def _remembered(name, rule):
    if rule is None:
        return property(lambda self: getattr(self.engines[0], name, None))
    return property(lambda self: rule(getattr(e, name, 0) for e in self.engines))


for _name in EngineGroup.ON_EVERY:
    setattr(EngineGroup, _name, _on_every(_name))
for _name, _lead in EngineGroup.BY_CHAIN.items():
    setattr(EngineGroup, _name, _by_chain(_name, _lead))
for _name, _rule in EngineGroup.REMEMBERED.items():
    setattr(EngineGroup, _name, _remembered(_name, _rule))
