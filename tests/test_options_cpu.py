"""The optional outputs of ``sample`` and ``resume`` as one table (``occuspytial_amd/gibbs/options.py``), without a library:
the table against the code it describes, every call one stand-in engine that knows all eight options receives -- in order, with
its arguments, as literals recorded from the hand-threaded samplers this table replaced -- and the order of the refusals."""
import inspect

import numpy as np
import pytest

from .conftest import load_golden
from .test_api_cpu import _inputs
from .test_holdout_cpu import withheld

KEYWORDS = ('site_summaries', 'waic', 'regions', 'ppc', 'spatial_check', 'site_intervals', 'site_diagnostics', 'holdout')


@pytest.fixture(scope='module')
def small():
    return _inputs(load_golden('ref_queen150_ragged'))[:4]   # 150 sites, 100 surveyed, p = 3, q = 2


# ---- the table against the code ---------------------------------------------------------------------------------------
def test_rows_are_the_keywords_of_sample_and_resume_in_their_order():
    from occuspytial_amd.gibbs.base import GibbsBase
    from occuspytial_amd.gibbs.logit import LogitICARGibbs
    from occuspytial_amd.gibbs.options import OPTIONS
    from occuspytial_amd.gibbs.probit import ProbitRSRGibbs
    assert tuple(o.keyword for o in OPTIONS) == KEYWORDS
    for fn in (GibbsBase.sample, LogitICARGibbs.resume, ProbitRSRGibbs.resume):
        params = inspect.signature(fn).parameters
        assert tuple(name for name in params if name in KEYWORDS) == KEYWORDS          # the rows' order is the parameters'
        assert list(params)[-len(KEYWORDS):] == list(KEYWORDS)
        for o in OPTIONS:
            assert params[o.keyword].default is o.default and o.default in (False, None)
            assert ('``%s' % o.keyword) in fn.__doc__                                   # every option keeps its paragraph


def test_rows_name_what_exists():
    from occuspytial_amd._engine import Engine, EngineGroup
    from occuspytial_amd.gibbs.options import OPTIONS
    from occuspytial_amd.posterior import PosteriorParameter
    results = [o.result for o in OPTIONS]
    assert results == ['sites', 'waic', 'regions', 'ppc', 'spatial_check', 'site_intervals', 'site_diagnostics', 'holdout']
    for o in OPTIONS:
        assert o.result in vars(PosteriorParameter) and getattr(PosteriorParameter, o.result) is None
        assert o.methods and o.switch in o.methods
        for name in o.methods:
            assert callable(getattr(Engine, name)), name
            assert callable(getattr(EngineGroup, name)), name
    named = {name for o in OPTIONS for name in o.methods}
    assert set(EngineGroup.ON_EVERY) <= named                 # every switch and input the group sends everywhere has a row
    assert {'region_draws', 'ppc_draws', 'moran_draws'} <= named <= set(EngineGroup.ON_EVERY) | set(EngineGroup.BY_CHAIN)
    remembered = [o.left_on for o in OPTIONS]
    assert remembered == ['_sums_on', '_sums_on', '_region_on', '_ppc_on', '_moran_on', '_hist_bins', '_conv_batch', '_holdout_on']
    assert set(remembered[2:]) <= set(EngineGroup.REMEMBERED)


def test_rows_state_their_texts_and_their_rules():
    from occuspytial_amd.gibbs.options import OPTIONS
    for o in OPTIONS:
        assert o.python_step.startswith('steps in Python: ') and o.python_step.endswith('the device engine only')
        assert o.rebuild.startswith(('has no ', 'does not '))
        assert (o.probit is None) == (o.keyword == 'regions')
        assert o.probit is None or o.probit.endswith('not available for the probit model')
    by = {o.keyword: o for o in OPTIONS}
    assert [o.keyword for o in OPTIONS if o.parsed == 'first'] == ['site_intervals', 'site_diagnostics']
    assert [o.keyword for o in OPTIONS if o.parsed == 'after the refusal'] == ['holdout']
    assert [o.keyword for o in OPTIONS if o.input] == ['regions', 'holdout']
    assert (by['regions'].input, by['holdout'].input) == ('regions', 'holdout_data')
    # resume, not asked: the sums and regions stay as the checkpoint set them, the other five go off
    assert [o.keyword for o in OPTIONS if o.resume_leaves] == ['site_summaries', 'waic', 'regions']
    assert by['regions'].vector == 'occupied' and [o.vector for o in OPTIONS if o is not by['regions']] == [None] * 7


# ---- one stand-in engine that knows all eight options ------------------------------------------------------------------
class StandIn:
    """An object with the Engine interface that logs every call with its arguments.  Accumulators count the iterations a
    ``run`` keeps while their switch is on (switching on zeroes); the rows of a call hold the number of the iteration."""

    def __init__(self, prob, n_chains, restored=None):
        self.prob, self.n_chains = prob, n_chains
        self._sums_on = {'site': False, 'll': False}
        self._regions, self._region_on = None, False
        self._ppc_on = self._moran_on = False
        self._hist_bins = self._conv_batch = 0
        self._holdout, self._holdout_on = None, False
        self.restored = restored or {}
        self.count = dict.fromkeys(('site', 'll', 'hist', 'conv', 'holdout'), 0)
        self.log, self.t, self._last = [], 0, (0, 0)

    def set_start(self, chain, alpha, beta, tau, eta):
        self.log.append(('set_start', chain))

    def set(self, name, value, chain=0):
        self.log.append(('set', name, chain))

    def get(self, name, chain=0):
        self.log.append(('get', name, chain))
        p = self.prob
        sizes = dict(alpha=p.q, beta=p.p, eta=p.n, z=p.n, omega_b=p.n, omega_a=p.R)
        if name == 'tau':
            return 1.0
        if name == 'exists':
            return np.ones(p.S)
        return np.ones(sizes[name])

    def restore(self, ckpt):
        self.log.append(('restore', sorted(ckpt)))
        for name, value in self.restored.items():
            setattr(self, name, value.copy() if hasattr(value, 'copy') else value)

    def sums_switch(self, kind, on):
        self.log.append(('sums_switch', kind, on))
        self._sums_on[kind] = bool(on)
        if on:
            self.count[kind] = 0

    def sums(self, kind, chain=0):
        self.log.append(('sums', kind, chain))
        names = {'site': ('psi', 'occ', 'z', 'eta', 'eta2'), 'll': ('lik', 'log', 'log2')}[kind]
        return {'count': self.count[kind], **{name: np.full(self.prob.n, float(self.count[kind])) for name in names}}

    def site_sums(self, chain=0):
        return self.sums('site', chain)

    def loglik_sums(self, chain=0):
        return self.sums('ll', chain)

    def regions(self, ids):
        self.log.append(('regions', int(np.max(ids)) + 1))
        self._regions, self._region_on = np.asarray(ids).copy(), False

    def region_stats(self, on):
        self.log.append(('region_stats', on))
        self._region_on = bool(on)

    def ppc_stats(self, on):
        self.log.append(('ppc_stats', on))
        self._ppc_on = bool(on)

    def moran_stats(self, on):
        self.log.append(('moran_stats', on))
        self._moran_on = bool(on)

    def _rows(self, on, width, chain):
        first, keep = self._last
        rows = np.arange(first, first + (keep if on else 0), dtype=np.float64)[:, None] + np.arange(width) / 16.0
        return rows + 1000.0 * chain

    def region_draws(self, chain=0):
        self.log.append(('region_draws', chain))
        return self._rows(self._region_on, int(self._regions.max()) + 1, chain)

    def ppc_draws(self, chain=0):
        self.log.append(('ppc_draws', chain))
        return self._rows(self._ppc_on, 4, chain)

    def moran_draws(self, chain=0):
        self.log.append(('moran_draws', chain))
        return self._rows(self._moran_on, 8, chain)

    def hist_stats(self, bins):
        self.log.append(('hist_stats', bins))
        self._hist_bins = int(bins)
        if bins:
            self.count['hist'] = 0

    def hist_counts(self, chain=0):
        self.log.append(('hist_counts', chain))
        counts = np.zeros((self._hist_bins, self.prob.n), dtype=np.uint32)
        counts[chain] = self.count['hist']
        return {'bins': self._hist_bins, 'count': self.count['hist'], 'counts': counts}

    def conv_stats(self, batch):
        self.log.append(('conv_stats', batch))
        self._conv_batch = int(batch)
        if batch:
            self.count['conv'] = 0

    def conv_sums(self, chain=0):
        self.log.append(('conv_sums', chain))
        sums = np.full((11, self.prob.n), float(chain))
        sums[0] = self.count['conv']
        return {'batch': self._conv_batch, 'count': self.count['conv'], 'sums': sums}

    def holdout_data(self, W, y=None):
        assert y is None
        self.log.append(('holdout_data', int(W[0]), int(W[1])))
        self._holdout, self._holdout_on, self.count['holdout'] = np.array(W), False, 0

    def holdout_stats(self, on):
        self.log.append(('holdout_stats', on))
        self._holdout_on = bool(on)
        if on:
            self.count['holdout'] = 0

    def holdout_sums(self, chain=0):
        self.log.append(('holdout_sums', chain))
        sums = np.full((5, int(self._holdout[0])), float(self.count['holdout']))
        sums[1] *= 0.5
        sums[2:4] *= -1.0
        return {'count': self.count['holdout'], 'sums': sums}

    def run(self, n_iter, burnin=0):
        keep, C, p = n_iter - burnin, self.n_chains, self.prob
        self.log.append(('run', n_iter, burnin))
        on = {'site': self._sums_on['site'], 'll': self._sums_on['ll'], 'hist': self._hist_bins, 'conv': self._conv_batch,
              'holdout': self._holdout_on}
        for name, flag in on.items():
            if flag:
                self.count[name] += keep
        self._last = (self.t + burnin, keep)
        self.t += n_iter
        draws = np.arange(self.t - keep, self.t, dtype=np.float64)
        return (np.tile(draws[None, :, None], (C, 1, p.q)), np.tile(draws[None, :, None], (C, 1, p.p)), np.tile(draws, (C, 1)))


def _ids(n):
    return np.where(np.arange(n) % 10 == 9, -1, np.arange(n) % 7)


def _all_eight(small):
    return dict(site_summaries=True, waic=True, regions=_ids(small[2].shape[0]), ppc=True, spatial_check=True, site_intervals=True,
                site_diagnostics=True, holdout=withheld(small))


def _on(chains, *names):
    return [(name, c) for name in names for c in range(chains)]


START = [('set_start', 0), ('set', 'z', 0), ('set_start', 1), ('set', 'z', 1), ('set_start', 2), ('set', 'z', 2)]
OFF = [('sums_switch', 'site', False), ('sums_switch', 'll', False), ('regions', 7), ('ppc_stats', False), ('moran_stats', False),
       ('hist_stats', 0), ('conv_stats', 0), ('holdout_data', 12, 43)]
ON = [('sums_switch', 'site', True), ('sums_switch', 'll', True), ('region_stats', True), ('ppc_stats', True), ('moran_stats', True),
      ('hist_stats', 64), ('conv_stats', 6), ('holdout_stats', True)]
DRAWS = _on(3, 'region_draws', 'ppc_draws', 'moran_draws')
PULL = [('get', name, 0) for name in ('alpha', 'beta', 'tau', 'eta', 'z', 'omega_b', 'exists', 'omega_a')]
RESULTS = [('sums', 'site', 0), ('sums', 'site', 1), ('sums', 'site', 2), ('sums', 'll', 0), ('sums', 'll', 1), ('sums', 'll', 2),
           *_on(3, 'hist_counts', 'conv_sums', 'holdout_sums')]


def _check_results(out, kept, counted, first=0):
    """The eight results hold what the stand-in gave: ``kept`` rows per chain from iteration ``first`` on, ``counted`` iterations."""
    from occuspytial_amd.convergence import SiteDiagnostics
    from occuspytial_amd.holdout import HoldoutScore
    from occuspytial_amd.intervals import SiteIntervals
    from occuspytial_amd.ppc import PredictiveCheck
    from occuspytial_amd.regions import RegionOccupancy
    from occuspytial_amd.sites import SiteSummary
    from occuspytial_amd.spatial import SpatialCheck
    from occuspytial_amd.waic import WAIC
    kinds = dict(sites=SiteSummary, waic=WAIC, regions=RegionOccupancy, ppc=PredictiveCheck, spatial_check=SpatialCheck,
                 site_intervals=SiteIntervals, site_diagnostics=SiteDiagnostics, holdout=HoldoutScore)
    for name, cls in kinds.items():
        assert type(getattr(out, name)) is cls, name
    t = np.arange(first, first + kept, dtype=np.float64)
    want = t[None, :, None] + np.arange(7) / 16.0 + 1000.0 * np.arange(3)[:, None, None]
    assert np.array_equal(out['occupied'], want) and np.array_equal(out.regions.occupied, want) and out.regions.n_regions == 7
    assert np.array_equal(out.ppc.ft_obs, want[:, :, 0]) and np.array_equal(out.ppc.sites_detected_rep, want[:, :, 3])
    assert out.spatial_check.moran_obs.shape == (3, kept) and out.spatial_check.n == 150
    assert np.array_equal(out['tau'], np.tile(t, (3, 1))) and out['alpha'].shape == (3, kept, 2)
    assert out.sites.n_draws.tolist() == out.waic.n_draws.tolist() == out.holdout.n_draws.tolist() == [counted] * 3
    assert out.site_intervals.bins == 64 and out.site_intervals.n_draws.tolist() == [counted] * 3
    assert out.site_diagnostics.n_draws.tolist() == [counted] * 3 and out.holdout.n_sites == 12


@pytest.mark.parametrize('progressbar', [False, True])
def test_sample_with_all_eight_sends_the_calls_of_the_hand_written_threading(small, progressbar):
    """60 iterations, 20 of them burn-in, 3 chains.  With the progress bar the call runs in chunks of 16: one whole chunk of
    burn-in between the block that switches off (or sets an input) and the block that switches on, the rows read after every
    chunk that keeps a draw."""
    from occuspytial_amd import LogitICARGibbs
    s = LogitICARGibbs(*small, random_state=3)
    fake = StandIn(s._problem, 3)
    s.__dict__['_get_engine'] = lambda keys: fake
    out = s.sample(60, burnin=20, chains=3, progressbar=progressbar, **_all_eight(small))
    if progressbar:
        assert fake.log == (START + OFF + [('run', 16, 15)] + ON + [('run', 16, 4)] + DRAWS + [('run', 16, 0)] + DRAWS
                            + [('run', 12, 0)] + DRAWS + PULL + RESULTS)
    else:
        assert fake.log == START + OFF + ON + [('run', 60, 20)] + DRAWS + PULL + RESULTS
    _check_results(out, 40, 40, first=20)
    assert out.site_diagnostics.batch == 6                                        # isqrt(40)
    assert sorted(s.chain._names) == ['alpha', 'beta', 'occupied', 'tau'] and not [k for k in vars(s) if 'result' in k or 'output' in k]
    # the same engine again with nothing asked: what the call left on goes off, each the way it always went
    del fake.log[:]
    plain = s.sample(10, burnin=2, chains=3, progressbar=False)
    assert fake.log == (START + [('sums_switch', 'site', False), ('sums_switch', 'll', False), ('region_stats', False), ('ppc_stats', False),
                                 ('moran_stats', False), ('hist_stats', 0), ('conv_stats', 0), ('holdout_stats', False)]
                        + [('run', 10, 2)] + PULL)
    assert sorted(plain.data) == ['alpha', 'beta', 'tau']
    assert all(getattr(plain, name) is None for name in ('sites', 'waic', 'regions', 'ppc', 'spatial_check', 'site_intervals',
                                                         'site_diagnostics', 'holdout'))
    # and with nothing on and nothing asked, no call about any option
    fresh = StandIn(s._problem, 3)
    s.__dict__['_get_engine'] = lambda keys: fresh
    s.sample(10, burnin=2, chains=3, progressbar=False)
    assert fresh.log == START + [('run', 10, 2)] + PULL


CKPT_PLAIN = ['keys', 'n_chains']
CKPT_SUMS = ['keys', 'll_stats', 'n_chains', 'site_stats']


def _everything_on(small, prob):
    from occuspytial_amd.holdout import holdout_arg
    return dict(_sums_on={'site': True, 'll': True}, _regions=_ids(prob.n), _region_on=True, _ppc_on=True, _moran_on=True, _hist_bins=64,
                _conv_batch=6, _holdout=holdout_arg(withheld(small), prob), _holdout_on=True)


def _resume(small, restored, ckpt_sums, **asked):
    from occuspytial_amd import LogitICARGibbs
    s = LogitICARGibbs(*small, random_state=3)
    fake = StandIn(s._problem, 3, restored(small, s._problem) if restored else None)
    fake.count = dict.fromkeys(fake.count, 40 if restored else 0)
    fake.t = 60
    s.__dict__['_get_engine'] = lambda keys: fake
    ckpt = {'n_chains': np.int64(3), 'keys': np.array([1, 2, 3], dtype=np.uint64)}
    if ckpt_sums:
        ckpt.update(site_stats=np.ones(3), ll_stats=np.ones(3))
    return fake, s.resume(ckpt, 30, progressbar=False, **asked)


def test_resume_from_a_checkpoint_with_nothing_on_sets_everything_on_from_zero(small):
    fake, out = _resume(small, None, False, **_all_eight(small))
    assert fake.log == ([('restore', CKPT_PLAIN), ('sums_switch', 'site', True), ('sums_switch', 'll', True), ('regions', 7),
                         ('region_stats', True), ('ppc_stats', True), ('moran_stats', True), ('hist_stats', 64), ('conv_stats', 5),
                         ('holdout_data', 12, 43), ('holdout_stats', True), ('run', 30, 0)] + DRAWS + PULL + RESULTS)
    _check_results(out, 30, 30, first=60)
    assert out.site_diagnostics.batch == 5                                        # isqrt(30)


def test_resume_from_a_checkpoint_with_everything_on_goes_on_from_its_state(small):
    """The accumulated five go on from what the checkpoint holds -- the batch length stays the checkpoint's 6, whatever is asked
    for -- and the draws of a call are set on again, the map with them."""
    fake, out = _resume(small, _everything_on, True, **_all_eight(small))
    assert fake.log == ([('restore', CKPT_SUMS), ('regions', 7), ('region_stats', True), ('ppc_stats', True), ('moran_stats', True),
                         ('run', 30, 0)] + DRAWS + PULL + RESULTS)
    _check_results(out, 30, 70, first=60)
    assert out.site_diagnostics.batch == 6
    # other values: the histograms and the held-out sums start from zero, the batch length still stays
    few = withheld(small, k=9)
    fake, out = _resume(small, _everything_on, True, site_intervals=32, site_diagnostics=3, holdout=few)
    assert fake.log == ([('restore', CKPT_SUMS), ('ppc_stats', False), ('moran_stats', False), ('hist_stats', 32),
                         ('holdout_data', 9, sum(len(v) for v in few[1].values())), ('holdout_stats', True), ('run', 30, 0)]
                        + PULL + _on(3, 'hist_counts', 'conv_sums', 'holdout_sums'))
    assert out.site_intervals.bins == 32 and out.site_diagnostics.batch == 6 and out.holdout.n_sites == 9
    assert out.site_intervals.n_draws.tolist() == out.holdout.n_draws.tolist() == [30] * 3
    assert out.site_diagnostics.n_draws.tolist() == [70] * 3 and out.sites is None and out.regions is None


def test_resume_that_asks_nothing_leaves_the_sums_and_the_regions_and_switches_the_other_five_off(small):
    fake, out = _resume(small, _everything_on, True)
    assert fake.log == ([('restore', CKPT_SUMS), ('ppc_stats', False), ('moran_stats', False), ('hist_stats', 0), ('conv_stats', 0),
                         ('holdout_stats', False), ('run', 30, 0)] + PULL)
    assert fake._sums_on == {'site': True, 'll': True} and fake._region_on and sorted(out.data) == ['alpha', 'beta', 'tau']
    fake, out = _resume(small, None, False)
    assert fake.log == [('restore', CKPT_PLAIN), ('run', 30, 0)] + PULL


# ---- the order of the refusals ---------------------------------------------------------------------------------------------
PYTHON_STEP = ['site summaries are accumulated by', 'the log-likelihood sums of WAIC are accumulated by', 'the occupied sites per region are counted by',
               'posterior predictive checks are formed by', 'the spatial residual check is formed by', 'site intervals are accumulated by',
               'site diagnostics are accumulated by', 'held-out scoring is accumulated by']
PROBIT = ['site summaries are not available for the probit model', 'WAIC is not available for the probit model', None,
          'posterior predictive checks are not available for the probit model', 'the spatial residual check is not available for the probit model',
          'site intervals are not available for the probit model', 'site diagnostics are not available for the probit model',
          'held-out scoring is not available for the probit model']


def PyStep(*a, **k):
    """A sampler with a Python ``step`` (the package is imported inside the tests)."""
    from occuspytial_amd.gibbs.base import GibbsBase

    class PyStep(GibbsBase):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self._configure(a[0], None)

        def step(self):
            raise AssertionError('step was called')
    return PyStep(*a, **k)


def _no_engine(monkeypatch):
    from occuspytial_amd import _engine

    def no_engine(*a, **k):
        raise AssertionError('an engine was created')
    monkeypatch.setattr(_engine.Engine, '__init__', no_engine)


def test_the_first_refusal_in_table_order_is_the_one_raised(small, monkeypatch):
    from occuspytial_amd import ProbitRSRGibbs
    _no_engine(monkeypatch)
    asked = _all_eight(small)
    probit, python = ProbitRSRGibbs(*small, random_state=1, q=10), PyStep(*small, random_state=1)
    for k in range(8):
        rest = {name: asked[name] for name in KEYWORDS[k:]}
        with pytest.raises(NotImplementedError) as exc:
            python.sample(5, **rest)
        assert str(exc.value) == 'PyStep steps in Python: %s the device engine only' % PYTHON_STEP[k]
        want = PROBIT[k] or PROBIT[k + 1]                                          # (the probit sampler counts the regions)
        for call in (lambda: probit.sample(5, chains=1, progressbar=False, **rest), lambda: probit.resume({'n_chains': 1}, 5, **rest)):
            with pytest.raises(NotImplementedError) as exc:
                call()
            assert str(exc.value) == want


def test_values_come_before_burnin_and_chains_and_those_before_the_options(small, monkeypatch):
    from occuspytial_amd import LogitICARGibbs, ProbitRSRGibbs
    _no_engine(monkeypatch)
    wrong = dict(burnin=9, chains=0)
    for s in (LogitICARGibbs(*small, random_state=1), ProbitRSRGibbs(*small, random_state=1, q=10), PyStep(*small, random_state=1)):
        with pytest.raises(ValueError, match='site_intervals must be'):
            s.sample(5, site_intervals=2, site_diagnostics=0.5, regions=False, ppc=1, **wrong)
        with pytest.raises(ValueError, match='site_diagnostics must be'):
            s.sample(5, site_intervals=8, site_diagnostics=0.5, regions=False, ppc=1, **wrong)
        with pytest.raises(ValueError, match='burnin value cannot be larger'):
            s.sample(5, site_intervals=8, site_diagnostics=2, regions=False, ppc=1, **wrong)
        with pytest.raises(ValueError, match='chains must a positive'):
            s.sample(5, site_intervals=8, site_diagnostics=2, regions=False, ppc=1, chains=0)
    s = LogitICARGibbs(*small, random_state=1)
    with pytest.raises(ValueError, match='regions must be'):                       # parsed in table order: regions, ppc, ...
        s.sample(5, regions=False, ppc=1, spatial_check=1, holdout=5)
    with pytest.raises(ValueError, match='ppc must be'):
        s.sample(5, ppc=1, spatial_check=1, holdout=5)
    with pytest.raises(ValueError, match='spatial_check must be'):
        s.sample(5, spatial_check=1, holdout=5)
    with pytest.raises(ValueError, match='holdout must be a pair'):
        s.sample(5, holdout=5)
    for t in (s, ProbitRSRGibbs(*small, random_state=1, q=10)):                    # resume: the two values, the size, the options
        with pytest.raises(ValueError, match='site_intervals must be'):
            t.resume({'n_chains': 1}, 0, site_intervals=2, site_diagnostics=0.5, regions=False)
        with pytest.raises(ValueError, match='site_diagnostics must be'):
            t.resume({'n_chains': 1}, 0, site_diagnostics=0.5, regions=False)
        with pytest.raises(ValueError, match='size must be a positive integer'):
            t.resume({'n_chains': 1}, 0, regions=False)
        with pytest.raises(ValueError, match='regions must be'):
            t.resume({'n_chains': 1}, 5, regions=False, ppc=1)
    # a probit sampler refuses ppc after it has looked at it, and held-out scoring before
    p = ProbitRSRGibbs(*small, random_state=1, q=10)
    with pytest.raises(ValueError, match='ppc must be'):
        p.sample(5, ppc=1)
    with pytest.raises(NotImplementedError, match='held-out scoring'):
        p.sample(5, holdout=5)


def test_probit_resume_refuses_the_sums_before_an_engine_exists(small, monkeypatch):
    """The sums are refused with the other options: no engine is built and restored first."""
    from occuspytial_amd import ProbitRSRGibbs
    _no_engine(monkeypatch)
    with pytest.raises(NotImplementedError, match='site summaries are not available for the probit model'):
        ProbitRSRGibbs(*small, random_state=1, q=10).resume({'n_chains': 1}, 5, site_summaries=True)
    with pytest.raises(NotImplementedError, match='WAIC is not available for the probit model'):
        ProbitRSRGibbs(*small, random_state=1, q=10).resume({'n_chains': 1}, 5, waic=True)
