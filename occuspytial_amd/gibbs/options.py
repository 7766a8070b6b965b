"""The optional outputs of ``sample`` and ``resume``: one row each in ``OPTIONS``, in the order of the keywords.

A row is the only place that states an option's keyword and default, the attribute of ``PosteriorParameter`` that holds its
result, how the keyword's value becomes what the engine is asked for (and when: ``parsed``), its three message texts, the
``Engine`` attribute that tells that an earlier call left it on, what is called in each of a call's four phases -- ``before``
the first chunk, ``on`` before the first chunk that keeps a draw, ``read`` after a kept chunk, ``finish`` at the end -- and its
rule for ``resume``.  The samplers loop over the rows (``GibbsBase.sample``, ``LogitICARGibbs._run_chains`` and ``resume``).

The rows come in the three families of the native side: the per-site running sums (``_lib.SUMS_KINDS``), the draws of a call
(``_lib.DRAWS_KINDS``: rows read after every chunk; nothing of them is carried over a checkpoint) and the accumulators behind
the z update (``_lib.ACCUM_KINDS``).  A ninth option is a row here, a keyword with its paragraph in ``sample`` and ``resume``, an attribute
of ``PosteriorParameter`` and the ``Engine`` methods the row names.
"""
import numpy as np

from .. import _lib
from ..convergence import SiteDiagnostics, diagnostics_batch
from ..holdout import HoldoutScore, holdout_arg
from ..intervals import SiteIntervals, interval_bins
from ..ppc import PredictiveCheck, ppc_flag
from ..regions import RegionOccupancy, region_ids
from ..sites import SiteSummary
from ..spatial import SpatialCheck, spatial_flag
from ..waic import WAIC

# when a keyword's value is looked at: before the checks of burnin, chains and size, or in table order next to the refusal
FIRST, BEFORE, AFTER = 'first', 'before the refusal', 'after the refusal'


class Option:
    """What the families share.  ``want`` is what the engine is asked for (``parse`` of the keyword's value): None if not asked."""
    default = False        # of the keyword: not asked
    parsed = BEFORE
    input = None           # the Engine method that takes the option's input, set with every chain's switch off
    off = False            # what the switch takes for off, and what an engine that does not know the option has it at
    draws = None           # the Engine method that reads a chain's rows of the last run
    vector = None          # the name under which the rows of a call join the chains
    resume_leaves = False  # resume, not asked: left as the checkpoint set it (else switched off)

    def __init__(self, keyword, result, parse, python_step, probit, rebuild, **rules):
        self.keyword, self.result, self.parse = keyword, result, parse
        # the refusals: of a sampler that steps in Python (after the class's name), of the probit sampler (None: it allows the
        # option), and the middle of 'the loaded engine library ... (...): rebuild it'
        self.python_step, self.probit, self.rebuild = 'steps in Python: ' + python_step, probit, rebuild
        vars(self).update(rules)   # switch, left_on (the Engine method and attribute) and what differs from the defaults above

    @property
    def methods(self):
        """The ``Engine`` / ``EngineGroup`` methods the row calls."""
        return tuple(name for name in (self.input, self.switch, self.draws) if name)

    def is_on(self, eng):
        return getattr(eng, self.left_on, self.off)   # (a stand-in engine of the tests knows only its own feature)

    def set(self, eng, value):
        getattr(eng, self.switch)(value)

    def rebuilt(self, call, *args):
        try:
            return call(*args)
        except ValueError as exc:   # a stale build, or a stand-in library that does not know the state names
            raise ValueError(f'the loaded engine library {self.rebuild} ({exc}): rebuild it') from None

    def before(self, eng, want):
        """Before the first chunk: off during burn-in -- asked, or left on by an earlier call on a reused engine -- which is also
        the early answer of a library that does not know the option.  An option with an input sets it instead (the engine
        then switches every chain off), and its bare switch-off of a reused engine answers for itself."""
        if self.input is None:
            if want is not None or self.is_on(eng):
                self.rebuilt(self.set, eng, self.off)
        elif want is not None:
            self.rebuilt(getattr(eng, self.input), want)
        elif self.is_on(eng):
            self.set(eng, self.off)

    def on(self, eng, want):
        """Before the first chunk that keeps a draw (which zeroes what accumulates).  A refusal here is a real one -- the spatial
        check's "every off-diagonal of Q <= 0" -- and keeps its own text."""
        self.set(eng, True if self.input else want)

    def rows(self, chains, keep, want):
        return None

    def read(self, eng, rows, lo, hi):
        """After a chunk that kept the draws ``lo`` to ``hi``."""

    def finish(self, eng, problem, want, rows):
        return self.cls.from_engine(eng)

    def carried(self, eng, want, checkpoint):
        return False

    def resume(self, eng, want, checkpoint):
        """After ``restore``.  Asked: on from zero (the input first) unless the option is ``carried``, that is, goes on from
        what the checkpoint holds.  Not asked: left as restored, or switched off -- bare, as in ``before``."""
        if want is None:
            if not self.resume_leaves and self.is_on(eng):
                self.set(eng, self.off)
        elif not self.carried(eng, want, checkpoint):
            self.rebuilt(self._from_zero, eng, want)

    def _from_zero(self, eng, want):
        if self.input:
            getattr(eng, self.input)(want)
        self.set(eng, True if self.input else want)


class Sums(Option):
    """Per-site running sums of one kind: switched by ``eng.sums_switch(kind, on)``, they accumulate across ``resume`` -- from
    zero only if the checkpoint lacks the kind's switch -- and stay as restored when a ``resume`` does not ask."""
    switch, left_on, resume_leaves = 'sums_switch', '_sums_on', True

    def __init__(self, keyword, result, kind, cls, python_step, probit):
        super().__init__(keyword, result, lambda value, problem, kept: True if value else None, python_step, probit,
                         'has no ' + _lib.SUMS_KINDS[kind].what, kind=kind, cls=cls)

    def is_on(self, eng):
        return getattr(eng, self.left_on, {}).get(self.kind)

    def set(self, eng, value):
        eng.sums_switch(self.kind, value)

    def on(self, eng, want):
        self.rebuilt(self.set, eng, True)   # (the one switch-on of a sample call that answers "rebuild it": it always has)

    def carried(self, eng, want, checkpoint):
        return _lib.SUMS_KINDS[self.kind].fields[0] in checkpoint


class Draws(Option):
    """Rows of the draws a call keeps, ``width`` numbers per draw, read with ``draws`` after every kept chunk; ``make`` turns them
    into the result.  They belong to a call: ``resume`` always sets the option on, whatever the checkpoint held."""

    def rows(self, chains, keep, want):
        return np.zeros((chains, keep, self.width(want)))

    def read(self, eng, rows, lo, hi):
        rows[:, lo:hi] = [getattr(eng, self.draws)(c) for c in range(len(rows))]

    def finish(self, eng, problem, want, rows):
        return self.make(problem, want, rows)


class Accum(Option):
    """An accumulator behind the z update: the switch's value is what is asked for (bins, batch length, True), the result is
    read from the engine at the end.  ``same(eng, on, want)``: ``resume`` goes on from what the checkpoint left ``on``."""

    def carried(self, eng, want, checkpoint):
        return self.same(eng, self.is_on(eng), want)


OPTIONS = (
    # (the probit z update conditions on the auxiliary eps: what "psi" should mean there is a modelling decision not yet made,
    # and the site's marginal likelihood is not what it forms)
    Sums('site_summaries', 'sites', 'site', SiteSummary,
         python_step='site summaries are accumulated by the device engine only',
         probit='site summaries are not available for the probit model'),
    Sums('waic', 'waic', 'll', WAIC,
         python_step='the log-likelihood sums of WAIC are accumulated by the device engine only',
         probit='WAIC is not available for the probit model'),
    # (the occupied sites per region ARE counted by the probit sampler: its z is drawn as the reference draws it)
    Draws('regions', 'regions', lambda value, problem, kept: region_ids(value, problem.n), default=None,
          python_step='the occupied sites per region are counted by the device engine only', probit=None,
          rebuild='does not count the occupied sites per region',
          input='regions', switch='region_stats', left_on='_region_on', resume_leaves=True, draws='region_draws',
          width=lambda ids: max(int(ids.max()) + 1, 1), vector='occupied',
          make=lambda problem, ids, rows: RegionOccupancy(ids, problem.obs, rows)),
    # (the probit detection part is a probit regression on the auxiliary scale: a check of it is out of scope so far)
    Draws('ppc', 'ppc', lambda value, problem, kept: ppc_flag(value) or None,
          python_step='posterior predictive checks are formed by the device engine only',
          probit='posterior predictive checks are not available for the probit model', rebuild='has no posterior predictive check',
          switch='ppc_stats', left_on='_ppc_on', draws='ppc_draws', width=lambda on: _lib.DRAWS_KINDS['ppc'].width,
          make=lambda problem, on, rows: PredictiveCheck.from_problem(problem, rows)),
    # (the probit psi is the modelling decision DESIGN 11 leaves open: this one and the three below)
    Draws('spatial_check', 'spatial_check', lambda value, problem, kept: spatial_flag(value) or None,
          python_step='the spatial residual check is formed by the device engine only',
          probit='the spatial residual check is not available for the probit model', rebuild='has no spatial residual check',
          switch='moran_stats', left_on='_moran_on', draws='moran_draws', width=lambda on: _lib.DRAWS_KINDS['moran'].width,
          make=lambda problem, on, rows: SpatialCheck.from_problem(problem, rows)),
    Accum('site_intervals', 'site_intervals', lambda value, problem, kept: interval_bins(value) or None, parsed=FIRST,
          python_step='site intervals are accumulated by the device engine only',
          probit='site intervals are not available for the probit model', rebuild='has no site intervals',
          switch='hist_stats', left_on='_hist_bins', off=0, cls=SiteIntervals,
          same=lambda eng, bins, want: bins == want),                  # (none, or of another number of bins: from zero)
    Accum('site_diagnostics', 'site_diagnostics', lambda value, problem, kept: diagnostics_batch(value, kept) or None, parsed=FIRST,
          python_step='site diagnostics are accumulated by the device engine only',
          probit='site diagnostics are not available for the probit model', rebuild='has no site diagnostics',
          switch='conv_stats', left_on='_conv_batch', off=0, cls=SiteDiagnostics,
          same=lambda eng, batch, want: bool(batch)),                  # (the checkpoint's batch length stays whenever it has one)
    Accum('holdout', 'holdout', lambda value, problem, kept: None if value is None else holdout_arg(value, problem), default=None,
          parsed=AFTER, python_step='held-out scoring is accumulated by the device engine only',
          probit='held-out scoring is not available for the probit model', rebuild='has no held-out scoring',
          input='holdout_data', switch='holdout_stats', left_on='_holdout_on', cls=HoldoutScore,
          same=lambda eng, on, want: on and np.array_equal(eng._holdout, want)),   # (none, or of other data: from zero)
)


def parse_first(given, problem, kept):
    """The values that are looked at before anything else is checked: keyword -> what the engine is asked for, or None."""
    return {o.keyword: o.parse(given[o.keyword], problem, kept) for o in OPTIONS if o.parsed == FIRST}


def ask(sampler, given, kept, first):
    """Validate and refuse in table order, before an engine exists -> {keyword: what the engine is asked for} of the options
    asked, none of the others.  ``given`` maps every keyword to its value, ``first`` is ``parse_first`` of it, and
    ``sampler._refusal(option)`` is the sampler's reason to refuse an option, or None."""
    asked = {}
    for o in OPTIONS:
        reason = sampler._refusal(o)
        if o.parsed == AFTER and reason and given[o.keyword] is not o.default:
            raise NotImplementedError(reason)
        want = first[o.keyword] if o.parsed == FIRST else o.parse(given[o.keyword], sampler._problem, kept)
        if want is not None:
            if reason:
                raise NotImplementedError(reason)
            asked[o.keyword] = want
    return asked
