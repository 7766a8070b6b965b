"""What the GPU tests of the optional outputs share (tests/test_gpu_site_summaries.py to tests/test_gpu_holdout.py): the engine
with some outputs switched on, the time limit of a test, and the two calls whose results the scheduling tests compare."""
import signal

import numpy as np
import pytest


def engine_with(prob, keys, starts, site=False, ll=False, ids=None, region_on=True, ppc=False, moran=False, bins=0, conv=0,
                holdout=None, holdout_on=True):
    """An ``Engine`` at ``starts`` (a start may hold ``eps``, the probit model's) with the outputs asked for switched on, in the
    one order every test uses: site sums, log-likelihood sums, regions (the map ``ids``, its switch with ``region_on``), PPC,
    Moran, histograms of ``bins``, batch means of length ``conv``, the withheld data ``holdout`` = (W, y) and their switch."""
    from occuspytial_amd._engine import Engine
    eng = Engine(prob, keys)
    for c, st in enumerate(starts):
        st = dict(st)
        eps = st.pop('eps', None)
        eng.set_start(c, **st)
        if eps is not None:
            eng.set('eps', eps, c)
    if site:
        eng.site_stats(True)
    if ll:
        eng.loglik_stats(True)
    if ids is not None:
        eng.regions(ids)
        if region_on:
            eng.region_stats(True)
    if ppc:
        eng.ppc_stats(True)
    if moran:
        eng.moran_stats(True)
    if bins:
        eng.hist_stats(bins)
    if conv:
        eng.conv_stats(conv)
    if holdout is not None:
        eng.holdout_data(*holdout)
        if holdout_on:
            eng.holdout_stats(True)
    return eng


@pytest.fixture(autouse=True)
def time_limit(request):
    """300 s per test (each takes seconds).  A module imports it as ``_time_limit``: autouse holds in that module."""
    def late(signum, frame):
        raise TimeoutError(f'a test of {request.module.__name__.rpartition(".")[2]}.py ran past its time limit')
    old = signal.signal(signal.SIGALRM, late)
    signal.alarm(300)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def two_calls(make_engine, read, split=((33, 4), (10, 0)), per_call=False):
    """run(33, 4) then run(10, 0) on ``make_engine()`` -> ``read(eng)`` after the last call (what accumulates across calls);
    ``per_call``: read after every call and joined per chain (the draws of a call, which every call starts anew)."""
    eng = make_engine()
    parts = []
    for n_iter, burnin in split:
        eng.run(n_iter, burnin)
        if per_call:
            parts.append(read(eng))
    out = [np.concatenate(rows) for rows in zip(*parts)] if per_call else read(eng)
    eng.close()
    return out
