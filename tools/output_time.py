"""Cost of one optional output of sample/resume: us per iteration of occ_run with its switch on against the switch off of the
SAME build, at 100x100 x 4 chains (the headline workload) and 500x500 x 1 chain.

    python tools/output_time.py FEATURE [options]        FEATURE: a row of FEATURES below

Per size: 200 warm-up iterations, then 2 000 kept iterations timed in the feature's modes, alternating, three times each (a
short re-warm after every flip: a flip that changes the z kernel or the launches of an iteration drops the captured graphs).
With --kernels (the features whose switch replaces k_z_ob) the in-graph launch time of k_z_ob from occ_profile, which always
times the kernel that accumulates nothing, is added for scale.  One JSON line per size, appended to --out
(profiles/FEATURE_time.jsonl): the common columns, the feature's own, and what was read after the feature's last switched-on
pass -- a count there is the pass's 2 000 iterations and the one kept iteration of the re-warm call before them.

Every size runs in a child process of its own under a time limit; a child that fails or runs out of time ends the tool with
its exit status, and nothing further is started on the device."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace
from typing import Callable, NamedTuple

import numpy as np

TOOLS = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(TOOLS), TOOLS]

SIZES = ((100, 100, 4), (500, 500, 1))
WORKLOAD = dict(visits=5, p=2, q=2, random_state=0)
KERNELS = ('--kernels',)


class Feature(NamedTuple):
    modes: tuple                # in the order they are timed; every mode but 'off' gets an _increase_us column
    flip: Callable              # (eng, mode, c): what a mode does to the engine before its re-warm
    capture: Callable           # (eng, c) -> c.last
    after: str                  # ... after every pass of this mode (None: once, after the last pass)
    columns: Callable           # (c, t) -> the JSON line in its order; t: the timing columns
    option: tuple = KERNELS     # the feature's own option: KERNELS, (flag, default, help) or None
    edit: Callable = None       # (c) -> edit(W, y) of tools/_workload.py, before the problem is built
    setup: Callable = None      # (eng, c), before the warm-up
    limit: int = 300            # seconds per size


def _guarded(switch, state, on_value=lambda c: True, off_value=False):
    """A flip that reaches the engine only when the mode wants the switch on or the engine has it on."""
    def flip(eng, mode, c):
        if mode != 'off' or getattr(eng, state):
            getattr(eng, switch)(on_value(c) if mode != 'off' else off_value)
    return flip


def _stacked(reader):
    return lambda eng, c: np.stack([getattr(eng, reader)(k) for k in range(c.chains)])


def _flip_waic(eng, mode, c):
    eng.loglik_stats(mode in ('ll', 'both'))
    eng.site_stats(mode in ('site', 'both'))


def _region_maps(eng, c):
    """g1: the whole lattice as one region; g64: an 8 x 8 grid of blocks."""
    r, col = np.divmod(np.arange(c.rows * c.cols), c.cols)
    c.maps = {'g1': np.zeros(c.rows * c.cols, dtype=np.int64), 'g64': (r * 8 // c.rows) * 8 + col * 8 // c.cols}


def _flip_regions(eng, mode, c):
    eng.site_stats(mode == 'site')      # (alone, for scale: it moves 80 B per site)
    if mode in c.maps:
        eng.regions(c.maps[mode])       # (switches off first)
        eng.region_stats(True)
    elif eng._region_on:
        eng.region_stats(False)


def _flip_ppc(eng, mode, c):
    eng.loglik_stats(mode == 'll')      # (alone, for scale: the same loop over every surveyed site's rows, without the Philox block)
    if mode == 'ppc' or eng._ppc_on:
        eng.ppc_stats(mode == 'ppc')


def _withhold(c):
    """Every c.opt-th site is left out of the problem and held out with its visits."""
    c.held = list(range(0, c.rows * c.cols, c.opt))

    def edit(W, y):
        c.Wt, c.yt = {s: W.pop(s) for s in c.held}, {s: y.pop(s) for s in c.held}
    return edit


def _site_stats_line(c, t):
    return {**c.size, **c.run, **c.solve, 'on_us': t['on_us'], 'off_us': t['off_us'], 'on_median_us': t['on_median_us'],
            'off_median_us': t['off_median_us'], 'increase_us': t['on_increase_us'], 'bytes_per_iteration': 80 * c.cells,
            'last_count': c.last}


def _regions_line(c, t):
    return {**c.size, **c.run, **c.solve, 'last_rows': list(c.last.shape),
            'last_mean_pao': float((c.last / np.bincount(c.maps['g64'], minlength=64)).mean()), **t}


def _result(module, cls):
    """The class that reads a feature's output, looked up when it is needed (the parent process never imports the package)."""
    return getattr(importlib.import_module('occuspytial_amd.' + module), cls)


def _check_line(module, cls, field):
    """ppc and spatial: the rows of every chain, and what the feature's check says of them."""
    def line(c, t):
        check = _result(module, cls).from_problem(c.prob, c.last)
        return {**c.size, 'R': int(c.prob.R), 'detection_sites': int(np.count_nonzero(c.prob.obs_site)), **c.run, **c.solve,
                'last_rows': list(c.last.shape), 'last_p_value': check.p_value, 'last_' + field: getattr(check, field), **t}
    return line


def _from_engine(module, cls):
    return lambda eng, c: _result(module, cls).from_engine(eng)


def _sums_line(own, last):
    """hist, conv and holdout: ``own(c)`` columns, every chain's count and one figure ``last(c.last)`` from the sums."""
    def line(c, t):
        name, value = last(c.last)
        return {**c.size, 'R': int(c.prob.R), **c.run, **own(c), **c.solve, 'last_count': c.last.n_draws.tolist(), name: float(value), **t}
    return line


FEATURES = {
    'site_stats': Feature(
        ('on', 'off'), lambda eng, mode, c: eng.site_stats(mode == 'on'),
        lambda eng, c: int(eng.get('site_count', 0)[0]), None, _site_stats_line, limit=240),
    'waic': Feature(
        ('ll', 'off', 'both', 'site'), _flip_waic, lambda eng, c: int(eng.get('ll_count', 0)[0]), 'both',
        lambda c, t: {**c.size, **c.run, **c.solve, 'bytes_per_iteration_ll': 48 * c.cells, 'last_count': c.last, **t}),
    'regions': Feature(
        ('off', 'g1', 'g64', 'site'), _flip_regions, lambda eng, c: eng.region_draws(0), 'g64', _regions_line, setup=_region_maps),
    'ppc': Feature(
        ('off', 'ppc', 'll'), _flip_ppc, _stacked('ppc_draws'), 'ppc', _check_line('ppc', 'PredictiveCheck', 'c_hat')),
    'spatial': Feature(
        ('off', 'moran'), _guarded('moran_stats', '_moran_on'), _stacked('moran_draws'), 'moran',
        _check_line('spatial', 'SpatialCheck', 'excess'), option=None),
    'hist': Feature(
        ('off', 'hist'), _guarded('hist_stats', '_hist_bins', lambda c: c.opt, 0), _from_engine('intervals', 'SiteIntervals'), 'hist',
        _sums_line(lambda c: {'bins': c.opt, 'histogram_bytes': 4 * c.opt * c.cells}, lambda s: ('last_width95', np.mean(s.width()))),
        option=('--bins', 64, None)),
    'conv': Feature(
        ('off', 'conv'), _guarded('conv_stats', '_conv_batch', lambda c: c.opt, 0), _from_engine('convergence', 'SiteDiagnostics'), 'conv',
        _sums_line(lambda c: {'batch': c.opt, 'sums_bytes': 88 * c.cells}, lambda s: ('last_median_ess_eta', np.nanmedian(s.ess('eta')))),
        option=('--batch', 44, 'floor(sqrt(2000))')),
    'holdout': Feature(
        ('off', 'holdout'), _guarded('holdout_stats', '_holdout_on'), _from_engine('holdout', 'HoldoutScore'), 'holdout',
        _sums_line(lambda c: {'held_out': len(c.held), 'held_rows': int(sum(len(v) for v in c.yt.values())),
                              'sums_bytes': 40 * len(c.held) * c.chains}, lambda s: ('last_elpd', s.elpd)),
        option=('--every', 5, 'every k-th site is withheld (5: 20 %%)'), edit=_withhold,
        setup=lambda eng, c: eng.holdout_data(c.Wt, c.yt)),
}


def measure(feature, rows, cols, chains, iters, warm, reps, opt=None):
    """-> the JSON line of one size.  ``opt``: the value of the feature's own option (--kernels: whether it was given)."""
    from _workload import lattice_engine
    row = FEATURES[feature]
    if opt is None and row.option and row.option != KERNELS:
        opt = row.option[1]
    c = SimpleNamespace(rows=rows, cols=cols, chains=chains, cells=rows * cols * chains, opt=opt, last=None,
                        size={'shape': f'{rows}x{cols}', 'n': rows * cols}, run={'chains': chains, 'iters': iters})
    c.prob, eng = lattice_engine(rows, cols, chains, edit=row.edit and row.edit(c), **WORKLOAD)
    if row.setup:
        row.setup(eng, c)
    eng.run(warm, warm - 1)
    us = {mode: [] for mode in row.modes}
    for _ in range(reps):
        for mode in row.modes:
            row.flip(eng, mode, c)
            eng.run(50, 49)
            t0 = time.perf_counter()
            eng.run(iters, 0)
            us[mode].append(1e6 * (time.perf_counter() - t0) / iters)
            if mode == row.after:
                c.last = row.capture(eng, c)
    if row.after is None:
        c.last = row.capture(eng, c)
    st = eng.stats()
    c.solve = {'persistent_solve': st['persistent_solve'], 'fused_fallbacks': st['fused_fallbacks']}
    t = {}
    for mode in row.modes:
        t[mode + '_us'] = [round(v, 3) for v in us[mode]]
        t[mode + '_median_us'] = float(np.median(us[mode]))
    for mode in row.modes:
        if mode != 'off':
            t[mode + '_increase_us'] = t[mode + '_median_us'] - t['off_median_us']
    out = row.columns(c, t)
    if row.option == KERNELS and opt:
        out['z_ob_profile_us'] = round(eng.profile(50)['z_ob']['avg_us'], 2)
    eng.close()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    sub = ap.add_subparsers(dest='feature', required=True, metavar='FEATURE')
    for name, row in FEATURES.items():
        p = sub.add_parser(name)
        p.add_argument('--iters', type=int, default=2000)
        p.add_argument('--warm', type=int, default=200)
        p.add_argument('--reps', type=int, default=3)
        if row.option == KERNELS:
            p.add_argument('--kernels', action='store_true')
        elif row.option:
            p.add_argument(row.option[0], type=int, default=row.option[1], help=row.option[2])
        p.add_argument('--limit', type=int, default=row.limit, help='seconds per size')
        p.add_argument('--out', default=os.path.join(os.path.dirname(TOOLS), 'profiles', name + '_time.jsonl'))
        p.add_argument('--one', type=int, nargs=3, metavar=('ROWS', 'COLS', 'CHAINS'), help='(child) measure this size and print its line')
    a = ap.parse_args(argv)
    option = FEATURES[a.feature].option
    opt = option and getattr(a, option[0][2:])
    if a.one:
        print(json.dumps(measure(a.feature, *a.one, a.iters, a.warm, a.reps, opt)), flush=True)
        return 0
    own = [] if not option else ['--kernels'] * opt if option == KERNELS else [option[0], str(opt)]
    for rows, cols, chains in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), a.feature, '--one', str(rows), str(cols), str(chains), '--iters', str(a.iters),
               '--warm', str(a.warm), '--reps', str(a.reps)] + own
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            print(f'{rows}x{cols}: no result within {a.limit} s; stopping', file=sys.stderr)
            return 124
        if r.returncode != 0:
            print(f'{rows}x{cols}: exit status {r.returncode}; stopping', file=sys.stderr)
            return r.returncode if r.returncode > 0 else 1
        line = r.stdout.strip().splitlines()[-1]
        json.loads(line)
        print(line, flush=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
