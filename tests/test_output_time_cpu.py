"""tools/output_time.py against the record of the eight tools it replaced (site_stats_time.py, waic_time.py, regions_time.py,
ppc_time.py, spatial_time.py, hist_time.py, conv_time.py, holdout_time.py).

``tests/golden/output_time_calls.json`` holds, per feature and with --kernels off and on where the feature has it, what the old
tool's ``measure`` did to a recording stand-in of ``Engine`` at 9x11 x 2 chains, iters=5, warm=3, reps=2, every option at its
default: every call in order with its arguments (arrays as shape, dtype and a checksum), the two ``perf_counter`` calls of
every pass among them, and the keys of its JSON line in order with their values' types.  It was recorded with ``record`` below
before the old tools were deleted; the new tool must do the same.  An extra or a missing flip of a switch drops the captured
graphs once more or once less, so it changes what is timed: it shows here as a changed log.  The runner is tested with
``subprocess.run`` replaced."""
import importlib.util
import json
import os
import subprocess
import zlib
from types import SimpleNamespace
from unittest import mock

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'output_time_calls.json')
SIZE, RUN = (9, 11, 2), (5, 3, 2)       # rows, cols, chains; iters, warm, reps
OPTIONS = {'site_stats': 'kernels', 'waic': 'kernels', 'regions': 'kernels', 'ppc': 'kernels', 'spatial': None, 'hist': 'bins',
           'conv': 'batch', 'holdout': 'every'}
RESULTS = {'ppc': 'PredictiveCheck', 'spatial': 'SpatialCheck', 'intervals': 'SiteIntervals', 'convergence': 'SiteDiagnostics',
           'holdout': 'HoldoutScore'}
CASES = [(f, k) for f, o in OPTIONS.items() for k in ((False, True) if o == 'kernels' else (False,))]


def load_tool(path='tools/output_time.py'):
    spec = importlib.util.spec_from_file_location(os.path.basename(path)[:-3], os.path.join(ROOT, path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _short(v):
    """An argument as the log keeps it.  A float array's checksum is taken at six decimals, so that the last bits of a start
    value, which may differ between two builds of numpy, do not enter it."""
    if isinstance(v, np.ndarray):
        data = np.round(v, 6) + 0.0 if v.dtype.kind == 'f' else v
        return {'shape': list(v.shape), 'dtype': str(v.dtype), 'crc': zlib.crc32(np.ascontiguousarray(data).tobytes())}
    if isinstance(v, dict):
        return {str(k): _short(u) for k, u in v.items()}
    if isinstance(v, (list, tuple)):
        return [_short(u) for u in v]
    return v.item() if isinstance(v, np.generic) else v


def _type(v):
    return 'list[%s]' % '|'.join(sorted({_type(u) for u in v})) if isinstance(v, list) else type(v).__name__


class RecordingEngine:
    """Stand-in for ``Engine``: logs every call, keeps the private attributes the tools' guards read, and answers the readers
    with canned arrays of the right shapes."""
    log = None      # (the list of the recording in progress)

    def __init__(self, prob, keys):
        self.prob, self.n_chains, self._kept, self._width = prob, len(keys), 0, 1
        self._region_on = self._ppc_on = self._moran_on = self._holdout_on = False
        self._hist_bins = self._conv_batch = 0
        self._say('Engine', {'n': int(prob.n), 'R': int(prob.R), 'S': int(prob.S)}, list(keys))

    def _say(self, name, *args):
        self.log.append([name] + [_short(a) for a in args])

    def set_start(self, chain, alpha, beta, tau, eta):
        self._say('set_start', chain, alpha, beta, tau, eta)

    def run(self, n_iter, burnin=0):
        self._kept = n_iter - burnin
        self._say('run', n_iter, burnin)

    def site_stats(self, on):
        self._say('site_stats', on)

    def loglik_stats(self, on):
        self._say('loglik_stats', on)

    def regions(self, ids):
        self._region_on, self._width = False, int(np.max(ids)) + 1      # (the engine switches off before it takes a map)
        self._say('regions', ids)

    def region_stats(self, on):
        self._region_on = bool(on)
        self._say('region_stats', on)

    def ppc_stats(self, on):
        self._ppc_on = bool(on)
        self._say('ppc_stats', on)

    def moran_stats(self, on):
        self._moran_on = bool(on)
        self._say('moran_stats', on)

    def hist_stats(self, bins):
        self._hist_bins = int(bins)
        self._say('hist_stats', bins)

    def conv_stats(self, batch):
        self._conv_batch = int(batch)
        self._say('conv_stats', batch)

    def holdout_data(self, W, y=None):
        self._holdout_on = False
        self._say('holdout_data', W, y)

    def holdout_stats(self, on):
        self._holdout_on = bool(on)
        self._say('holdout_stats', on)

    def get(self, name, chain=0):
        self._say('get', name, chain)
        return np.array([float(self._kept + 1)])

    def _draws(self, name, chain, width):
        self._say(name, chain)
        return np.arange(self._kept * width).reshape(self._kept, width) % 3

    def region_draws(self, chain=0):
        return self._draws('region_draws', chain, self._width)

    def ppc_draws(self, chain=0):
        return self._draws('ppc_draws', chain, 4).astype(np.float64)

    def moran_draws(self, chain=0):
        return self._draws('moran_draws', chain, 8).astype(np.float64)

    def stats(self):
        self._say('stats')
        return {'persistent_solve': 1, 'fused_fallbacks': 0}

    def profile(self, reps=200):
        self._say('profile', reps)
        return {'z_ob': {'avg_us': 12.3456}}

    def close(self):
        self._say('close')


def result_standin(cls_name):
    """Stand-in for a class that reads a feature's output: logs how it was made and answers what the tools read of it."""
    class Result:
        p_value, c_hat, excess, elpd = 0.25, 1.5, 0.125, np.float64(-3.5)

        def __init__(self, chains):
            self.n_draws = np.full(chains, 6)

        @classmethod
        def from_problem(cls, prob, rows):
            RecordingEngine.log.append([cls_name + '.from_problem', _short(rows)])
            return cls(rows.shape[0])

        @classmethod
        def from_engine(cls, eng):
            RecordingEngine.log.append([cls_name + '.from_engine'])
            return cls(eng.n_chains)

        def width(self, level=0.95):
            return np.array([0.5, 0.25])

        def ess(self, name):
            RecordingEngine.log.append([cls_name + '.ess', name])
            return np.array([4.0, np.nan, 8.0])
    return Result


def record(measure, *args):
    """-> {'log', 'keys'} of one ``measure(*args)`` against the stand-ins, with ``time.perf_counter`` a logged counter."""
    log, ticks = [], iter(range(10 ** 6))

    def perf_counter():
        log.append(['perf_counter'])
        return 0.001 * next(ticks)
    with mock.patch('occuspytial_amd._engine.Engine', RecordingEngine), mock.patch.object(RecordingEngine, 'log', log), \
            mock.patch('time.perf_counter', perf_counter):
        patches = [mock.patch(f'occuspytial_amd.{module}.{cls}', result_standin(cls)) for module, cls in RESULTS.items()]
        for p in patches:
            p.start()
        try:
            out = measure(*args)
        finally:
            for p in patches:
                p.stop()
    return {'log': json.loads(json.dumps(log)), 'keys': [[k, _type(v)] for k, v in json.loads(json.dumps(out)).items()]}


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_record_covers_every_feature_with_and_without_kernels(recorded):
    assert sorted(recorded) == sorted(f + ('+kernels' if k else '') for f, k in CASES) and len(CASES) == 12
    assert list(load_tool().FEATURES) == list(OPTIONS)


@pytest.mark.parametrize('feature,kernels', CASES)
def test_measure_does_to_the_engine_what_the_old_tool_did(recorded, feature, kernels):
    """The same calls in the same order with the same arguments, and a JSON line of the same keys, order and types."""
    want = recorded[feature + ('+kernels' if kernels else '')]
    got = record(load_tool().measure, feature, *SIZE, *RUN, kernels if OPTIONS[feature] == 'kernels' else None)
    assert got['keys'] == want['keys']
    assert ('z_ob_profile_us' in dict(got['keys'])) == kernels
    for i, (g, w) in enumerate(zip(got['log'], want['log'])):
        assert g == w, (i, g, w)
    assert len(got['log']) == len(want['log'])
    # (and the record is one of the protocol: per pass a re-warm, then the two clock readings around the timed call alone)
    runs = [i for i, e in enumerate(got['log']) if e == ['run', 5, 0]]
    assert len(runs) == 2 * len(load_tool().FEATURES[feature].modes)
    for i in runs:
        assert got['log'][i - 2:i + 2] == [['run', 50, 49], ['perf_counter'], ['run', 5, 0], ['perf_counter']]


# ------------------------------------------------------------------ the runner
def _children(monkeypatch, answer):
    """``subprocess.run`` replaced: every call is noted and answered by ``answer(number of the call)``."""
    calls = []

    def run(cmd, **kw):
        calls.append((cmd, kw))
        return answer(len(calls))
    monkeypatch.setattr(subprocess, 'run', run)
    return calls


@pytest.mark.parametrize('status,ends_with', [(3, 3), (-11, 1)])
def test_a_failing_child_ends_the_tool_with_its_status_and_nothing_further_is_started(monkeypatch, tmp_path, status, ends_with):
    calls = _children(monkeypatch, lambda k: SimpleNamespace(returncode=status, stdout=''))
    out = tmp_path / 'lines.jsonl'
    assert load_tool().main(['hist', '--out', str(out)]) == ends_with
    assert len(calls) == 1 and not out.exists()


def test_a_child_past_its_time_limit_ends_the_tool_with_124_and_nothing_further_is_started(monkeypatch, tmp_path):
    def late(k):
        raise subprocess.TimeoutExpired('child', 7)
    calls = _children(monkeypatch, late)
    out = tmp_path / 'lines.jsonl'
    assert load_tool().main(['waic', '--kernels', '--limit', '7', '--out', str(out)]) == 124
    assert len(calls) == 1 and calls[0][1]['timeout'] == 7 and not out.exists()


@pytest.mark.parametrize('feature,given,passed_on,limit', [
    ('site_stats', [], [], 240), ('site_stats', ['--kernels'], ['--kernels'], 240), ('waic', [], [], 300), ('regions', ['--kernels'], ['--kernels'], 300),
    ('ppc', [], [], 300), ('spatial', [], [], 300), ('hist', [], ['--bins', '64'], 300), ('conv', [], ['--batch', '44'], 300),
    ('holdout', ['--every', '7'], ['--every', '7'], 300)])
def test_success_appends_one_line_per_size(monkeypatch, tmp_path, capsys, feature, given, passed_on, limit):
    calls = _children(monkeypatch, lambda k: SimpleNamespace(returncode=0, stdout='noise\n{"size": %d}\n' % k))
    out = tmp_path / 'lines.jsonl'
    out.write_text('{"earlier": true}\n')
    tool = load_tool()
    assert tool.main([feature, '--iters', '30', '--out', str(out)] + given) == 0
    assert out.read_text().splitlines() == ['{"earlier": true}', '{"size": 1}', '{"size": 2}']
    assert capsys.readouterr().out.splitlines() == ['{"size": 1}', '{"size": 2}']
    assert tool.SIZES == ((100, 100, 4), (500, 500, 1)) and len(calls) == 2
    for (cmd, kw), size in zip(calls, tool.SIZES):
        assert cmd[1:] == [os.path.join(ROOT, 'tools', 'output_time.py'), feature, '--one'] + [str(v) for v in size] + \
            ['--iters', '30', '--warm', '200', '--reps', '3'] + passed_on
        assert kw['timeout'] == limit and kw['stdout'] == subprocess.PIPE


@pytest.mark.parametrize('feature', list(OPTIONS))
def test_the_default_out_is_the_file_of_the_old_tool(monkeypatch, feature):
    _children(monkeypatch, lambda k: SimpleNamespace(returncode=0, stdout='{}\n'))
    tool = load_tool()
    with mock.patch('builtins.open', mock.mock_open()) as opened:
        assert tool.main([feature]) == 0
    assert [c.args for c in opened.call_args_list] == [(os.path.join(ROOT, 'profiles', feature + '_time.jsonl'), 'a')] * 2


@pytest.mark.parametrize('argv,opt', [(['conv'], 44), (['hist', '--bins', '8'], 8), (['site_stats', '--kernels'], True),
                                      (['ppc'], False), (['spatial'], None)])
def test_a_child_measures_its_size_with_the_options_given(capsys, argv, opt):
    tool = load_tool()
    with mock.patch.object(tool, 'measure', lambda *a: {'args': list(a)}):
        assert tool.main(argv + ['--one', '9', '11', '2', '--reps', '1']) == 0
    assert json.loads(capsys.readouterr().out) == {'args': [argv[0], 9, 11, 2, 2000, 200, 1, opt]}


@pytest.mark.parametrize('feature', list(OPTIONS))
def test_an_option_of_another_feature_is_rejected(monkeypatch, capsys, feature):
    calls = _children(monkeypatch, lambda k: SimpleNamespace(returncode=0, stdout='{}\n'))
    for name, value in (('kernels', []), ('bins', ['8']), ('batch', ['4']), ('every', ['5'])):
        if name != OPTIONS[feature]:
            with pytest.raises(SystemExit) as e:
                load_tool().main([feature, '--' + name] + value)
            assert e.value.code == 2 and 'unrecognized arguments: --' + name in capsys.readouterr().err
    with pytest.raises(SystemExit):
        load_tool().main(['--iters', '5'])      # (no feature)
    assert not calls
