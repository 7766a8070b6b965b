"""tools/output_time.py on the device: every feature's ``measure`` at 12x15 x 2 chains (both sides at least 8, so that each of
the 64 regions of ``g64`` has a site), 20 timed iterations, a warm-up of 4, one pass per mode, --bins 8, --batch 4, --every 5.
The JSON line has the keys the replaced tool's had (tests/golden/output_time_calls.json), every pass was timed, and what was
read after the feature's last switched-on pass is what the protocol implies: a count is the pass's 20 iterations and the one
kept iteration of the re-warm call ``run(50, 49)`` before them; the draws of a call are those of the timed call alone."""
import json
import math

import pytest

from ._outputs_gpu import time_limit as _time_limit  # noqa: F401 (autouse in this module)
from .test_output_time_cpu import FIXTURE, OPTIONS, load_tool

pytestmark = pytest.mark.gpu
EXTRA = {'hist': 8, 'conv': 4, 'holdout': 5}
IMPLIED = {'site_stats': {'last_count': 21}, 'waic': {'last_count': 21}, 'regions': {'last_rows': [20, 64]},
           'ppc': {'last_rows': [2, 20, 4]}, 'spatial': {'last_rows': [2, 20, 8]}, 'hist': {'last_count': [21, 21]},
           'conv': {'last_count': [21, 21]}, 'holdout': {'last_count': [21, 21]}}
IN_RANGE = {'last_mean_pao': (0.0, 1.0), 'last_p_value': (0.0, 1.0), 'last_width95': (0.0, 1.0), 'last_elpd': (-math.inf, 0.0)}


@pytest.mark.parametrize('feature', list(OPTIONS))
def test_measure_gives_the_line_of_the_old_tool_and_the_state_its_protocol_implies(feature):
    tool = load_tool()
    out = json.loads(json.dumps(tool.measure(feature, 12, 15, 2, iters=20, warm=4, reps=1, opt=EXTRA.get(feature))))
    print(out)
    with open(FIXTURE) as f:
        assert list(out) == [k for k, _ in json.load(f)[feature]['keys']]
    modes = tool.FEATURES[feature].modes
    assert [k for k in out if k.endswith('_us') and isinstance(out[k], list)] == [m + '_us' for m in modes]
    for m in modes:
        assert len(out[m + '_us']) == 1 and math.isfinite(out[m + '_us'][0]) and out[m + '_us'][0] > 0
        assert math.isfinite(out[m + '_median_us']) and out[m + '_median_us'] > 0
    assert (out['shape'], out['n'], out['chains'], out['iters']) == ('12x15', 180, 2, 20)
    for name, value in IMPLIED[feature].items():
        assert out[name] == value, (name, out[name])
    for name, (low, high) in IN_RANGE.items():
        if name in out:
            assert low <= out[name] <= high, (name, out[name])
    if feature == 'holdout':
        assert out['held_out'] == 36 and out['sums_bytes'] == 40 * 36 * 2
