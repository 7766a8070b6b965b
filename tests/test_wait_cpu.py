"""The host's deadline poll (csrc/occ_wait.hpp) on the CPU, through the stand-alone program occ_wait_check.cpp that
`make wait_check` builds with g++ under AddressSanitizer and UBSan: how OCC_HOST_WAIT_S is read, and the three endings of the
loop -- done, failed with the query's own code, late -- against a scripted query.  The engine's poll_stream and the side
libraries' wait are calls of this loop with hipStreamQuery as the query (600 stands for hipErrorNotReady here).
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'occuspytial_amd', 'csrc')


@pytest.fixture(scope='module')
def wait_check():
    subprocess.run(['make', '-s', '-C', CSRC, 'wait_check'], check=True)
    exe = os.path.join(ROOT, 'build', 'occ_wait_check')

    def run(text, limit=None):
        env = {k: v for k, v in os.environ.items() if k != 'OCC_HOST_WAIT_S'}
        if limit is not None:
            env['OCC_HOST_WAIT_S'] = limit
        r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stderr[-2000:])   # (a sanitizer report ends the program with a non-zero status)
        assert r.stderr == '', r.stderr[-2000:]
        return [ln.split() for ln in r.stdout.splitlines()]
    return run


def test_the_limit_is_read_from_the_environment(wait_check):
    assert wait_check('limit\n') == [['limit', '20']]
    assert wait_check('limit\n', '0.5') == [['limit', '0.5']]
    for bad in ('0', '-3', 'x', ''):
        assert wait_check('limit\n', bad) == [['limit', '20']], bad


def test_done_on_the_first_poll_and_after_a_thousand(wait_check):
    first, later = wait_check('poll 20 0 0 0\npoll 20 1000 0 0\n')
    assert first[:3] == ['done', '0', '1']
    assert later[:3] == ['done', '0', '1001']


@pytest.mark.parametrize('k', [1, 2, 64, 65, 1000])
def test_a_failure_is_handed_back_unchanged_and_is_not_late(wait_check, k):
    """Poll k answers 719 (the others: not ready, for ever): the loop ends there with that code -- also at k = 64, the first poll
    at which the clock is read, with a limit that has long passed by then."""
    for limit in ('20', '1e-9') if k <= 64 else ('20',):
        (got,) = wait_check('poll %s -1 %d 719\n' % (limit, k))
        assert got[:3] == ['failed', '719', str(k)], (limit, got)


def test_never_ready_ends_as_late_once_the_limit_has_passed(wait_check):
    (got,) = wait_check('poll 0.05 -1 0 0\n')
    end, code, polls, sec = got[0], int(got[1]), int(got[2]), float(got[3])
    print('late after', sec, 's and', polls, 'polls')
    assert (end, code) == ('late', 600)
    assert polls % 64 == 0                                    # the clock is read every 64th poll
    assert 0.05 <= sec < 2.0                                  # (2 s only keeps the test from hanging: a condition, not a measurement)
