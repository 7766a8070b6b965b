"""The eight optional outputs of ``sample`` and ``resume`` asked for together (``occuspytial_amd/gibbs/options.py``): the draws are
those of a plain call, every output is the one of a call that asks for it alone, and ``resume`` ends where an uninterrupted run
ends.  ``LogitICARGibbs`` on the 30x40 lattice with every fourth site withheld, 3 chains, 7 regions.  Nothing here is
statistical: every comparison is equality."""

import numpy as np
import pytest

from ._outputs_gpu import time_limit as _time_limit  # noqa: F401 (autouse in this module)
from .test_gpu_holdout import _sampler
from .test_gpu_regions import _ids

pytestmark = pytest.mark.gpu

RESULT = dict(site_summaries='sites', waic='waic', regions='regions', ppc='ppc', spatial_check='spatial_check',
              site_intervals='site_intervals', site_diagnostics='site_diagnostics', holdout='holdout')
PER_CALL = ('regions', 'ppc', 'spatial_check')      # rows of the draws a call keeps; the other five accumulate across resume


def _asked(held, diagnostics=True):
    return dict(site_summaries=True, waic=True, regions=_ids(1200, 7), ppc=True, spatial_check=True, site_intervals=True,
                site_diagnostics=diagnostics, holdout=held)


def _arrays(obj, prefix=''):
    """name -> every numpy array in the ``__dict__`` of a result (those inside its dicts too)."""
    out = {}
    for name, value in (obj.items() if isinstance(obj, dict) else vars(obj).items()):
        if isinstance(value, np.ndarray):
            out[prefix + str(name)] = value
        elif isinstance(value, dict):
            out.update(_arrays(value, prefix + str(name) + '.'))
    return out


def _same(a, b, cut=None):
    """Every array of result ``a`` equals the one of ``b`` (NaN at the same places); ``cut``: ``b``'s rows per draw from there on."""
    A, B = _arrays(a), _arrays(b)
    assert A and sorted(A) == sorted(B)
    for name in A:
        want = B[name][:, cut:] if cut and B[name].ndim >= 2 and B[name].shape[:2] == (3, 70) else B[name]   # (90 less the burn-in)
        assert A[name].dtype == want.dtype and np.array_equal(A[name], want, equal_nan=A[name].dtype.kind == 'f'), name


@pytest.fixture(scope='module')
def all8():
    """(the sampler, the withheld data, its sample with all eight asked): chunks of 16, one all burn-in, one that straddles."""
    s, held = _sampler()
    return s, held, s.sample(60, burnin=20, chains=3, progressbar=True, **_asked(held))


def test_the_draws_are_those_of_a_plain_call(all8):
    plain = _sampler()[0].sample(60, burnin=20, chains=3, progressbar=True)
    for name in ('alpha', 'beta', 'tau'):
        assert all8[2][name].shape[:2] == (3, 40) and np.array_equal(all8[2][name], plain[name])
    assert sorted(plain.data) == ['alpha', 'beta', 'tau'] and all(getattr(plain, r) is None for r in RESULT.values())


@pytest.mark.parametrize('keyword', list(RESULT))
def test_every_output_is_the_one_of_a_call_that_asks_for_it_alone(all8, keyword):
    _, held, out = all8
    alone = _sampler()[0].sample(60, burnin=20, chains=3, progressbar=True, **{keyword: _asked(held)[keyword]})
    assert [r for r in RESULT.values() if getattr(alone, r) is not None] == [RESULT[keyword]]
    _same(getattr(out, RESULT[keyword]), getattr(alone, RESULT[keyword]))
    if keyword == 'regions':
        assert out['occupied'].shape == (3, 40, 7) and np.array_equal(out['occupied'], alone['occupied'])
        assert np.array_equal(out.regions.occupied, out['occupied'])
    else:
        assert 'occupied' not in alone.data


def test_resume_ends_where_an_uninterrupted_run_ends(all8):
    """The accumulated outputs are those of 90 iterations; the draws and the rows of a call are its last 30.  The batch length
    of the diagnostics stays the checkpoint's, floor(sqrt(40)) = 6, so the uninterrupted run is given that one."""
    s, held, out = all8
    assert out.site_diagnostics.batch == 6
    ck = s.checkpoint()
    more = s.resume(ck, 30, progressbar=False, **_asked(held))
    longer = _sampler()[0].sample(90, burnin=20, chains=3, progressbar=False, **_asked(held, diagnostics=6))
    for name in ('alpha', 'beta', 'tau', 'occupied'):
        assert more[name].shape[:2] == (3, 30) and np.array_equal(more[name], longer[name][:, 40:])
    for keyword, result in RESULT.items():
        _same(getattr(more, result), getattr(longer, result), cut=40 if keyword in PER_CALL else None)
    assert more.sites.n_draws.tolist() == more.holdout.n_draws.tolist() == more.site_diagnostics.n_draws.tolist() == [70] * 3
    assert more.ppc.ft_obs.shape == more.spatial_check.moran_obs.shape == (3, 30)
