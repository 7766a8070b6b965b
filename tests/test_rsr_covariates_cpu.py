"""LogitRSRGibbs with more than 8 covariates of a kind, through the oracle's build of the C ABI (no GPU): the Python layer
has no cap of its own, so p = 12, q = 10 reach the engine; p = 33 is refused where it always was, when the problem is laid out."""
import numpy as np
import pytest

from .test_cpu_abi import cpu_abi  # noqa: F401  (the oracle's build of the C ABI)


def _problem(p, q):
    from occuspytial_amd.utils import make_lattice_problem
    return make_lattice_problem(17, 19, visits=6, p=p, q=q, random_state=p + q)[:4]


def test_twelve_and_ten_covariates_reach_the_engine(cpu_abi):
    from occuspytial_amd import LogitRSRGibbs
    Q, W, X, y = _problem(12, 10)
    s = LogitRSRGibbs(Q, W, X, y, random_state=7, q=40)
    assert s._problem.rsr['dim'] == 40 and s._problem.p == 12 and s._problem.q == 10
    out = s.sample(30, burnin=5, chains=2, progressbar=False)
    assert out['alpha'].shape == (2, 25, 10) and out['beta'].shape == (2, 25, 12) and out['tau'].shape == (2, 25)
    assert np.all(np.isfinite(out['alpha'])) and np.all(np.isfinite(out['beta'])) and np.all(out['tau'] > 0)
    assert s.state.eta.shape == (40,) and np.allclose(s.state.spatial, s.fixed.K @ s.state.eta, atol=1e-12)
    again = LogitRSRGibbs(Q, W, X, y, random_state=7, q=40).sample(30, burnin=5, chains=2, progressbar=False)
    for k in ('alpha', 'beta', 'tau'):
        assert np.array_equal(out[k], again[k])


def test_thirty_three_covariates_are_refused_with_the_same_text(cpu_abi):
    from occuspytial_amd import LogitRSRGibbs
    Q, W, X, y = _problem(33, 2)
    with pytest.raises(ValueError, match='at most 32 occupancy and 32 detection covariates are supported'):
        LogitRSRGibbs(Q, W, X, y, random_state=7, q=40)
