"""Spatial residual check: Moran's I of the occupancy residuals from the rows the engine records per draw (``Engine.moran_draws``)."""
import numpy as np

from .ppc import tail_probability

N_COLUMNS = 8   # per kept draw: A, B, C, D of the residuals z - psi, then of their replicate z* - psi


def spatial_flag(v):
    """The ``spatial_check=`` argument of ``sample`` / ``resume`` as a bool; anything but ``True`` / ``False`` is a ``ValueError``."""
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    raise ValueError('spatial_check must be True or False, not %r' % (v,))


def weights_total(Q):
    """``S0``: the sum of the weights ``w_ij = -Q_ij`` over the off-diagonals of a sparse (or dense) precision matrix."""
    if hasattr(Q, 'diagonal') and hasattr(Q, 'sum'):
        return float(Q.diagonal().sum() - Q.sum())
    Q = np.asarray(Q, dtype=np.float64)
    return float(np.trace(Q) - Q.sum())


def moran_from_sums(A, B, C, D, n, S0):
    r"""Moran's I of a vector r, centred at its mean, from the four sums the device forms:
    :math:`A = \sum_i r_i \sum_j w_{ij} r_j`, :math:`B = \sum_i d_i r_i` (:math:`d_i = \sum_j w_{ij}`), :math:`C = \sum_i r_i`,
    :math:`D = \sum_i r_i^2`; with :math:`\bar r = C/n`,

    .. math:: I = \frac{n}{S_0}\,\frac{A - 2\bar r B + \bar r^2 S_0}{D - n\bar r^2}.

    (Symmetric weights: :math:`\sum_i \sum_j w_{ij} r_j = \sum_j d_j r_j = B`.)"""
    A, B, C, D = (np.asarray(v, dtype=np.float64) for v in (A, B, C, D))
    rbar = C / n
    with np.errstate(divide='ignore', invalid='ignore'):
        return (n / S0) * (A - 2.0 * rbar * B + rbar * rbar * S0) / (D - n * rbar * rbar)


class SpatialCheck:
    r"""Did the spatial term absorb the spatial structure?  Moran's I of the occupancy residuals against its posterior
    predictive distribution.

    Per kept draw, with :math:`\psi_i = \mathrm{expit}(x_i^\top\beta + \eta_i)`, the engine forms the sums of Moran's I
    (weights :math:`w_{ij} = -Q_{ij}`) of :math:`r = z - \psi` and of one replicate :math:`r^* = z^* - \psi`,
    :math:`z^*_i \sim \mathrm{Bernoulli}(\psi_i)`.  Residuals that are still positively autocorrelated give observed values
    above the replicated ones.

    ``SpatialCheck(rows, n, S0)``: ``rows`` is ``(chains, draws, 8)`` as ``Engine.moran_draws`` gives them, ``n`` the number
    of sites and ``S0`` the sum of the weights.

    * ``moran_obs``, ``moran_rep`` -- ``(chains, draws)`` Moran's I of the residuals and of their replicate;
    * ``expected`` -- ``-1 / (n - 1)``, the value under no autocorrelation;
    * ``p_value`` -- :math:`(\#\{I_{rep} > I_{obs}\} + \tfrac12 \#\{=\}) / N`, pooled over chains: near 0 the residuals are
      more autocorrelated than the model says they should be;
    * ``excess`` -- ``mean(moran_obs) - mean(moran_rep)``;
    * ``n_draws`` -- ``chains * draws``.
    """

    def __init__(self, rows, n, S0):
        rows = np.asarray(rows, dtype=np.float64)
        if rows.ndim != 3 or rows.shape[2] != N_COLUMNS:
            raise ValueError('rows must be (chains, draws, %d)' % N_COLUMNS)
        self.n = int(n)
        self.S0 = float(S0)
        self.moran_obs = moran_from_sums(rows[:, :, 0], rows[:, :, 1], rows[:, :, 2], rows[:, :, 3], self.n, self.S0)
        self.moran_rep = moran_from_sums(rows[:, :, 4], rows[:, :, 5], rows[:, :, 6], rows[:, :, 7], self.n, self.S0)

    @classmethod
    def from_problem(cls, problem, rows):
        """With the number of sites and the weights of a ``FlatProblem``."""
        return cls(rows, problem.n, weights_total(problem.Q))

    @property
    def expected(self):
        return -1.0 / (self.n - 1)

    @property
    def n_draws(self):
        return int(self.moran_obs.size)

    @property
    def p_value(self):
        return tail_probability(self.moran_rep, self.moran_obs)

    @property
    def excess(self):
        if self.n_draws == 0:
            return float('nan')
        return float(np.mean(self.moran_obs) - np.mean(self.moran_rep))

    def __repr__(self):
        return (f'SpatialCheck(chains={self.moran_obs.shape[0]}, draws={self.moran_obs.shape[1]}, '
                f'p_value={self.p_value:.3f}, excess={self.excess:.4f})')
