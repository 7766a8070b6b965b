"""Posterior predictive check of the detection histories from the rows the engine records per draw (``Engine.ppc_draws``)."""
import numpy as np

N_COLUMNS = 4   # per kept draw: T_obs, T_rep (Freeman-Tukey), replicated detections, replicated sites with a detection


def ppc_flag(ppc):
    """The ``ppc=`` argument of ``sample`` / ``resume`` as a bool; anything but ``True`` / ``False`` is a ``ValueError``."""
    if isinstance(ppc, (bool, np.bool_)):
        return bool(ppc)
    raise ValueError('ppc must be True or False, not %r' % (ppc,))


def tail_probability(rep, obs):
    r"""``(#{rep > obs} + #{rep == obs} / 2) / N`` over all entries: the Bayesian p-value with ties counted half."""
    rep = np.asarray(rep, dtype=np.float64)
    obs = np.broadcast_to(np.asarray(obs, dtype=np.float64), rep.shape)
    if rep.size == 0:
        return float('nan')
    return float((np.count_nonzero(rep > obs) + 0.5 * np.count_nonzero(rep == obs)) / rep.size)


class PredictiveCheck:
    r"""Posterior predictive check of an occupancy model's detection histories (Kery and Royle), conditional on z.

    Per kept draw the engine replicates every surveyed site's detections from the draw's :math:`(z, \alpha)`:
    :math:`y^*_{ir} \sim \mathrm{Bernoulli}(z_i\,\mathrm{expit}(w_r^\top\alpha))`.  With :math:`y_i` and :math:`y^*_i` a site's
    observed and replicated detections and :math:`E_i = z_i \sum_r \mathrm{expit}(w_r^\top\alpha)`, the Freeman-Tukey
    discrepancies are :math:`T_{obs} = \sum_i (\sqrt{y_i} - \sqrt{E_i})^2` and
    :math:`T_{rep} = \sum_i (\sqrt{y^*_i} - \sqrt{E_i})^2`.

    ``PredictiveCheck(rows, detections, sites_detected)``: ``rows`` is ``(chains, draws, 4)`` as ``Engine.ppc_draws``
    gives them, ``detections`` the observed :math:`\sum y` and ``sites_detected`` the observed sites with a detection.

    * ``ft_obs``, ``ft_rep`` -- ``(chains, draws)`` the two discrepancies;
    * ``detections_rep``, ``sites_detected_rep`` -- ``(chains, draws)`` replicated detections and replicated sites with one;
    * ``detections``, ``sites_detected`` -- their observed counterparts, constants;
    * ``p_value`` -- :math:`(\#\{T_{rep} > T_{obs}\} + \tfrac12 \#\{=\}) / N`, pooled over chains: near 0 or 1 the model
      does not reproduce the data;
    * ``c_hat`` -- ``mean(ft_obs) / mean(ft_rep)``, the lack-of-fit ratio (1: as dispersed as the model says);
    * ``p_detections``, ``p_sites_detected`` -- the same tail probability of the two integer statistics against their
      observed constants;
    * ``n_draws`` -- ``chains * draws``.
    """

    def __init__(self, rows, detections, sites_detected):
        rows = np.asarray(rows, dtype=np.float64)
        if rows.ndim != 3 or rows.shape[2] != N_COLUMNS:
            raise ValueError('rows must be (chains, draws, %d)' % N_COLUMNS)
        self.ft_obs = rows[:, :, 0].copy()
        self.ft_rep = rows[:, :, 1].copy()
        self.detections_rep = rows[:, :, 2].copy()
        self.sites_detected_rep = rows[:, :, 3].copy()
        self.detections = int(detections)
        self.sites_detected = int(sites_detected)

    @classmethod
    def from_problem(cls, problem, rows):
        """With the observed constants of a ``FlatProblem``."""
        return cls(rows, int(np.count_nonzero(problem.y)), int(np.count_nonzero(problem.obs_site)))

    @property
    def n_draws(self):
        return int(self.ft_obs.size)

    @property
    def p_value(self):
        return tail_probability(self.ft_rep, self.ft_obs)

    @property
    def c_hat(self):
        if self.n_draws == 0:
            return float('nan')
        with np.errstate(divide='ignore', invalid='ignore'):
            return float(np.mean(self.ft_obs) / np.mean(self.ft_rep))

    @property
    def p_detections(self):
        return tail_probability(self.detections_rep, self.detections)

    @property
    def p_sites_detected(self):
        return tail_probability(self.sites_detected_rep, self.sites_detected)

    def __repr__(self):
        return (f'PredictiveCheck(chains={self.ft_obs.shape[0]}, draws={self.ft_obs.shape[1]}, '
                f'p_value={self.p_value:.3f}, c_hat={self.c_hat:.3f})')
