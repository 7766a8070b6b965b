"""The graph of a spatial precision: its connected components.

An ICAR precision ``Q = D - W`` of a map with islands, habitat fragments or isolated cells has one zero eigenvalue per
connected component.  ``LogitICARGibbs(..., constraint='component')`` centres the spatial effect on every component
("Sum-to-zero per connected component"); this module finds them.
"""
import numpy as np
from scipy import sparse
from scipy.sparse.csgraph import connected_components

CONSTRAINTS = ('global', 'component')


def components(Q):
    """``(k, labels)``: the number of connected components of the graph of ``Q`` and the component of every site.

    Two sites are neighbours where ``Q`` has a non-zero off-diagonal entry (stored zeros and the diagonal do not count; the
    pattern is read as undirected).  ``labels`` is int32 in ``[0, k)``, numbered by each component's lowest site: site 0 is
    in component 0, the lowest site outside it in component 1, and so on.  A site without neighbours is a component of its own.

    With ``k <= 256`` the labels are a valid ``sample(..., regions=labels)``: the occupied sites per component -- occupancy
    per island -- then come with every kept draw, for nothing more than the keyword.
    """
    A = sparse.csr_matrix(Q).astype(np.float64).tocoo()
    off = (A.row != A.col) & (A.data != 0)
    n = A.shape[0]
    pattern = sparse.csr_matrix((np.ones(int(off.sum())), (A.row[off], A.col[off])), shape=(n, n))
    k, raw = connected_components(pattern, directed=False)
    # number by lowest site: the first appearance of every raw label, in site order
    _, first = np.unique(raw, return_index=True)
    rank = np.empty(k, dtype=np.int64)
    rank[np.argsort(first, kind='stable')] = np.arange(k)
    return int(k), rank[raw].astype(np.int32)


def scale(Q, draws=1024, random_state=None, device=0, field=None):
    """``(Q_scaled, factors)``: the ICAR precision scaled so that ``tau`` has a size-free meaning (Sorbye & Rue 2014; per
    connected component as Freni-Sterrantino et al. 2018 recommend).

    Every component ``k`` of two or more sites has its block of ``Q`` multiplied by
    ``c_k = exp(mean_i log var_i - (psi(nu / 2) - log(nu / 2)))``, ``var`` the marginal variances ``diag(Q^+)`` estimated from
    ``nu = draws`` device-drawn fields (:func:`occuspytial_amd.simulate.marginal_variance`); the subtracted term is the exact
    bias of the logarithm of a chi-square(nu) / nu variate.  Under ``Q_scaled`` the geometric mean of the marginal variances
    is 1 on every such component.  Singletons are untouched (factor 1).  ``Q_scaled`` is CSR and still an ICAR precision:
    it goes straight into the samplers.  ``field`` replaces ``icar_field`` as in ``marginal_variance``.
    """
    from scipy.special import digamma

    from .simulate import marginal_variance
    Qc = sparse.csr_matrix(Q).astype(np.float64)
    var, nu = marginal_variance(Qc, draws=draws, random_state=random_state, device=device, field=field)
    k, labels = components(Qc)
    size = np.bincount(labels, minlength=k)
    many = size[labels] > 1
    if np.any(var[many] <= 0):
        raise ValueError('a site with neighbours has no variance: too few draws')
    logv = np.where(many, np.log(np.where(many, var, 1.0)), 0.0)
    factors = np.exp(np.bincount(labels, weights=logv, minlength=k) / size - (digamma(0.5 * nu) - np.log(0.5 * nu)))
    factors[size == 1] = 1.0
    Qs = sparse.csr_matrix(sparse.diags(factors[labels]) @ Qc)
    return Qs, factors


def centre(eta, labels):
    """``eta`` minus the mean of its component at every site (a site alone in its component: exactly 0.0)."""
    eta = np.asarray(eta, dtype=np.float64)
    labels = np.asarray(labels)
    size = np.bincount(labels)
    mean = np.bincount(labels, weights=eta) / size
    out = eta - mean[labels]
    out[size[labels] == 1] = 0.0
    return out
