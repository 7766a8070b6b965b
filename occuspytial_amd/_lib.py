"""ctypes binding of ``libocc_gibbs.so`` (the C ABI declared in ``include/occ_gibbs.h``).

There is no CPU fallback: if the shared library is missing, or no MI355X is usable, every entry
point that would compute raises.  Build the library with ``python -c "import __graft_entry__ as g;
g.build()"`` or ``make -C occuspytial_amd/csrc``.
"""
import ctypes as C
import os
from typing import NamedTuple

from ._native import EngineUnavailable, load_library  # noqa: F401  (EngineUnavailable: the name its users import from here)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libocc_gibbs.so')

OCC_OK = 0
OCC_E_BADARG, OCC_E_HIP, OCC_E_MINRES, OCC_E_CHOLESKY, OCC_E_STATE = -1, -2, -3, -4, -5
N_KERNEL_KINDS = 9
# state names of the per-site posterior sums (occ_get_state / occ_set_state, see the header): the chain's switch, its count
# of accumulated iterations, and the five sums of length n
SITE_FIELDS = ('site_stats', 'site_count', 'site_psi', 'site_occ', 'site_z', 'site_eta', 'site_eta2')
# likewise the per-site log-likelihood sums of streaming WAIC: switch, count, and the three sums of length n
LOGLIK_FIELDS = ('ll_stats', 'll_count', 'll_lik', 'll_log', 'll_log2')
# per-site intervals: the chain's switch (a word of the handle: 0 off, B on with B bins), its count of accumulated iterations,
# its histograms of psi (B n, bin-major)
HIST_FIELDS = ('hist_stats', 'hist_count', 'hist_counts')
# per-site convergence diagnostics: the chain's switch (a word of the handle: 0 off, L on with batch length L), its count of
# accumulated iterations, its batch-means sums (11 n, slot-major: cnt, then ref, s1, s2, run, bsq of psi, then of eta)
CONV_FIELDS = ('conv_stats', 'conv_count', 'conv_sums')
# held-out predictive scoring: the handle's withheld data (packed: H, R, site[H], ptr[H + 1], y[R], W[R q] row-major), the
# chain's switch (a word of the handle, 0 or 1), its count of accumulated iterations, its sums (5 H, slot-major: cnt, the sums
# of L, of l, of l^2 and of pd)
HOLDOUT_FIELDS = ('holdout_data', 'holdout_stats', 'holdout_count', 'holdout_sums')
KERNEL_KINDS = ('omega_b', 'noise', 'eta_init', 'minres', 'beta_partial', 'omega_a', 'alpha_draw', 'z_ob', 'iter')


class StateName(NamedTuple):
    """One plain state name of a chain (``STATE`` of csrc/occ_names.hpp), as Python sees it."""
    unit: str           # its length: '1', 'n', 'S', 'R', 'p', 'q', 'm', '2n' or 'm*m'
    read: int           # the models that answer a read ...
    write: int          # ... and that accept a write: a mask over ICAR, RSR, PROBIT
    prologue: bool      # a write on a logit handle makes the next call redraw omega_b
    ckpt: int           # the models whose checkpoint holds it (``Engine.checkpoint``, in this order)


ICAR, RSR, PROBIT = 1, 2, 4
_LOGIT, _ALL = ICAR | RSR, ICAR | RSR | PROBIT
STATE_NAMES = {
    'alpha': StateName('q', _ALL, _ALL, True, _ALL),
    'beta': StateName('p', _ALL, _ALL, True, _ALL),
    'tau': StateName('1', _ALL, _ALL, True, _ALL),
    'eta': StateName('n', _ALL, _ALL, True, ICAR | PROBIT),
    'theta': StateName('m', RSR | PROBIT, RSR | PROBIT, True, RSR | PROBIT),
    'z': StateName('n', _ALL, _ALL, True, _ALL),
    'xz': StateName('2n', _LOGIT, _LOGIT, True, ICAR),
    'c': StateName('m', PROBIT, PROBIT, False, PROBIT),
    'eps': StateName('n', PROBIT, PROBIT, False, PROBIT),
    'iter': StateName('1', _ALL, _ALL, True, 0),
    'k': StateName('n', _ALL, 0, False, 0),
    'exists': StateName('S', _ALL, 0, False, 0),
    'omega_a': StateName('R', _ALL, _ALL, True, 0),
    'omega_b': StateName('n', _ALL, 0, False, 0),
    'rhs': StateName('n', _LOGIT, 0, False, 0),
    'minres_itn': StateName('1', _LOGIT, 0, False, 0),
    'rsr_gram': StateName('m*m', RSR, 0, False, 0),
    'link': StateName('1', PROBIT, 0, False, 0),
    'debug_close_window': StateName('1', 0, _LOGIT, False, 0),
    'debug_maxiter': StateName('1', 0, _LOGIT, True, 0),
}


class SumsKind(NamedTuple):
    """One kind of per-site running sums the engine keeps on the device (``SUMS`` of csrc/occ_names.hpp), as Python sees it."""
    fields: tuple       # its state names: switch, count, sums (a sum's short name drops the kind's prefix, 'site_' / 'll_')
    what: str           # what messages call it


# (what the samplers make of a kind -- keyword, result, refusals -- is its row of gibbs/options.py)
SUMS_KINDS = {'site': SumsKind(SITE_FIELDS, 'site summaries'), 'll': SumsKind(LOGLIK_FIELDS, 'log-likelihood sums')}


class AccumKind(NamedTuple):
    """One accumulator the engine keeps behind the z update (``ACCUM`` of csrc/occ_accum.hpp), as Python sees it.  ``Engine`` has
    a method by the name of the switch and, where there is one, of the input."""
    fields: tuple       # its state names: (the handle's input first, if it needs one,) switch, count, data
    on: str             # the attribute of ``Engine`` that holds the switch's value while on (bins, batch length, True), else 0
    slots: int          # arrays per chain on the device
    dtype: str          # of a chain's data as Python returns and checkpoints them (the count: int64)
    shape: tuple        # ... and their shape; 'n': the problem's sites

    @property
    def input(self):
        return self.fields[0] if len(self.fields) == 4 else None


ACCUM_KINDS = {
    'hist': AccumKind(HIST_FIELDS, '_hist_bins', 1, 'uint32', (-1, 'n')),       # (B, n)
    'conv': AccumKind(CONV_FIELDS, '_conv_batch', 11, 'float64', (11, -1)),     # (11, n)
    'holdout': AccumKind(HOLDOUT_FIELDS, '_holdout_on', 5, 'float64', (5, -1)),  # (5, H)
}


class DrawsKind(NamedTuple):
    """One kind of draws of a call (``DRAWS`` of csrc/occ_draws.hpp), as Python sees it.  ``Engine`` has a method by the name of
    the switch and of the rows."""
    fields: tuple       # its state names: (the handle's input first, if it needs one,) switch, rows
    on: str             # the attribute of ``Engine`` that holds the switch
    width: int          # numbers per row; None: set by the input

    @property
    def input(self):
        return self.fields[0] if len(self.fields) == 3 else None


DRAWS_KINDS = {
    # the occupied sites per region and draw: the handle's map (n), the chain's switch, its counts of the last occ_run (keep G)
    'region': DrawsKind(('region_id', 'region_stats', 'region_draws'), '_region_on', None),
    # the posterior predictive check: T_obs, T_rep, the replicated detections, the replicated sites with a detection
    'ppc': DrawsKind(('ppc_stats', 'ppc_draws'), '_ppc_on', 4),
    # the spatial residual check: the sums A, B, C, D of Moran's I of z - psi, then those of its replicate
    'moran': DrawsKind(('moran_stats', 'moran_draws'), '_moran_on', 8),
}
REGION_FIELDS, PPC_FIELDS, MORAN_FIELDS = (k.fields for k in DRAWS_KINDS.values())   # (the names the tests know them by)


class OccProblem(C.Structure):
    _fields_ = [
        ('n', C.c_int64), ('n_surveyed', C.c_int64), ('n_rows', C.c_int64),
        ('p', C.c_int32), ('q', C.c_int32),
        ('q_indptr', C.c_void_p), ('q_indices', C.c_void_p), ('q_data', C.c_void_p),
        ('X', C.c_void_p), ('site_id', C.c_void_p), ('site_ptr', C.c_void_p),
        ('W', C.c_void_p), ('y', C.c_void_p),
        ('a_mu', C.c_void_p), ('a_prec', C.c_void_p), ('b_mu', C.c_void_p), ('b_prec', C.c_void_p),
        ('tau_rate', C.c_double), ('tau_shape', C.c_double),
        ('rsr_dim', C.c_int32), ('rsr_K', C.c_void_p), ('rsr_Q', C.c_void_p), ('rsr_E', C.c_void_p),
        ('prior_factor', C.c_void_p), ('prior_factor_cols', C.c_int64),
        ('link', C.c_int32), ('pb_Phi', C.c_void_p), ('pb_G', C.c_void_p), ('pb_lam', C.c_void_p),   # ABI 7
    ]


class OccStats(C.Structure):
    _fields_ = [
        ('iterations', C.c_int64), ('graph_launches', C.c_int64), ('eager_iterations', C.c_int64),
        ('stalls', C.c_int64), ('krylov_cap', C.c_int32), ('krylov_last', C.c_int32),
        ('krylov_mean', C.c_double), ('krylov_total', C.c_int64), ('solves', C.c_int64), ('last_run_ms', C.c_double),
        ('n_blocks_sites', C.c_int32), ('n_blocks_rows', C.c_int32), ('threads_per_block', C.c_int32),
        ('n_chains', C.c_int32), ('persistent_solve', C.c_int32), ('solve_workgroups', C.c_int32),
        ('main_stream_cus', C.c_int32), ('fused_fallbacks', C.c_int32), ('profile_minres_iterations', C.c_double),
        ('iter_kernel_launches', C.c_int64), ('iter_kernel_mean_us', C.c_double),
        ('repromotions', C.c_int32), ('stream_probes', C.c_int32), ('handover_mode', C.c_int32),
        ('stream_pairs_masked', C.c_int32), ('stream_pairs_plain', C.c_int32), ('demoted', C.c_int32),
        ('profile_iter_dispatch_us', C.c_double),
        ('stream_pairs_idle', C.c_int32), ('stream_pairs_evicted', C.c_int32),
    ]


# every symbol include/occ_gibbs.h declares: (name, restype, argtypes)
SYMBOLS = (
    ('occ_abi_version', C.c_int32, []),
    ('occ_device_count', C.c_int32, []),
    ('occ_last_error', C.c_char_p, [C.c_void_p]),
    ('occ_create', C.c_int, [C.POINTER(OccProblem), C.c_int32, C.POINTER(C.c_uint64), C.c_int32,
                             C.POINTER(C.c_void_p)]),
    ('occ_destroy', C.c_int, [C.c_void_p]),
    ('occ_set_keys', C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ('occ_set_start', C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    ('occ_step', C.c_int, [C.c_void_p]),
    ('occ_run', C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('occ_get_state', C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_void_p, C.c_int64,
                                C.POINTER(C.c_int64)]),
    ('occ_set_state', C.c_int, [C.c_void_p, C.c_int32, C.c_char_p, C.c_void_p, C.c_int64]),
    ('occ_get_stats', C.c_int, [C.c_void_p, C.POINTER(OccStats)]),
    ('occ_profile', C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    ('occ_create_group', C.c_int, [C.POINTER(OccProblem), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)]),
    ('occ_comm_unique_id', C.c_int, [C.c_void_p]),
    ('occ_comm_create', C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    ('occ_comm_destroy', C.c_int, [C.c_void_p]),
    ('occ_comm_barrier', C.c_int, [C.c_void_p]),
    ('occ_comm_allreduce_max', C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    ('occ_comm_broadcast_host', C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]),
    ('occ_comm_last_error', C.c_char_p, [C.c_void_p]),
    ('occ_create_distributed', C.c_int, [C.POINTER(OccProblem), C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_void_p)]),
    ('occ_group_transport', C.c_char_p, [C.c_void_p]),
    ('occ_synchronize', C.c_int, [C.c_void_p]),
    ('occ_cond_tau', C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.POINTER(C.c_double)]),
    ('occ_cond_eta', C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_int32)]),
    ('occ_cond_beta', C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('occ_cond_alpha', C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ('occ_cond_z', C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    ('occ_draw', C.c_int, [C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p]),
)

_lib = None
ABI_VERSION = 7  # OCC_ABI_VERSION of include/occ_gibbs.h this binding was written against


def load():
    """Load the shared library and declare its prototypes (no GPU call is made here)."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS, 'occ_abi_version', ABI_VERSION, 'the HIP engine', version_noun='ABI version')
    return _lib


def error_text(handle=None):
    msg = load().occ_last_error(handle)
    return msg.decode() if msg else ''


def raise_for(code, handle=None):
    """Map a status code to the exception the reference raises for the same condition."""
    if code == OCC_OK:
        return
    text = error_text(handle)
    if code in (OCC_E_BADARG, OCC_E_STATE):
        raise ValueError(text or 'bad argument')
    if code == OCC_E_MINRES:
        raise RuntimeError('MINRES solver did not converge!')          # reference logit.py:91-92
    if code == OCC_E_CHOLESKY:
        raise RuntimeError('Cholesky factorization/solver failed!')    # reference distributions.pyx:21
    raise EngineUnavailable(f'HIP engine failure: {text}')
