"""ctypes binding of ``libocc_sim.so`` (the C ABI declared in ``include/occ_sim.h``): realisations of the ICAR field
``x ~ N(0, Q^+)`` on the device.  A library of its own, beside ``libocc_gibbs.so`` and ``libocc_basis.so``; it is loaded only
when a field is asked for (:mod:`occuspytial_amd.simulate`).  There is no CPU fallback: a missing library raises
:class:`EngineUnavailable`.
"""
import ctypes as C
import os

import numpy as np
from scipy import sparse

from ._lib import EngineUnavailable

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libocc_sim.so')

VERSION = 1  # OCC_SIM_VERSION of include/occ_sim.h this binding was written against
OK, E_BADARG, E_HIP = 0, -1, -2
MAX_B = 64

_dp = C.c_void_p
# every symbol include/occ_sim.h declares: (name, restype, argtypes)
SYMBOLS = (
    ('occ_sim_version', C.c_int32, []),
    ('occ_sim_last_error', C.c_char_p, [C.c_void_p]),
    ('occ_sim_create', C.c_int, [C.c_int64, _dp, _dp, _dp, _dp, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ('occ_sim_destroy', C.c_int, [C.c_void_p]),
    ('occ_sim_info', C.c_int, [C.c_void_p, _dp]),
    ('occ_sim_draw', C.c_int, [C.c_void_p, C.c_uint64, C.c_int64, C.c_int32]),
    ('occ_sim_solve', C.c_int, [C.c_void_p, C.c_double, C.c_int64, C.c_int32, _dp]),
    ('occ_sim_get', C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32]),
)

_lib = None


def load():
    """Load the shared library and declare its prototypes (no GPU call is made here)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise EngineUnavailable(
                f'{LIB_PATH} is missing: the field simulator has not been built '
                '(run __graft_entry__.build() or `make -C occuspytial_amd/csrc`). There is no CPU fallback for icar_field.')
        lib = C.CDLL(LIB_PATH)
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        if lib.occ_sim_version() != VERSION:
            raise EngineUnavailable(f'{LIB_PATH} has version {lib.occ_sim_version()}, this binding needs {VERSION}: rebuild it '
                                    '(`make -C occuspytial_amd/csrc`)')
        _lib = lib
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class DeviceFieldOps:
    """The ``ops`` of :func:`occuspytial_amd.simulate.icar_field` on the device: one handle of ``libocc_sim.so``.

    ``draw(key, first, b)`` forms the right-hand sides ``u = B'eps`` of the draws ``first .. first + b - 1`` of ``key``,
    ``solve`` turns them into ``x = Q^+ u`` (centred on every component of ``labels``), ``get`` copies ``x`` or ``u`` out.
    ``b_max`` (at most 64) bounds the number of columns: five ``n x b_max`` blocks of doubles are allocated."""

    def __init__(self, Q, labels, b_max, device=0):
        lib = load()
        Qc = sparse.csr_matrix(Q).astype(np.float64)
        Qc.sum_duplicates()
        Qc.sort_indices()
        self.n = Qc.shape[0]
        if Qc.shape != (self.n, self.n):
            raise ValueError('Q must be square')
        if Qc.nnz >= 2 ** 31:
            raise ValueError('Q has too many entries for int32 indices')
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.shape != (self.n,):
            raise ValueError('labels holds one component per site')
        indptr = np.ascontiguousarray(Qc.indptr, dtype=np.int32)
        indices = np.ascontiguousarray(Qc.indices, dtype=np.int32)
        data = np.ascontiguousarray(Qc.data, dtype=np.float64)
        self.b_max = int(b_max)
        self._lib = lib
        self._h = C.c_void_p()
        code = lib.occ_sim_create(self.n, _ptr(indptr), _ptr(indices), _ptr(data), _ptr(labels), self.b_max, int(device), C.byref(self._h))
        if code != OK:
            self._h = C.c_void_p()
            self._raise(code, None)
        self.b = 0

    def _raise(self, code, handle):
        msg = self._lib.occ_sim_last_error(handle)
        text = msg.decode() if msg else ''
        if code == E_BADARG:
            raise ValueError(text or 'bad argument')
        raise EngineUnavailable(f'field simulator failure: {text}')

    def _check(self, code):
        if code != OK:
            self._raise(code, self._h)

    def info(self):
        out = np.zeros(6)
        self._check(self._lib.occ_sim_info(self._h, _ptr(out)))
        return {'ell_w': int(out[0]), 'ld': int(out[1]), 'tiles': int(out[2]), 'components': int(out[3]), 'b': int(out[4]),
                'chunks': int(out[5])}

    def draw(self, key, first, b):
        if not 0 <= int(key) < 2 ** 64:
            raise ValueError('key is a 64-bit word')
        if not -2 ** 63 <= int(first) < 2 ** 63:
            raise ValueError('first + b must not exceed 2^32')
        self._check(self._lib.occ_sim_draw(self._h, int(key), int(first), int(b)))
        self.b = int(b)

    def solve(self, tol=1e-10, max_iter=None, check_every=16):
        """-> ``{'iterations': (b,) int, 'residual': (b,) float}``; ValueError if a column is not done after ``max_iter``."""
        if self.b < 1:
            raise ValueError('no right-hand side has been drawn')
        max_iter = 4 * self.n + 100 if max_iter is None else int(max_iter)
        out = np.zeros(2 * self.b)
        self._check(self._lib.occ_sim_solve(self._h, float(tol), max_iter, int(check_every), _ptr(out)))
        return {'iterations': out[:self.b].astype(np.int64), 'residual': out[self.b:].copy()}

    def get(self, which=0):
        """``x`` (``which=0``) or ``u`` (``which=1``) of the last draw, ``n x b``."""
        if self.b < 1:
            raise ValueError('no right-hand side has been drawn')
        out = np.empty((self.n, self.b))
        self._check(self._lib.occ_sim_get(self._h, int(which), _ptr(out), self.b))
        return out

    def close(self):
        if self._h:
            self._lib.occ_sim_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
