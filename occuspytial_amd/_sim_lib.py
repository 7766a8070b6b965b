"""ctypes binding of ``libocc_sim.so`` (the C ABI declared in ``include/occ_sim.h``): realisations of the ICAR field
``x ~ N(0, Q^+)`` on the device.  A library of its own, beside ``libocc_gibbs.so`` and ``libocc_basis.so``; it is loaded only
when a field is asked for (:mod:`occuspytial_amd.simulate`).  There is no CPU fallback: a missing library raises
:class:`EngineUnavailable`.
"""
import ctypes as C
import os

import numpy as np

from ._native import NativeHandle, csr_arrays, load_library, ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libocc_sim.so')

VERSION = 1  # OCC_SIM_VERSION of include/occ_sim.h this binding was written against
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
        _lib = load_library(LIB_PATH, SYMBOLS, 'occ_sim_version', VERSION, 'the field simulator', 'icar_field')
    return _lib


class DeviceFieldOps(NativeHandle):
    """The ``ops`` of :func:`occuspytial_amd.simulate.icar_field` on the device: one handle of ``libocc_sim.so``.

    ``draw(key, first, b)`` forms the right-hand sides ``u = B'eps`` of the draws ``first .. first + b - 1`` of ``key``,
    ``solve`` turns them into ``x = Q^+ u`` (centred on every component of ``labels``), ``get`` copies ``x`` or ``u`` out.
    ``b_max`` (at most 64) bounds the number of columns: five ``n x b_max`` blocks of doubles are allocated."""

    _LAST_ERROR, _DESTROY, _NOUN = 'occ_sim_last_error', 'occ_sim_destroy', 'field simulator'

    def __init__(self, Q, labels, b_max, device=0):
        lib = load()
        self.n, indptr, indices, data = csr_arrays(Q)
        labels = np.ascontiguousarray(labels, dtype=np.int32)
        if labels.shape != (self.n,):
            raise ValueError('labels holds one component per site')
        self.b_max = int(b_max)
        self._lib = lib
        self._h = C.c_void_p()
        self._created(lib.occ_sim_create(self.n, ptr(indptr), ptr(indices), ptr(data), ptr(labels), self.b_max, int(device), C.byref(self._h)))
        self.b = 0

    def info(self):
        out = np.zeros(6)
        self._check(self._lib.occ_sim_info(self._h, ptr(out)))
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
        self._check(self._lib.occ_sim_solve(self._h, float(tol), max_iter, int(check_every), ptr(out)))
        return {'iterations': out[:self.b].astype(np.int64), 'residual': out[self.b:].copy()}

    def get(self, which=0):
        """``x`` (``which=0``) or ``u`` (``which=1``) of the last draw, ``n x b``."""
        if self.b < 1:
            raise ValueError('no right-hand side has been drawn')
        out = np.empty((self.n, self.b))
        self._check(self._lib.occ_sim_get(self._h, int(which), ptr(out), self.b))
        return out
