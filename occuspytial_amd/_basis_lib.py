"""ctypes binding of ``libocc_basis.so`` (the C ABI declared in ``include/occ_basis.h``): the device primitives that build
the reduced-rank Moran basis.  A library of its own, beside ``libocc_gibbs.so``; it is loaded only when ``basis='device'``
is asked for.  There is no CPU fallback: a missing library raises :class:`EngineUnavailable`.
"""
import ctypes as C
import os

import numpy as np

from ._native import NativeHandle, csr_arrays, load_library, ptr

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libocc_basis.so')

VERSION = 1  # OCC_BASIS_VERSION of include/occ_basis.h this binding was written against
MAX_P = 32

_dp = C.c_void_p
# every symbol include/occ_basis.h declares: (name, restype, argtypes)
SYMBOLS = (
    ('occ_basis_version', C.c_int32, []),
    ('occ_basis_last_error', C.c_char_p, [C.c_void_p]),
    ('occ_basis_create', C.c_int, [C.c_int64, _dp, _dp, _dp, _dp, C.c_int32, _dp, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    ('occ_basis_destroy', C.c_int, [C.c_void_p]),
    ('occ_basis_info', C.c_int, [C.c_void_p, _dp]),
    ('occ_basis_set_block', C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32]),
    ('occ_basis_get_block', C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32]),
    ('occ_basis_apply', C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    ('occ_basis_project', C.c_int, [C.c_void_p]),
    ('occ_basis_filter', C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double]),
    ('occ_basis_gram', C.c_int, [C.c_void_p, C.c_int32, _dp]),
    ('occ_basis_rotate', C.c_int, [C.c_void_p, _dp, C.c_int32]),
    ('occ_basis_residual', C.c_int, [C.c_void_p, _dp, _dp]),
)

_lib = None


def load():
    """Load the shared library and declare its prototypes (no GPU call is made here)."""
    global _lib
    if _lib is None:
        _lib = load_library(LIB_PATH, SYMBOLS, 'occ_basis_version', VERSION, 'the basis library', "basis='device'")
    return _lib


def xtx_inverse(X):
    """``(X'X)^-1`` as ``FlatProblem.enable_rsr`` forms it (Cholesky, two triangular solves)."""
    from scipy.linalg import solve_triangular
    chol = np.linalg.cholesky(X.T @ X)
    zi = solve_triangular(chol, np.eye(X.shape[1]), lower=True)
    return np.ascontiguousarray(solve_triangular(chol, zi, lower=True, trans=1))


class DeviceBasisOps(NativeHandle):
    """The ``ops`` of :func:`occuspytial_amd.basis.moran_basis` on the device: one handle of ``libocc_basis.so``.

    ``V`` is the handle's block 0; ``filter`` and ``rotate`` replace it, ``gram(1)`` and ``residual`` leave ``Omega V`` in
    block 1.  ``b_max`` bounds the number of columns (three ``n x b_max`` blocks of doubles are allocated)."""

    _LAST_ERROR, _DESTROY, _NOUN = 'occ_basis_last_error', 'occ_basis_destroy', 'basis library'

    def __init__(self, Q, X, b_max, device=0):
        lib = load()
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2 or not 1 <= X.shape[1] <= MAX_P:
            raise ValueError(f"basis='device' takes 1 to {MAX_P} occupancy covariates")
        self.n, self.p = X.shape
        _, indptr, indices, data = csr_arrays(Q, self.n)
        xi = xtx_inverse(X)
        self.b_max = int(b_max)
        self._lib = lib
        self._h = C.c_void_p()
        self._created(lib.occ_basis_create(self.n, ptr(indptr), ptr(indices), ptr(data), ptr(X), self.p, ptr(xi), self.b_max, int(device),
                                           C.byref(self._h)))
        info = self.info()
        self.scale, self.rho, self.ell_w, self.ld = info['s'], info['rho'], info['ell_w'], info['ld']
        self.b = 0

    def info(self):
        out = np.zeros(6)
        self._check(self._lib.occ_basis_info(self._h, ptr(out)))
        return {'s': float(out[0]), 'rho': float(out[1]), 'ell_w': int(out[2]), 'ld': int(out[3]), 'b': int(out[4]), 'wmax': int(out[5])}

    def set_block(self, V, which=0):
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.ndim != 2 or V.shape[0] != self.n:
            raise ValueError('a block is n x b')
        self._check(self._lib.occ_basis_set_block(self._h, which, ptr(V), V.shape[1]))
        self.b = V.shape[1]

    def get_block(self, which=0):
        V = np.empty((self.n, self.b))
        self._check(self._lib.occ_basis_get_block(self._h, which, ptr(V), self.b))
        return V

    def apply(self, src=0, dst=1):
        self._check(self._lib.occ_basis_apply(self._h, src, dst))

    def project(self):
        self._check(self._lib.occ_basis_project(self._h))

    def filter(self, degree, lo, hi, top):
        self._check(self._lib.occ_basis_filter(self._h, int(degree), float(lo), float(hi), float(top)))

    def gram(self, which):
        out = np.empty((self.b, self.b))
        self._check(self._lib.occ_basis_gram(self._h, int(which), ptr(out)))
        return out

    def rotate(self, Y):
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[0] != self.b:
            raise ValueError('Y must have as many rows as the block has columns')
        self._check(self._lib.occ_basis_rotate(self._h, ptr(Y), Y.shape[1]))
        self.b = Y.shape[1]

    def residual(self, lam):
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        if lam.shape != (self.b,):
            raise ValueError('one value per column')
        out = np.empty(self.b)
        self._check(self._lib.occ_basis_residual(self._h, ptr(lam), ptr(out)))
        return out
