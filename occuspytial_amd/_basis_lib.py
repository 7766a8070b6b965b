"""ctypes binding of ``libocc_basis.so`` (the C ABI declared in ``include/occ_basis.h``): the device primitives that build
the reduced-rank Moran basis.  A library of its own, beside ``libocc_gibbs.so``; it is loaded only when ``basis='device'``
is asked for.  There is no CPU fallback: a missing library raises :class:`EngineUnavailable`.
"""
import ctypes as C
import os

import numpy as np
from scipy import sparse

from ._lib import EngineUnavailable

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libocc_basis.so')

VERSION = 1  # OCC_BASIS_VERSION of include/occ_basis.h this binding was written against
OK, E_BADARG, E_HIP = 0, -1, -2
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
        if not os.path.exists(LIB_PATH):
            raise EngineUnavailable(
                f'{LIB_PATH} is missing: the basis library has not been built '
                "(run __graft_entry__.build() or `make -C occuspytial_amd/csrc`). There is no CPU fallback for basis='device'.")
        lib = C.CDLL(LIB_PATH)
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        if lib.occ_basis_version() != VERSION:
            raise EngineUnavailable(f'{LIB_PATH} has version {lib.occ_basis_version()}, this binding needs {VERSION}: rebuild it '
                                    '(`make -C occuspytial_amd/csrc`)')
        _lib = lib
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def xtx_inverse(X):
    """``(X'X)^-1`` as ``FlatProblem.enable_rsr`` forms it (Cholesky, two triangular solves)."""
    from scipy.linalg import solve_triangular
    chol = np.linalg.cholesky(X.T @ X)
    zi = solve_triangular(chol, np.eye(X.shape[1]), lower=True)
    return np.ascontiguousarray(solve_triangular(chol, zi, lower=True, trans=1))


class DeviceBasisOps:
    """The ``ops`` of :func:`occuspytial_amd.basis.moran_basis` on the device: one handle of ``libocc_basis.so``.

    ``V`` is the handle's block 0; ``filter`` and ``rotate`` replace it, ``gram(1)`` and ``residual`` leave ``Omega V`` in
    block 1.  ``b_max`` bounds the number of columns (three ``n x b_max`` blocks of doubles are allocated)."""

    def __init__(self, Q, X, b_max, device=0):
        lib = load()
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2 or not 1 <= X.shape[1] <= MAX_P:
            raise ValueError(f"basis='device' takes 1 to {MAX_P} occupancy covariates")
        Qc = sparse.csr_matrix(Q).astype(np.float64)
        Qc.sum_duplicates()
        Qc.sort_indices()
        self.n, self.p = X.shape
        if Qc.shape != (self.n, self.n):
            raise ValueError('Q must be n x n with n = X.shape[0]')
        if Qc.nnz >= 2 ** 31:
            raise ValueError('Q has too many entries for int32 indices')
        indptr = np.ascontiguousarray(Qc.indptr, dtype=np.int32)
        indices = np.ascontiguousarray(Qc.indices, dtype=np.int32)
        data = np.ascontiguousarray(Qc.data, dtype=np.float64)
        xi = xtx_inverse(X)
        self.b_max = int(b_max)
        self._lib = lib
        self._h = C.c_void_p()
        code = lib.occ_basis_create(self.n, _ptr(indptr), _ptr(indices), _ptr(data), _ptr(X), self.p, _ptr(xi), self.b_max, int(device),
                                    C.byref(self._h))
        if code != OK:
            self._h = C.c_void_p()
            self._raise(code, None)
        info = self.info()
        self.scale, self.rho, self.ell_w, self.ld = info['s'], info['rho'], info['ell_w'], info['ld']
        self.b = 0

    def _raise(self, code, handle):
        msg = self._lib.occ_basis_last_error(handle)
        text = msg.decode() if msg else ''
        if code == E_BADARG:
            raise ValueError(text or 'bad argument')
        raise EngineUnavailable(f'basis library failure: {text}')

    def _check(self, code):
        if code != OK:
            self._raise(code, self._h)

    def info(self):
        out = np.zeros(6)
        self._check(self._lib.occ_basis_info(self._h, _ptr(out)))
        return {'s': float(out[0]), 'rho': float(out[1]), 'ell_w': int(out[2]), 'ld': int(out[3]), 'b': int(out[4]), 'wmax': int(out[5])}

    def set_block(self, V, which=0):
        V = np.ascontiguousarray(V, dtype=np.float64)
        if V.ndim != 2 or V.shape[0] != self.n:
            raise ValueError('a block is n x b')
        self._check(self._lib.occ_basis_set_block(self._h, which, _ptr(V), V.shape[1]))
        self.b = V.shape[1]

    def get_block(self, which=0):
        V = np.empty((self.n, self.b))
        self._check(self._lib.occ_basis_get_block(self._h, which, _ptr(V), self.b))
        return V

    def apply(self, src=0, dst=1):
        self._check(self._lib.occ_basis_apply(self._h, src, dst))

    def project(self):
        self._check(self._lib.occ_basis_project(self._h))

    def filter(self, degree, lo, hi, top):
        self._check(self._lib.occ_basis_filter(self._h, int(degree), float(lo), float(hi), float(top)))

    def gram(self, which):
        out = np.empty((self.b, self.b))
        self._check(self._lib.occ_basis_gram(self._h, int(which), _ptr(out)))
        return out

    def rotate(self, Y):
        Y = np.ascontiguousarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[0] != self.b:
            raise ValueError('Y must have as many rows as the block has columns')
        self._check(self._lib.occ_basis_rotate(self._h, _ptr(Y), Y.shape[1]))
        self.b = Y.shape[1]

    def residual(self, lam):
        lam = np.ascontiguousarray(lam, dtype=np.float64)
        if lam.shape != (self.b,):
            raise ValueError('one value per column')
        out = np.empty(self.b)
        self._check(self._lib.occ_basis_residual(self._h, _ptr(lam), _ptr(out)))
        return out

    def close(self):
        if self._h:
            self._lib.occ_basis_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
