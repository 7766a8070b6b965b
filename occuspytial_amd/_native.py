"""What the ctypes bindings of the three native libraries share: loading a library against its table of symbols, array
pointers, the canonical CSR arrays of ``Q``, and the error mapping and lifetime of a side library's handle."""
import ctypes as C
import os

import numpy as np
from scipy import sparse


class EngineUnavailable(RuntimeError):
    """The HIP engine cannot be used (library not built, or no usable gfx950 device)."""


def load_library(path, symbols, version_symbol, version, what, no_fallback_for=None, version_noun='version'):
    """Load the shared library at ``path`` and declare the prototypes of ``symbols`` (no GPU call is made here)."""
    if not os.path.exists(path):
        raise EngineUnavailable(f'{path} is missing: {what} has not been built (run __graft_entry__.build() or '
                                '`make -C occuspytial_amd/csrc`). There is no CPU fallback'
                                + (f' for {no_fallback_for}.' if no_fallback_for else '.'))
    lib = C.CDLL(path)
    for name, restype, argtypes in symbols:
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    found = getattr(lib, version_symbol)()
    if found != version:  # a stale build: struct layouts and prototypes would not match
        raise EngineUnavailable(f'{path} has {version_noun} {found}, this binding needs {version}: rebuild it (`make -C occuspytial_amd/csrc`)')
    return lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def csr_arrays(Q, n=None):
    """``(n, indptr, indices, data)`` of ``Q`` as the libraries take it: float64, duplicates summed, columns sorted, contiguous
    int32 / int32 / float64.  ``n``: the rows of the ``X`` that ``Q`` must match (default: ``Q`` need only be square)."""
    Qc = sparse.csr_matrix(Q).astype(np.float64)
    Qc.sum_duplicates()
    Qc.sort_indices()
    if Qc.shape != ((Qc.shape[0],) * 2 if n is None else (n, n)):
        raise ValueError('Q must be square' if n is None else 'Q must be n x n with n = X.shape[0]')
    n = Qc.shape[0]
    if Qc.nnz >= 2 ** 31:
        raise ValueError('Q has too many entries for int32 indices')
    return (n, np.ascontiguousarray(Qc.indptr, dtype=np.int32), np.ascontiguousarray(Qc.indices, dtype=np.int32),
            np.ascontiguousarray(Qc.data, dtype=np.float64))


class NativeHandle:
    """One handle of a side library: a subclass names the library's ``*_last_error`` and ``*_destroy`` and what a failure is
    called, sets ``_lib`` and ``_h``, and hands the status of its create call to ``_created``."""
    _LAST_ERROR = _DESTROY = _NOUN = _h = None
    OK, E_BADARG = 0, -1

    def _created(self, code):
        if code != self.OK:
            self._h = C.c_void_p()
            self._raise(code, None)

    def _raise(self, code, handle):
        msg = getattr(self._lib, self._LAST_ERROR)(handle)
        text = msg.decode() if msg else ''
        if code == self.E_BADARG:
            raise ValueError(text or 'bad argument')
        raise EngineUnavailable(f'{self._NOUN} failure: {text}')

    def _check(self, code):
        if code != self.OK:
            self._raise(code, self._h)

    def close(self):
        if self._h:
            getattr(self._lib, self._DESTROY)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
