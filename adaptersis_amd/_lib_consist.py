"""ctypes binding of libasis_consist.so (the C ABI declared in include/asis_consist.h): the gated consistency loss of mean-teacher
training, a library beside libasis_hip.so that is loaded on first use.  Like there: no fallback, a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libasis_consist.so")

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGNATURES = {
    "asis_consist_tile": [],
    "asis_consist_nblk": [_i64],
    "asis_consist_loss": [_vp, _vp, _i, _i, _i] + [_vp] * 4 + [_i] * 4 + [_f, _f, _vp, _f, _i] + [_vp] * 4,
}

_dlib = None


def loaded() -> bool:
    """whether the library has been opened (a training step without a teacher never opens it)"""
    return _dlib is not None


def lib() -> C.CDLL:
    """Load (once) and return libasis_consist.so, after libasis_hip.so, which holds the error text both report through."""
    global _dlib
    if _dlib is not None:
        return _dlib
    _lib.lib()
    _dlib = _lib.load(LIB_PATH, SIGNATURES)
    return _dlib
