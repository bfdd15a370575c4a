"""ctypes binding of libasis_adapt.so (the C ABI declared in include/asis_adapt.h): the consistency loss gated by a threshold per
class, the statistics of the teacher's maps and the update of the thresholds; a library beside libasis_hip.so that is loaded on
first use.  Like there: no fallback, a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libasis_adapt.so")

_vp, _i, _i64, _f, _d = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double
SIGNATURES = {
    "asis_adapt_tile": [],
    "asis_adapt_nblk": [_i64],
    "asis_adapt_stats_nblk": [_i64],
    "asis_adapt_consist_loss": [_vp, _vp, _i, _i, _i] + [_vp] * 4 + [_i] * 4 + [_f, _vp, _vp, _f, _i] + [_vp] * 4,
    "asis_adapt_mix_consist_loss": [_vp, _vp, _i, _i, _i] + [_vp] * 4 + [_i] * 4 + [_f, _vp, _vp, _vp, _vp, _f, _i] + [_vp] * 4,
    "asis_adapt_stats": [_vp, _i] + [_vp] * 4 + [_i] * 4 + [_f, _vp, _vp, _vp],
    "asis_adapt_update": [_vp, _vp, _vp, _vp, _i, _d],
}

_dlib = None


def loaded() -> bool:
    """whether the library has been opened (a training step without class thresholds never opens it)"""
    return _dlib is not None


def lib() -> C.CDLL:
    """Load (once) and return libasis_adapt.so, after libasis_hip.so, which holds the error text both report through."""
    global _dlib
    if _dlib is not None:
        return _dlib
    _lib.lib()
    _dlib = _lib.load(LIB_PATH, SIGNATURES)
    return _dlib
