"""ctypes binding of libasis_distill.so (the C ABI declared in include/asis_distill.h): the distillation loss, a library beside
libasis_hip.so that is loaded on first use.  Like there: no fallback, a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libasis_distill.so")

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGNATURES = {
    "asis_distill_tile": [],
    "asis_distill_nblk": [_i64],
    "asis_distill_loss": [_vp, _vp, _i, _i, _i] + [_vp] * 4 + [_i] * 4 + [_f, _f, _i] + [_vp] * 3,
}

_dlib = None


def lib() -> C.CDLL:
    """Load (once) and return libasis_distill.so, after libasis_hip.so, which holds the error text both report through."""
    global _dlib
    if _dlib is not None:
        return _dlib
    _lib.lib()
    _dlib = _lib.load(LIB_PATH, SIGNATURES)
    return _dlib
