"""ctypes binding of libasis_semi.so (the C ABI declared in include/asis_semi.h): the fused segmentation loss with an ignore
label, the hard loss of semi-supervised training, a library beside libasis_hip.so that is loaded on first use.  Like there: no
fallback, a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libasis_semi.so")

_vp, _i, _f = C.c_void_p, C.c_int, C.c_float
SIGNATURES = {
    "asis_semi_partial_stride": [_i],
    "asis_semi_loss": [_vp] * 4 + [_i] * 9 + [_f, _i, _f] + [_vp] * 6,
}

_dlib = None


def loaded() -> bool:
    """whether the library has been opened (a training step without an ignore label or an unlabelled frame never opens it)"""
    return _dlib is not None


def lib() -> C.CDLL:
    """Load (once) and return libasis_semi.so, after libasis_hip.so, which holds the error text both report through."""
    global _dlib
    if _dlib is not None:
        return _dlib
    _lib.lib()
    _dlib = _lib.load(LIB_PATH, SIGNATURES)
    return _dlib
