"""ctypes binding of libasis_strong.so (the C ABI declared in include/asis_strong.h): the strong student view of semi-supervised
training (colour jitter, greyscale, Gaussian blur after the augmentation), a library beside libasis_hip.so that is loaded on first
use.  Like there: no fallback, a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libasis_strong.so")

_vp, _i = C.c_void_p, C.c_int
SIGNATURES = {
    "asis_strong_chunk": [],
    "asis_strong_nblk": [C.c_int64],
    "asis_strong_mean": [_vp] * 5 + [_i] * 3 + [_vp],
    "asis_strong_view": [_vp] * 8 + [_i] * 4 + [_vp],
}

_dlib = None


def loaded() -> bool:
    """whether the library has been opened (a training step without --aug_strong never opens it)"""
    return _dlib is not None


def lib() -> C.CDLL:
    """Load (once) and return libasis_strong.so, after libasis_hip.so, which holds the error text both report through."""
    global _dlib
    if _dlib is not None:
        return _dlib
    _lib.lib()
    _dlib = _lib.load(LIB_PATH, SIGNATURES)
    return _dlib
