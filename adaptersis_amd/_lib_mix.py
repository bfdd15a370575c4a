"""ctypes binding of libasis_mix.so (the C ABI declared in include/asis_mix.h): CutMix / ClassMix over the samples of a batch and the
consistency loss over such a batch, a library beside libasis_hip.so that is loaded on first use.  Like there: no fallback, a missing
library raises."""
from __future__ import annotations

import ctypes as C
import os

from . import _lib

LIB_PATH = os.path.join(os.path.dirname(_lib.LIB_PATH), "libasis_mix.so")

_vp, _i, _i64, _f = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGNATURES = {
    "asis_mix_tile": [],
    "asis_mix_nblk": [_i, _i64],
    "asis_mix_class_sets": [_vp] * 5 + [_i] * 5 + [_vp],
    "asis_mix_apply": [_vp] * 7 + [_i] * 3 + [_vp] * 4,
    "asis_mix_consist_tile": [],
    "asis_mix_consist_nblk": [_i64],
    "asis_mix_consist_loss": [_vp, _vp, _i, _i, _i] + [_vp] * 4 + [_i] * 4 + [_f, _f, _vp, _vp, _vp, _f, _i] + [_vp] * 4,
}

_dlib = None


def loaded() -> bool:
    """whether the library has been opened (a training step that mixes nothing never opens it)"""
    return _dlib is not None


def lib() -> C.CDLL:
    """Load (once) and return libasis_mix.so, after libasis_hip.so, which holds the error text both report through."""
    global _dlib
    if _dlib is not None:
        return _dlib
    _lib.lib()
    _dlib = _lib.load(LIB_PATH, SIGNATURES)
    return _dlib
