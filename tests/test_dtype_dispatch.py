"""CPU: an operand dtype that is neither ASIS_F16 nor ASIS_BF16 never reaches a launch.

Every entry below is called with real, 16-byte-aligned host buffers, a NULL stream and a shape that passes each check
the entry makes before it looks at the dtype; with dtype 7 it must return ASIS_EINVAL and leave "<name>: bad dtype 7"
in asis_last_error().  <name> is the name the entry uses in its messages: the `_split` / `_qkv` entries report under
the name of the entry family they implement (asis_swiglu, asis_im2col_patch, asis_msda_fwd, asis_attention_fwd).
Nothing is launched, so the test needs no GPU (and is skipped where one is present: a launch there would be real).
"""
import ctypes as C

import pytest
import torch

from adaptersis_amd import _lib

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="host-side argument checks: run on the CPU box")

BAD = 7
_keep = []


def buf(nbytes=4096):
    """Address of a zeroed, 16-byte-aligned host buffer."""
    raw = C.create_string_buffer(nbytes + 16)
    _keep.append(raw)
    return (C.addressof(raw) + 15) & ~15


# entry -> (name in its messages, arguments after (stream, dtype))
CASES = {
    "asis_bn_act": ("asis_bn_act", lambda: [buf(), buf(), buf(), 1, buf(), buf(), 4, 8]),
    "asis_swiglu_split": ("asis_swiglu", lambda: [buf(), buf(), buf(), 4, 8]),
    "asis_mx_from_pair": ("asis_mx_from_pair", lambda: [buf(), buf(), 8, buf(), 8, 4, 8, buf(), 0]),
    "asis_gelu_split": ("asis_gelu_split", lambda: [buf(), buf(), buf(), 8]),
    "asis_swiglu_bwd": ("asis_swiglu_bwd", lambda: [buf(), buf(), buf(), 4, 8]),
    "asis_colsum": ("asis_colsum", lambda: [buf(), 8, buf(), 4, 8]),
    "asis_cast_pad": ("asis_cast_pad", lambda: [buf(), 8, buf(), 8, 4, 8, 1.0, 0]),
    "asis_im2col_patch_split": ("asis_im2col_patch", lambda: [buf(), 1, 14, 14, 14, buf(), buf(), 592]),
    "asis_layernorm_mx": ("asis_layernorm_mx", lambda: [buf(), 8, buf(), buf(), 1e-6, buf(), buf(), 8, buf(), 4, 8]),
    "asis_msda_fwd_split": ("asis_msda_fwd", lambda: [buf(), buf(), 3, buf(), buf(), buf(), buf(), buf(), 1, 1, 1, 1, 1, 1, 8]),
    "asis_dropout_t16": ("asis_dropout_t16", lambda: [buf(), None, 8, 1, 0, 0.5, 0]),
    "asis_resize_bilinear_bwd": ("asis_resize_bilinear_bwd", lambda: [buf(), 1, 4, 4, 2, 2, 2, 8, buf(), buf(), buf()]),
    "asis_conv3x3_smallcout_fwd": ("asis_conv3x3_smallcout_fwd", lambda: [buf(), buf(), buf(), buf(), buf(), 1, 4, 4, 8, 2]),
    "asis_transpose_tokens": ("asis_transpose_tokens", lambda: [buf(), 64, buf(), 64, 1, 4, 64]),
    "asis_dilate2": ("asis_dilate2", lambda: [buf(), buf(), buf(), buf(), 1, 2, 2, 3, 3, 8]),
    "asis_attention_fwd_qkv": ("asis_attention_fwd", lambda: [buf(), buf(), buf(), 64, buf(), buf(), 64, 1, 4, 0, 0, 1, 0.125, 0, None]),
}


def expect_bad_dtype(lib, rc, name):
    assert rc == _lib.ASIS_EINVAL
    assert b"%s: bad dtype %d" % (name.encode(), BAD) in lib.asis_last_error()


@pytest.mark.parametrize("entry", sorted(CASES))
def test_bad_dtype_is_refused(entry):
    lib = _lib.lib()
    name, args = CASES[entry]
    rc = getattr(lib, entry)(None, BAD, *args())
    expect_bad_dtype(lib, rc, name)


def test_bad_dtype_is_refused_asis_gemm():
    lib = _lib.lib()
    d = _lib.GemmDesc(A=buf(), B=buf(), C=buf(), lda=8, ldb=8, ldc=8, batch=1, M=8, N=8, K=8, dtype=BAD)
    expect_bad_dtype(lib, lib.asis_gemm(None, C.byref(d)), "asis_gemm")


def test_bad_dtype_is_refused_asis_wgrad():
    lib = _lib.lib()
    d = _lib.WgradDesc(dy=buf(), x=buf(), out=buf(), ld_dy=8, P=16, dtype=BAD, Cout=8, CoP=8, Cin=8, B_=1, H=4, W=4, OH=4, OW=4,
                       KH=1, KW=1, stride=1, pad=0, splits=1)
    expect_bad_dtype(lib, lib.asis_wgrad(None, C.byref(d)), "asis_wgrad")
