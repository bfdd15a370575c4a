"""CPU: which kernel form and grid ``asis_gemm`` picks for a descriptor (``asis_gemm_plan``: nothing is launched, so this runs
with or without a GPU), and the Python shape predicates that ask the plan instead of mirroring the dispatcher.

EXPECTED was recorded from the dispatcher as it stood BEFORE it was split into plan + launch switch: that file compiled for the
host with the launch macro redefined to note the kernel instantiation and the grid, run over ROWS.  It is the reference; it was
not produced by ``asis_gemm_plan``.  A form name stands for one template instantiation (csrc/gemm.hip: launch).
The rows on the vector-epilogue requirement (include/asis_hip.h; ``*_bytes_in``, ``conv_stats_bias_aligned``) came later and
state the rule itself: the dispatcher before the split launched them and the kernel dropped the statistics, GELU' or K-part bias.

Shapes: the ViT-L/14 trunk of the default step (R = 42348 stacked token rows, D = 1024, hidden 4096; V^T GEMMs of 6 images with
3529 -> 3536 tokens), its SwiGLU / adapter / patch-embedding relatives, and the FeatureDecoder convolutions (12 images, 42^2 ..
336^2 pixels, 1024 -> 512 -> 256 -> 128 -> 64 channels)."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import pytest

from adaptersis_amd import _lib, ops
from adaptersis_amd._lib import ACT_GELU, ACT_GELU_GRAD, ACT_SILU_MUL
from adaptersis_amd.backbones import decoders

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 1 << 20            # present, 16-byte aligned; never dereferenced
R, D, HD = 42348, 1024, 4096
POINTERS = ("bias_n", "bias_m", "scale_n", "res", "stats", "A_lo", "B_lo", "aux", "mx_amax_a", "mx_amax_b", "C_lo", "rowstats", "res16",
            "res16_lo", "ln_mr", "ln_cs")


def mk(M, N, K, has=(), conv=0, **kw):
    """dense [M, K] x [N, K]^T (``conv`` = kernel size: K = conv^2 Cin over M one-pixel images, fp32 out), contiguous, the
    pointer fields named in ``has`` present; ``kw`` overrides any field"""
    d = _lib.GemmDesc(A=PTR, B=PTR, C=PTR, lda=K, ldb=K, ldc=N, batch=1, M=M, N=N, K=K, dtype=_lib.ASIS_F16, ldr=N, ldr16=N, ld_aux=N)
    if conv:
        d.conv, d.B_, d.H, d.W, d.OH, d.OW, d.Cin, d.KH, d.KW, d.stride, d.pad, d.out_f32 = 1, M, 1, 1, 1, 1, K // (conv * conv), conv, conv, 1, conv // 2, 1
    for name in has:
        assert name in POINTERS
        setattr(d, name, PTR)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


LN = ("ln_mr", "ln_cs")
PROD = ("C_lo", "rowstats", "res16", "res16_lo")
SPLIT = ("A_lo", "B_lo")
MX = SPLIT + ("mx_amax_a", "mx_amax_b")
# label -> (p8 option, descriptor)
ROWS = {
    # ---- trunk, default switches
    "qk_fold": (1, mk(R, 2 * D, D, LN + ("bias_n",))),
    "qk_plain": (1, mk(R, 2 * D, D, ("bias_n",))),
    "proj_res": (1, mk(R, D, D, ("bias_n", "scale_n", "res"))),
    "proj_producer": (1, mk(R, D, D, PROD + ("bias_n", "scale_n"))),
    "fc1_fold_gelu": (1, mk(R, HD, D, LN + ("bias_n",), act=ACT_GELU)),
    "fc2_producer": (1, mk(R, D, HD, PROD + ("bias_n", "scale_n"))),
    "fc2_res": (1, mk(R, D, HD, ("bias_n", "scale_n", "res"))),
    "vt_fold_batched": (1, mk(D, 3536, D, LN, batch=6, ln_cols=1, strideB=3536 * D, strideC=3536 * D)),
    "vt_plain_batched": (1, mk(D, 3536, D, batch=6, strideB=3536 * D, strideC=3536 * D)),
    "fc2_dgrad_gelu_grad": (1, mk(R, HD, D, ("aux",), act=ACT_GELU_GRAD)),
    "fc1_dgrad": (1, mk(R, D, HD)),
    "weight_split_k1024": (1, mk(R, D, D, ("B_lo", "bias_n"))),
    "weight_split_k4096": (1, mk(R, D, HD, ("B_lo", "bias_n"))),
    "split_f32": (1, mk(R, D, D, SPLIT, out_f32=1)),
    "split_f32_64cols": (1, mk(R, 64, D, SPLIT, out_f32=1)),
    "dense_mx": (1, mk(R, D, D, MX + ("bias_n",))),
    "swiglu": (1, mk(4096, 1376, 256, ("bias_n",), act=ACT_SILU_MUL, ldc=688)),
    "swiglu_mx": (1, mk(4096, 1376, 256, MX + ("bias_n",), act=ACT_SILU_MUL, ldc=688)),
    "patch_embed_k592": (1, mk(42336, D, 592, ("bias_n",))),
    "adapter_256cols_k1024": (1, mk(R, 256, D, ("bias_n",))),
    "msda_offsets_192cols": (1, mk(R, 192, D, ("bias_n",))),
    "narrow_64cols": (1, mk(R, 64, D, ("bias_n",))),
    "few_rows": (1, mk(200, D, D, ("bias_n",))),
    "small_k256": (1, mk(R, D, 256)),
    "column_stats_f32": (1, mk(R, D, D, ("stats",), out_f32=1)),
    # ---- decoder convolutions
    "conv_1024_512_split": (1, mk(21168, 512, 9 * 1024, SPLIT + ("bias_n",), conv=3)),
    "conv_1024_512_split_ksplit3": (1, mk(21168, 512, 9 * 1024, SPLIT + ("bias_n",), conv=3, ksplit=3, strideC=21168 * 512)),
    "conv_512_256_split_stats": (1, mk(84672, 256, 9 * 512, SPLIT + ("bias_n", "stats"), conv=3)),
    "conv_256_128_split": (1, mk(338688, 128, 9 * 256, SPLIT + ("bias_n", "stats"), conv=3)),
    "conv_128_64_split": (1, mk(1354752, 64, 9 * 128, SPLIT + ("bias_n", "stats"), conv=3)),
    "conv_128_64_split_ksplit3": (1, mk(21168, 64, 9 * 128, SPLIT, conv=3, ksplit=3, strideC=21168 * 64)),
    "conv_128_64_split_few_rows": (1, mk(300, 64, 9 * 128, SPLIT, conv=3)),
    "conv_1024_512_mx": (1, mk(21168, 512, 9 * 1024, MX + ("bias_n",), conv=3)),
    "conv_1024_512_mx_ksplit3": (1, mk(21168, 512, 9 * 1024, MX, conv=3, ksplit=3, strideC=21168 * 512)),
    "conv_256_128_mx": (1, mk(338688, 128, 9 * 256, MX + ("bias_n", "stats"), conv=3)),
    "conv_128_64_mx": (1, mk(1354752, 64, 9 * 128, MX + ("bias_n", "stats"), conv=3)),
    "conv_128_64_mx_ksplit3": (1, mk(21168, 64, 9 * 128, MX, conv=3, ksplit=3, strideC=21168 * 64)),
    "conv_plain_512": (1, mk(21168, 512, 9 * 1024, ("bias_n", "stats"), conv=3)),
    "conv_plain_128": (1, mk(338688, 128, 9 * 256, ("bias_n", "stats"), conv=3)),
    "conv_plain_64": (1, mk(1354752, 64, 9 * 128, ("bias_n", "stats"), conv=3)),
    "conv_plain_384_ragged_tile": (1, mk(21168, 384, 9 * 64, conv=3)),
    "conv_stem_cin8": (1, mk(1354752, 64, 9 * 8, ("bias_n", "stats"), conv=3)),
    "conv1x1_16bit_out": (1, mk(1354752, 8, 64, ("bias_n",), conv=1, out_f32=0)),
    # ---- the "p8" option
    "qk_plain@p8=0": (0, mk(R, 2 * D, D, ("bias_n",))),
    "qk_fold@p8=0": (0, mk(R, 2 * D, D, LN + ("bias_n",))),
    "fold_k512@p8=1": (1, mk(R, 2 * D, 512, LN)),
    "fold_k512@p8=0": (0, mk(R, 2 * D, 512, LN)),
    "16_tiles_k4096@p8=1": (1, mk(1024, 1024, HD)),
    "16_tiles_k4096@p8=2": (2, mk(1024, 1024, HD)),
    "16_tiles_k4096@p8=3": (3, mk(1024, 1024, HD)),
    "15_tiles@p8=2": (2, mk(3840, 256, D)),
    "fc1_dgrad@p8=3": (3, mk(R, D, HD)),
    "fc1_dgrad@p8=2": (2, mk(R, D, HD)),
    # ---- refusals
    "refuse_null_operand": (1, mk(R, D, D, A=None)),
    "refuse_k_not_8": (1, mk(R, D, 1020)),
    "refuse_rowstats_ragged_group": (1, mk(R, 1000, HD, ("rowstats",))),
    "refuse_gelu_grad_without_aux": (1, mk(R, HD, D, act=ACT_GELU_GRAD)),
    "refuse_gelu_grad_narrow": (1, mk(R, 64, D, ("aux",), act=ACT_GELU_GRAD)),
    "refuse_swiglu_n_not_32": (1, mk(4096, 1360, 256, act=ACT_SILU_MUL, ldc=680)),
    "refuse_swiglu_plain_split": (1, mk(4096, 1376, 256, SPLIT, act=ACT_SILU_MUL, ldc=688)),
    "refuse_dense_ksplit": (1, mk(R, D, D, ksplit=3)),
    "refuse_fold_small_k": (1, mk(2048, D, 512, LN)),
    "refuse_producer_with_activation": (1, mk(R, D, HD, PROD, act=ACT_GELU)),
    "refuse_split_few_rows": (1, mk(200, D, D, SPLIT, out_f32=1)),
    "refuse_split_conv_16bit_out": (1, mk(21168, 512, 9 * 1024, SPLIT, conv=3, out_f32=0)),
    "refuse_mx_one_maximum": (1, mk(R, D, D, SPLIT + ("mx_amax_a",))),
    "refuse_mx_dense_128cols": (1, mk(R, 128, D, MX)),
    "refuse_mx_conv_input_2g_elements": (1, mk(1354752, 64, 9 * 2048, MX, conv=3)),      # 1354752 * 2048 >= 2^31
    "conv_1024_64_mx_below_2g_elements": (1, mk(1354752, 64, 9 * 1024, MX, conv=3)),
    "refuse_conv_ksplit2": (1, mk(21168, 512, 9 * 1024, SPLIT, conv=3, ksplit=2, strideC=21168 * 512)),
    "refuse_conv_ksplit_stats": (1, mk(21168, 512, 9 * 1024, ("stats",), conv=3, ksplit=3, strideC=21168 * 512)),
    "refuse_generic_conv_ksplit": (1, mk(21168, 512, 9 * 8, conv=3, ksplit=3, strideC=21168 * 512)),
    # statistics, GELU' and K parts live in the vector epilogue of the large-tile kernels, which the kernel leaves at run time for
    # an operand off its 16-byte boundary (tests/gemm_ref.py: MISALIGNED holds the same four launches for the GPU)
    "refuse_conv_stats_bias_4_bytes_in": (1, mk(312, 136, 9 * 64, ("stats",), conv=3, bias_n=PTR + 4)),
    "refuse_conv_ksplit_bias_4_bytes_in": (1, mk(312, 136, 9 * 64, conv=3, ksplit=3, strideC=312 * 136, bias_n=PTR + 4)),
    "refuse_gelu_grad_bias_4_bytes_in": (1, mk(300, 136, 96, ("aux",), act=ACT_GELU_GRAD, bias_n=PTR + 4)),
    "refuse_gelu_grad_res_8_bytes_in": (1, mk(300, 136, 96, ("aux", "scale_n"), act=ACT_GELU_GRAD, out_f32=1, res=PTR + 8)),
    "conv_stats_bias_aligned": (1, mk(312, 136, 9 * 64, ("stats", "bias_n"), conv=3)),
    "plain_bias_4_bytes_in_scalar_epilogue": (1, mk(300, 136, 96, bias_n=PTR + 4)),
}
# the two messages of "no kernel form takes this descriptor"
NO_FORM = ("asis_gemm: split-precision operands / ASIS_ACT_GELU_GRAD / ksplit need the large-tile path (K % 64 == 0 (GELU_GRAD: 32), "
           "M >= 256, N >= 32 (128), N and ldc multiples of 4, fp32 output for split; conv: Cin % 64 == 0)")
NOT_VEC = "asis_gemm: stats / ASIS_ACT_GELU_GRAD / ksplit run in the vector epilogue of the large-tile kernels only: %s (include/asis_hip.h)"
NO_SWIGLU_FORM = ("asis_gemm: ASIS_ACT_SILU_MUL needs a dense 16-bit-output launch on the 8-phase form (include/asis_hip.h: K % 64 == 0, "
                  "M >= 256, N >= 256, N % 32 == 0, ldc % 8 == 0, plain or MX split operands, bias only)")
# (form, grid_x, grid_y, block), or the message of the ASIS_EINVAL refusal
EXPECTED = {
    "qk_fold": ("p8_ln", 256, 1, 512),
    "qk_plain": ("p8", 256, 1, 512),
    "proj_res": ("p8", 256, 1, 512),
    "proj_producer": ("ph8_ln", 664, 1, 512),
    "fc1_fold_gelu": ("p8_ln", 256, 1, 512),
    "fc2_producer": ("ph8_ln", 664, 1, 512),
    "fc2_res": ("ph8_m16", 664, 1, 512),
    "vt_fold_batched": ("ph8_ln", 56, 6, 512),
    "vt_plain_batched": ("ph8_m16", 56, 6, 512),
    "fc2_dgrad_gelu_grad": ("p8", 256, 1, 512),
    "fc1_dgrad": ("ph8_m16", 664, 1, 512),
    "weight_split_k1024": ("p8", 256, 1, 512),
    "weight_split_k4096": ("big_256x128_split", 1328, 1, 512),
    "split_f32": ("big_256x128_split", 1328, 1, 512),
    "split_f32_64cols": ("big_256x64_split", 166, 1, 512),
    "dense_mx": ("ph8_mx", 664, 1, 512),
    "swiglu": ("ph8_m16", 96, 1, 512),
    "swiglu_mx": ("ph8_mx", 96, 1, 512),
    "patch_embed_k592": ("generic", 2648, 1, 256),
    "adapter_256cols_k1024": ("ph8_m16", 166, 1, 512),
    "msda_offsets_192cols": ("big_256x128_m16", 332, 1, 512),
    "narrow_64cols": ("generic", 331, 1, 256),
    "few_rows": ("generic", 16, 1, 256),
    "small_k256": ("p8", 256, 1, 512),
    "column_stats_f32": ("generic", 2648, 1, 256),
    "conv_1024_512_split": ("conv_ph8_split", 166, 1, 512),
    "conv_1024_512_split_ksplit3": ("conv_ph8_split", 166, 3, 512),
    "conv_512_256_split_stats": ("conv_ph8_split", 331, 1, 512),
    "conv_256_128_split": ("conv_256x128_split", 1323, 1, 512),
    "conv_128_64_split": ("conv_512x64_split", 2646, 1, 512),
    "conv_128_64_split_ksplit3": ("conv_256x64_split", 83, 3, 512),
    "conv_128_64_split_few_rows": ("conv_256x64_split", 2, 1, 512),
    "conv_1024_512_mx": ("conv_ph8_mx", 166, 1, 512),
    "conv_1024_512_mx_ksplit3": ("conv_ph8_mx", 166, 3, 512),
    "conv_256_128_mx": ("conv_256x128_mx", 1323, 1, 512),
    "conv_128_64_mx": ("conv_512x64_mx", 2646, 1, 512),
    "conv_128_64_mx_ksplit3": ("conv_256x64_mx", 83, 3, 512),
    "conv_1024_64_mx_below_2g_elements": ("conv_512x64_mx", 2646, 1, 512),
    "conv_plain_512": ("conv_ph8", 166, 1, 512),
    "conv_plain_128": ("conv_256x128", 1323, 1, 512),
    "conv_plain_64": ("conv_256x64", 5292, 1, 512),
    "conv_plain_384_ragged_tile": ("conv_256x128", 249, 1, 512),
    "conv_stem_cin8": ("generic_conv", 10584, 1, 256),
    "conv1x1_16bit_out": ("generic_conv", 10584, 1, 256),
    "qk_plain@p8=0": ("ph8_m16", 1328, 1, 512),
    "qk_fold@p8=0": ("ph8_ln", 1328, 1, 512),
    "fold_k512@p8=1": ("p8_ln", 256, 1, 512),
    "fold_k512@p8=0": NO_FORM,
    "16_tiles_k4096@p8=1": ("ph8_m16", 16, 1, 512),
    "16_tiles_k4096@p8=2": ("p8", 16, 1, 512),
    "16_tiles_k4096@p8=3": ("ph8_m16", 16, 1, 512),
    "15_tiles@p8=2": ("big_256x128_m16", 30, 1, 512),
    "fc1_dgrad@p8=3": ("p8", 256, 1, 512),
    "fc1_dgrad@p8=2": ("p8", 256, 1, 512),
    "refuse_null_operand": "asis_gemm: null operand pointer",
    "refuse_k_not_8": "asis_gemm: K=1020 must be a multiple of 8",
    "refuse_rowstats_ragged_group": "asis_gemm: rowstats need N % 64 == 0 (N = 1000)",
    "refuse_gelu_grad_without_aux": NO_FORM,
    "refuse_gelu_grad_narrow": NO_FORM,
    "refuse_swiglu_n_not_32": NO_SWIGLU_FORM,
    "refuse_swiglu_plain_split": NO_SWIGLU_FORM,
    "refuse_dense_ksplit": NO_FORM,
    "refuse_fold_small_k": NO_FORM,
    "refuse_producer_with_activation": NO_FORM,
    "refuse_split_few_rows": NO_FORM,
    "refuse_split_conv_16bit_out": NO_FORM,
    "refuse_mx_one_maximum": NO_FORM,
    "refuse_mx_dense_128cols": NO_FORM,
    "refuse_mx_conv_input_2g_elements": NO_FORM,
    "refuse_conv_ksplit2": NO_FORM,
    "refuse_conv_ksplit_stats": NO_FORM,
    "refuse_generic_conv_ksplit": NO_FORM,
    "refuse_conv_stats_bias_4_bytes_in": NOT_VEC % "bias_n must be 16-byte aligned",
    "refuse_conv_ksplit_bias_4_bytes_in": NOT_VEC % "bias_n must be 16-byte aligned",
    "refuse_gelu_grad_bias_4_bytes_in": NOT_VEC % "bias_n must be 16-byte aligned",
    "refuse_gelu_grad_res_8_bytes_in": NOT_VEC % "res must be 16-byte aligned in every batch entry (strideR a multiple of 4)",
    "conv_stats_bias_aligned": ("conv_256x128", 4, 1, 512),
    "plain_bias_4_bytes_in_scalar_epilogue": ("big_256x128_m16", 4, 1, 512),
}
# switch in the child's environment -> label -> expectation (recorded the same way, with the switch set)
ENV_ROWS = {
    "ASIS_GEMM_8P=0": ("fc2_res", "fc2_producer", "fc1_dgrad"),
    "ASIS_CONV_8P=0": ("conv_1024_512_split", "conv_plain_512", "conv_512_256_split_stats"),
}
ENV_EXPECTED = {
    "ASIS_GEMM_8P=0": {
        "fc2_res": ("big_256x128_m16", 1328, 1, 512),
        "fc2_producer": NO_FORM,
        "fc1_dgrad": ("big_256x128_m16", 1328, 1, 512)},
    "ASIS_CONV_8P=0": {
        "conv_1024_512_split": ("conv_256x128_split", 332, 1, 512),
        "conv_plain_512": ("conv_256x128", 332, 1, 512),
        "conv_512_256_split_stats": ("conv_256x128_split", 662, 1, 512)},
}
DEFAULT_FORMS = {"p8", "p8_ln", "ph8_m16", "ph8_ln", "ph8_mx", "big_256x128_m16", "big_256x128_split", "big_256x64_split", "conv_ph8",
                 "conv_256x128", "conv_256x64", "conv_ph8_split", "conv_512x64_split", "conv_256x128_split", "conv_256x64_split",
                 "conv_ph8_mx", "conv_512x64_mx", "conv_256x128_mx", "conv_256x64_mx", "generic", "generic_conv"}


def plan(d):
    """what EXPECTED holds, from asis_gemm_plan"""
    lib = _lib.lib()
    form, gx, gy, block = C.c_int(-1), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = lib.asis_gemm_plan(C.byref(d), C.byref(form), C.byref(gx), C.byref(gy), C.byref(block))
    if rc != 0:
        assert rc == _lib.ASIS_EINVAL and form.value == -1
        return lib.asis_last_error().decode()
    return lib.asis_gemm_form_name(form.value).decode(), gx.value, gy.value, block.value


@pytest.fixture
def p8_option():
    yield lambda v: ops.gemm_set_option("p8", v)
    ops.gemm_set_option("p8", 1)


@pytest.mark.parametrize("label", sorted(ROWS))
def test_plan_is_what_the_dispatcher_did(label, p8_option):
    p8, d = ROWS[label]
    p8_option(p8)
    got = plan(d)
    print(label, got)
    assert got == EXPECTED[label]
    assert isinstance(got, str) == (label.startswith("refuse") or label == "fold_k512@p8=0")
    if isinstance(got, str):
        with pytest.raises(ValueError, match="asis_gemm: "):
            ops.gemm_plan(d)
    else:
        assert ops.gemm_plan(d) == got[:3]


def test_expected_table_has_every_default_form_and_the_option_flips():
    """completeness of the recorded table itself (test_plan_is_what_the_dispatcher_did holds the library to it)"""
    seen = {e[0] for lab, e in EXPECTED.items() if ROWS[lab][0] == 1 and not isinstance(e, str)}
    assert seen == DEFAULT_FORMS
    assert EXPECTED["qk_plain"][0] == "p8" and EXPECTED["qk_plain@p8=0"][0] == "ph8_m16"
    assert EXPECTED["qk_fold"][0] == "p8_ln" and EXPECTED["qk_fold@p8=0"][0] == "ph8_ln"
    assert EXPECTED["fold_k512@p8=1"][0] == "p8_ln" and isinstance(EXPECTED["fold_k512@p8=0"], str)
    assert [EXPECTED["16_tiles_k4096@p8=%d" % v][0] for v in (1, 2, 3)] == ["ph8_m16", "p8", "ph8_m16"]
    assert EXPECTED["fc1_dgrad"][0] == "ph8_m16" and EXPECTED["fc1_dgrad@p8=3"][0] == EXPECTED["fc1_dgrad@p8=2"][0] == "p8"


def test_predicates_follow_the_p8_option(p8_option):
    """the shape predicates answer for the dispatcher as it is set: rows fold_k512@p8=1 / @p8=0"""
    assert ops.ln_fold_supported(R, 2 * D, 512)
    p8_option(0)
    assert not ops.ln_fold_supported(R, 2 * D, 512)
    p8_option(1)
    assert ops.ln_fold_supported(R, 2 * D, 512)


def test_unknown_form_and_null_outputs():
    lib = _lib.lib()
    assert lib.asis_gemm_form_name(-1) == lib.asis_gemm_form_name(1000) == b"?"
    names = [lib.asis_gemm_form_name(i).decode() for i in range(28)]
    assert len(set(names)) == 28 and "?" not in names and DEFAULT_FORMS <= set(names)
    assert lib.asis_gemm_plan(C.byref(ROWS["qk_plain"][1]), None, None, None, None) == 0
    assert lib.asis_gemm_plan(None, None, None, None, None) == _lib.ASIS_EINVAL and b"null descriptor" in lib.asis_last_error()


@pytest.mark.parametrize("switch", sorted(ENV_ROWS))
def test_options_record_honours_the_environment(switch):
    code = ("import sys; sys.path.insert(0, %r)\nfrom tests import test_gemm_plan as t\n"
            "for lab in t.ENV_ROWS[%r]: print(repr((lab, t.plan(t.ROWS[lab][1]))))" % (ROOT, switch))
    name, value = switch.split("=")
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{name: value}), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = dict(eval(line) for line in out.stdout.splitlines() if line.startswith("("))
    assert got == ENV_EXPECTED[switch]
    assert all(got[lab] != EXPECTED[lab] for lab in got)      # the switch changes every one of these rows


# ---- the Python predicates against the formulas they replaced (frozen here as they stood), default environment --------------
MS = (8, 128, 255, 256, 264, 511, 512, 2048, 3840, 3841, 4096, 32512, 32513, 32768, 42348, 65280, 65281, 65536)
NS = (8, 32, 36, 64, 68, 100, 128, 132, 255, 256, 260, 264, 288, 320, 512, 768, 1000, 1024, 1032, 2048, 2052, 4096)
KS = (8, 32, 64, 96, 128, 192, 256, 512, 768, 1024, 1056, 2048, 2080, 2112, 4096)


def old_ln_fold_supported(M, N, K, batch=1, producer=False):
    if M < 256 or N < 256 or K % 64 or K < 128 or N % 8:
        return False
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    if not producer and batch == 1 and tiles >= 256 and K <= 2048:
        return True
    return K >= 2048 or (K >= 1024 and tiles * batch >= 128)


def old_swiglu_fused_ok(M, Hd, K, split, mx):
    return Hd % 16 == 0 and 2 * Hd >= 256 and M >= 256 and K % 64 == 0 and (mx or not split)


def old_fused_split(M, N, K):
    return K % 64 == 0 and M >= 256 and N >= 32 and N % 4 == 0


def old_conv_ksplit(P, Cout, Cin, split):
    if Cin % 64 or P < 256 or Cout < 32 or Cout % 4:
        return 1
    cus = 256
    if Cout >= 256 and (Cout % 256 == 0 or Cout >= 1024):
        tiles = ((P + 255) // 256) * ((Cout + 255) // 256)
        now, cut = -(-tiles // cus), -(-3 * tiles // cus) / 3.0 * 1.08
        return 3 if cut < 0.88 * now else 1
    tiles = ((P + 255) // 256) * ((Cout + 127) // 128 if Cout > 64 else (Cout + 63) // 64)

    def cost(t):
        c = -(-t // cus)
        return 1.7 * (c // 2) + (c % 2)

    now, cut = cost(tiles), cost(3 * tiles) / 3.0 * 1.08
    return 3 if cut < 0.88 * now else 1


def test_ln_fold_supported_is_the_old_formula():
    n = 0
    for M, N, K in itertools.product(MS, NS, KS):
        for batch in (1, 2, 6):
            assert ops.ln_fold_supported(M, N, K, batch=batch) == old_ln_fold_supported(M, N, K, batch), (M, N, K, batch)
        assert ops.ln_fold_supported(M, N, K, producer=True) == old_ln_fold_supported(M, N, K, 1, True), (M, N, K, "producer")
        n += 4
    assert n == 4 * len(MS) * len(NS) * len(KS)


def test_swiglu_fused_ok_is_the_old_formula():
    assert ops._SWIGLU_FUSED
    for M, N, K in itertools.product(MS, NS, KS):
        for Hd in {N // 2, N // 2 + 1, N} if N % 2 == 0 else {N}:
            for split, mx in ((False, False), (True, False), (True, True), (False, True)):
                assert ops.swiglu_fused_ok(M, Hd, K, split, mx) == old_swiglu_fused_ok(M, Hd, K, split, mx), (M, Hd, K, split, mx)


def test_fused_split_rule_is_the_old_formula(monkeypatch):
    for M, N, K in itertools.product(MS, NS, KS):
        want = old_fused_split(M, N, K)
        assert ops._split_shape_ok(M, N, K) == want and ops._fused_split(M, N, K) == want and ops.mx_conv_ok(M, K, N) == want, (M, N, K)
    monkeypatch.setattr(ops, "_SPLIT_FUSED", False)      # ASIS_SPLIT_FUSED=0: the routing switch of the callers
    assert not ops._fused_split(R, D, D) and not ops.mx_conv_ok(R, D, D) and ops._split_shape_ok(R, D, D)


def test_conv_ksplit_is_the_old_cost_model():
    assert decoders._KSPLIT
    cases = 0
    for P, Cout, Cin in itertools.product(MS + (21168, 84672, 338688, 1354752), NS, (8, 64, 96, 128, 512, 1024, 3072)):
        for split in (False, True):
            assert decoders._conv_ksplit(P, Cout, Cin, split) == old_conv_ksplit(P, Cout, Cin, split), (P, Cout, Cin, split)
            cases += 1
    threes = sum(decoders._conv_ksplit(P, C_, 1024, True) == 3 for P in (21168, 84672) for C_ in (64, 128, 256, 512))
    assert cases > 5000 and threes >= 2      # the model does cut layers of the default decoder (decoder_1, decoder_2)
