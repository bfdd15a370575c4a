"""Tensor-level wrappers over the C ABI (include/asis_hip.h).

torch is used here only as the owner of device memory and of the current HIP stream: every
function takes CUDA(=HIP) tensors, passes raw pointers/sizes to libasis_hip.so and returns
tensors allocated with ``torch.empty``.  A CPU tensor, a missing library or a bad shape raises.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from typing import Optional

import torch

from . import _lib, config
from ._lib import ACT_GELU, ACT_GELU_GRAD, ACT_NONE, ACT_RELU, ACT_SILU_MUL, GemmDesc, check, lib  # noqa: F401

T16_DEFAULT = torch.float16

# bench.py sets this to a list to time every GEMM launch with HIP events recorded on the launch stream:
# entries are (kind, algorithmic_flops, start_event, end_event, algorithmic_bytes).  None = no instrumentation.
# Algorithmic = 2*M*N*K and one read of each operand + one write of the output, also for split-precision launches
# (their two extra products are this build's precision choice, not work the reference asks for).
PROFILE = None


def _launch_timed(kind: str, flops: float, fn, nbytes: float = 0.0):
    if PROFILE is None:
        return fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    rc = fn()
    e.record()
    PROFILE.append((kind, flops, s, e, nbytes))
    return rc


def _dt(dtype: torch.dtype) -> int:
    if dtype == torch.float16:
        return _lib.ASIS_F16
    if dtype == torch.bfloat16:
        return _lib.ASIS_BF16
    raise ValueError(f"operand dtype must be float16 or bfloat16, got {dtype}")


def _dev(*ts) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.AsisError("adaptersis_amd ops run on an MI355X (HIP) device only; got a CPU tensor "
                                 "(there is no CPU fallback)")


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32c(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("expected a contiguous float32 tensor")
    return t


def _split_shape_ok(M: int, N: int, K: int) -> bool:
    """shapes whose split-precision product runs as ONE launch over the virtual 2K / 3K reduction (large-tile kernels,
    include/asis_hip.h: A_lo / B_lo; convolutions: K = Cin); the callers' alternative is three accumulate passes"""
    return K % 64 == 0 and M >= 256 and N >= 32 and N % 4 == 0


def _gemm_desc(a: torch.Tensor, b: torch.Tensor, *, out: Optional[torch.Tensor] = None, out_f32: bool = False,
               bias_n: Optional[torch.Tensor] = None, bias_m: Optional[torch.Tensor] = None,
               scale_n: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None, act: int = ACT_NONE,
               stats: Optional[torch.Tensor] = None, a_lo: Optional[torch.Tensor] = None,
               b_lo: Optional[torch.Tensor] = None, aux: Optional[torch.Tensor] = None,
               out_lo: Optional[torch.Tensor] = None, rowstats: Optional[torch.Tensor] = None, res16=None, ln=None, mx=None):
    """-> (filled GemmDesc, out tensor, algorithmic flops, algorithmic bytes) of one ``gemm`` call (see ``gemm``).
    LayerNorm-fold chain (include/asis_hip.h): ``out_lo`` = second 16-bit plane of the output, ``rowstats`` = fp32
    [M, ceil(N / 64), 2] per-row partial sums, ``res16`` = (hi, lo) planes of the residual, ``ln`` = (mr [rows, 2], cs, cols)."""
    _dev(a, b, out, bias_n, bias_m, scale_n, res, stats, out_lo, rowstats)
    if a.dtype != b.dtype:
        raise ValueError("gemm operands must have the same 16-bit dtype")
    batch = 1
    if a.dim() == 3 or b.dim() == 3:
        batch = a.shape[0] if a.dim() == 3 else b.shape[0]
    M, K = a.shape[-2], a.shape[-1]
    N = b.shape[-2]
    if b.shape[-1] != K:
        raise ValueError(f"gemm: inner dims differ: a[...,{K}] vs b[...,{b.shape[-1]}]")
    if a.stride(-1) != 1 or b.stride(-1) != 1:
        raise ValueError("gemm: K must be contiguous in both operands")
    n_out = N // 2 if act == ACT_SILU_MUL else N      # SwiGLU epilogue: b = interleaved w12 (swiglu_rows), out = [M, Hd]
    if act == ACT_SILU_MUL and (out_f32 or batch != 1 or N % 32):
        raise ValueError("gemm: ACT_SILU_MUL writes a 16-bit [M, N / 2] matrix of one unbatched launch (N % 32 == 0)")
    if out is None:
        shape = (batch, M, n_out) if (a.dim() == 3 or b.dim() == 3) else (M, n_out)
        out = torch.empty(shape, device=a.device, dtype=torch.float32 if out_f32 else a.dtype)
    else:
        out_f32 = out.dtype == torch.float32
        if out.stride(-1) != 1 or out.shape[-1] != n_out:
            raise ValueError("gemm: out must be contiguous in its last dim, one column per output feature")
    d = GemmDesc()
    d.A, d.B, d.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    d.lda, d.ldb, d.ldc = a.stride(-2), b.stride(-2), out.stride(-2)
    d.strideA = a.stride(0) if a.dim() == 3 else 0
    d.strideB = b.stride(0) if b.dim() == 3 else 0
    d.strideC = out.stride(0) if out.dim() == 3 else 0
    d.batch, d.M, d.N, d.K = batch, M, N, K
    d.bias_n, d.bias_m, d.scale_n = _p(_f32c(bias_n)), _p(_f32c(bias_m)), _p(_f32c(scale_n))
    if res is not None:
        if res.dtype != torch.float32 or res.stride(-1) != 1:
            raise ValueError("gemm: res must be float32, contiguous in its last dim")
        d.res, d.ldr = res.data_ptr(), res.stride(-2)
        d.strideR = res.stride(0) if res.dim() == 3 else 0
    d.act, d.out_f32, d.dtype = act, int(out_f32), _dt(a.dtype)
    d.stats = _p(stats)
    if aux is not None:
        if aux.dtype != a.dtype or aux.shape[-2:] != (M, N) or aux.stride(-1) != 1:
            raise ValueError("gemm: aux must be a 16-bit [M, N] matrix of the operand dtype")
        d.aux, d.ld_aux = aux.data_ptr(), aux.stride(-2)
    flops = 2.0 * batch * M * N * K
    if (a_lo is None) != (b_lo is None) and not (_split_shape_ok(M, N, K) and out.stride(-2) % 4 == 0):
        a_lo = b_lo = None   # one-sided (weight) split is an optional refinement: shapes off the large-tile path run plain
    if a_lo is not None:
        if a_lo.stride() != a.stride():
            raise ValueError("gemm: split halves must share the layout of their hi parts")
        d.A_lo = a_lo.data_ptr()
    if b_lo is not None:
        if b_lo.stride() != b.stride():
            raise ValueError("gemm: split halves must share the layout of their hi parts")
        d.B_lo = b_lo.data_ptr()
    if mx is not None:
        if a_lo is None or b_lo is None:
            raise ValueError("gemm: mx needs both MX planes (a_lo and b_lo)")
        _dev(mx[0], mx[1])
        d.mx_amax_a, d.mx_amax_b = mx[0].data_ptr(), mx[1].data_ptr()
    if out_lo is not None:
        if out_lo.dtype != out.dtype or out_lo.stride() != out.stride() or out.dtype == torch.float32:
            raise ValueError("gemm: out_lo must be a 16-bit tensor with the layout of out")
        d.C_lo = out_lo.data_ptr()
    if rowstats is not None:
        if rowstats.dtype != torch.float32 or rowstats.numel() != M * ((N + 63) // 64) * 2 or not rowstats.is_contiguous():
            raise ValueError("gemm: rowstats must be a contiguous float32 [M, ceil(N / 64), 2] tensor")
        d.rowstats = rowstats.data_ptr()
    if res16 is not None:
        rh, rl = res16
        _dev(rh, rl)
        if rh.dtype != a.dtype or rl.dtype != a.dtype or rh.stride() != rl.stride() or rh.stride(-1) != 1 or rh.shape[-2:] != (M, N):
            raise ValueError("gemm: res16 = (hi, lo) 16-bit [M, N] planes of the operand dtype with equal strides")
        d.res16, d.res16_lo, d.ldr16 = rh.data_ptr(), rl.data_ptr(), rh.stride(-2)
    if ln is not None:
        mr, cs, cols = ln
        _dev(mr, cs)
        d.ln_mr, d.ln_cs, d.ln_cols = _f32c(mr).data_ptr(), _f32c(cs).data_ptr(), int(bool(cols))
    nbytes = batch * (2.0 * (M * K + N * K) + M * N * ((4 if (out_f32 or out_lo is not None) else 2) +
                                                    (4 if (res is not None or res16 is not None) else 0)))
    return d, out, flops, nbytes


def gemm(a: torch.Tensor, b: torch.Tensor, **kw) -> torch.Tensor:
    """``out = epilogue(a @ b.T)``; a [M,K] or [batch,M,K], b [N,K] or [batch,N,K] (16-bit, K contiguous).
    Keywords: out, out_f32, bias_n, bias_m, scale_n, res, act, stats, a_lo, b_lo, aux (see ``_gemm_desc``).
    ``act=ACT_GELU_GRAD`` with ``aux`` (16-bit [M, N] pre-activation): out = (a @ b.T) * gelu'(aux).

    A 2-D operand next to a 3-D one is shared by every batch element.  Row strides may exceed K.
    """
    d, out, flops, nbytes = _gemm_desc(a, b, **kw)
    check(_launch_timed("gemm", flops, lambda: lib().asis_gemm(_stream(), C.byref(d)), nbytes), "asis_gemm")
    return out


def gemm_tiles_m(M: int) -> int:
    return lib().asis_gemm_tiles_m(int(M))


def _plan(d: GemmDesc):
    """``gemm_plan``, or None where ``asis_gemm`` refuses ``d``"""
    form, gx, gy = C.c_int(), C.c_int(), C.c_int()
    if lib().asis_gemm_plan(C.byref(d), C.byref(form), C.byref(gx), C.byref(gy), None) != 0:
        return None
    return lib().asis_gemm_form_name(form.value).decode(), gx.value, gy.value


def gemm_plan(d: GemmDesc):
    """-> (form name, grid_x, grid_y): the kernel form ``asis_gemm`` would launch for ``d`` and its grid (include/asis_hip.h:
    asis_gemm_plan); ValueError where it refuses ``d``.  Launches nothing and needs no GPU."""
    return _plan(d) or check(_lib.ASIS_EINVAL, "asis_gemm_plan")


_PRESENT = 1 << 20   # a 16-byte-aligned placeholder address: the plan only tests pointers for null and alignment


@functools.lru_cache(maxsize=None)
def _shape_plan(M: int, N: int, K: int, batch: int = 1, act: int = ACT_NONE, out_f32: bool = False, split: bool = False,
                mx: bool = False, ln: bool = False, producer: bool = False, conv3x3: bool = False):
    """``gemm_plan`` (None: refused) of a contiguous launch of this shape (lda = ldb = K, ldc = N, or N / 2 for SwiGLU) with the
    named operand fields present: what the shape predicates below ask instead of repeating the dispatcher's rules.  ``producer``:
    C_lo, res16 and (N in whole 64-column groups) rowstats; ``conv3x3``: K = 9 Cin, stride 1, pad 1, M one-pixel images.  The
    answers follow the dispatcher's switches, the run-time ``"p8"`` option included: ``gemm_set_option`` empties this cache.  A
    first refused query leaves its message in ``asis_last_error`` (read only after a call that failed, so nobody sees it)."""
    d = GemmDesc(A=_PRESENT, B=_PRESENT, C=_PRESENT, lda=K, ldb=K, ldc=N // 2 if act == ACT_SILU_MUL else N, batch=batch, M=M, N=N,
                 K=K, act=act, out_f32=int(out_f32), dtype=_lib.ASIS_F16)
    if split:
        d.A_lo = d.B_lo = _PRESENT
    if mx:
        d.mx_amax_a = d.mx_amax_b = _PRESENT
    if ln:
        d.ln_mr = d.ln_cs = _PRESENT
    if producer:
        d.C_lo = d.res16 = d.res16_lo = _PRESENT
        d.ldr16, d.rowstats = N, (_PRESENT if N % 64 == 0 else None)
    if conv3x3:
        d.conv, d.B_, d.H, d.W, d.OH, d.OW, d.Cin, d.KH, d.KW, d.stride, d.pad = 1, M, 1, 1, 1, 1, K // 9, 3, 3, 1, 1
    return _plan(d)


def conv3x3_plan(P: int, Cout: int, Cin: int, split: bool):
    """``gemm_plan`` of a 3x3 convolution with P output pixels and an fp32 output (None: refused)"""
    return _shape_plan(P, Cout, 9 * Cin, out_f32=True, split=split, conv3x3=True)


def gemm_set_option(name: str, value: int) -> None:
    """Run-time dispatch switch of ``asis_gemm`` (``"p8"``: the persistent 8-phase form, include/asis_hip.h)."""
    check(lib().asis_gemm_set_option(name.encode(), int(value)), "asis_gemm_set_option")
    _shape_plan.cache_clear()


def _conv_desc(x_nhwc: torch.Tensor, w_packed: torch.Tensor, KH: int, KW: int, stride: int, pad: int, *,
               out: Optional[torch.Tensor] = None, out_f32: bool = True, bias_n: Optional[torch.Tensor] = None,
               act: int = ACT_NONE, stats: Optional[torch.Tensor] = None, accumulate: bool = False,
               x_lo: Optional[torch.Tensor] = None, w_lo: Optional[torch.Tensor] = None, ksplit: int = 1, mx=None):
    """-> (filled GemmDesc, the tensor the launch writes, algorithmic flops) of one ``conv_gemm`` call (see ``conv_gemm``); with
    ``ksplit`` > 1 the written tensor is the [ksplit, B, OH, OW, Cout] stack of partial maps."""
    _dev(x_nhwc, w_packed, out, bias_n, stats)
    if not x_nhwc.is_contiguous():
        raise ValueError("conv_gemm: x must be contiguous NHWC")
    Bn, H, W, Cin = x_nhwc.shape
    Cout, K = w_packed.shape
    OH = (H + 2 * pad - KH) // stride + 1
    OW = (W + 2 * pad - KW) // stride + 1
    if ksplit > 1:
        if out is not None or accumulate or not out_f32 or act != ACT_NONE or stats is not None:
            raise ValueError("conv_gemm: ksplit needs a fresh fp32 output without activation; take the BatchNorm "
                             "statistics from the sum with colstats()")
        out = torch.empty((ksplit, Bn, OH, OW, Cout), device=x_nhwc.device, dtype=torch.float32)
    if out is None:
        out = torch.empty((Bn, OH, OW, Cout), device=x_nhwc.device, dtype=torch.float32 if out_f32 else x_nhwc.dtype)
    d = GemmDesc()
    d.A, d.B, d.C = x_nhwc.data_ptr(), w_packed.data_ptr(), out.data_ptr()
    if ksplit > 1:
        d.ksplit, d.strideC = ksplit, Bn * OH * OW * Cout
    d.lda, d.ldb, d.ldc = K, w_packed.stride(0), Cout
    d.batch, d.M, d.N, d.K = 1, Bn * OH * OW, Cout, K
    d.bias_n = _p(_f32c(bias_n))
    if accumulate:  # out += conv(x, w): the epilogue adds the previous fp32 contents (same element, same thread)
        if out.dtype != torch.float32:
            raise ValueError("conv_gemm: accumulate needs an fp32 output")
        d.res, d.ldr = out.data_ptr(), Cout
    d.act, d.out_f32, d.dtype = act, int(out.dtype == torch.float32), _dt(x_nhwc.dtype)
    d.conv, d.B_, d.H, d.W, d.Cin, d.OH, d.OW = 1, Bn, H, W, Cin, OH, OW
    d.KH, d.KW, d.stride, d.pad = KH, KW, stride, pad
    d.stats = _p(stats)
    flops = 2.0 * d.M * Cout * K
    if x_lo is not None:
        d.A_lo, d.B_lo = x_lo.data_ptr(), w_lo.data_ptr()
    if mx is not None:     # x_lo / w_lo are in the MX form; mx = (amax of x, amax of w) device floats
        d.mx_amax_a, d.mx_amax_b = _f32c(mx[0]).data_ptr(), _f32c(mx[1]).data_ptr()
    return d, out, flops


def conv_gemm(x_nhwc: torch.Tensor, w_packed: torch.Tensor, KH: int, KW: int, stride: int, pad: int, **kw) -> torch.Tensor:
    """Implicit-GEMM convolution: x [B,H,W,Cin] (16-bit NHWC), w_packed [Cout, KH*KW*Cin] ->
    out [B,OH,OW,Cout] (fp32 by default: BatchNorm statistics are taken on it).
    ``ksplit`` > 1: the reduction runs as that many side-by-side parts (fp32 partial maps summed in a fixed order, then the
    caller takes the
    BatchNorm statistics from the sum with ``colstats``) — for layers whose tile count fills only part of the machine."""
    d, out, flops = _conv_desc(x_nhwc, w_packed, KH, KW, stride, pad, **kw)
    check(_launch_timed("conv", flops, lambda: lib().asis_gemm(_stream(), C.byref(d))), "asis_gemm(conv)")
    if d.ksplit > 1:
        parts, out = out, torch.empty(out.shape[1:], device=out.device, dtype=torch.float32)
        reduce_rows(parts.view(d.ksplit, -1), 1.0, out.view(-1))
    return out


_SPLIT_FUSED = os.environ.get("ASIS_SPLIT_FUSED", "1") != "0"   # 0: split-precision products as three accumulate passes


def _fused_split(M: int, N: int, K: int) -> bool:
    """``_split_shape_ok`` and the one-launch path is there: the switch above, and the large-tile kernels (a minimal split launch plans)"""
    return _SPLIT_FUSED and _split_shape_ok(M, N, K) and _shape_plan(256, 32, 64, out_f32=True, split=True) is not None


# narrow MX convolutions (64 / 128 output channels) on the halo-tile kernel (csrc/convhalo.hip): 256 -> 128 at 168^2 544 vs 577 us,
# 128 -> 64 at 336^2 540 vs 692 us against the implicit-GEMM form (scripts/bench_conv_halo.py, profiles/r04_conv_halo_ab.txt);
# ASIS_CONV_HALO=0: implicit GEMM
CONV_HALO = os.environ.get("ASIS_CONV_HALO", "1") not in ("0", "")


def conv_gemm_split(x_hi, x_lo, w_hi, w_lo, KH: int, KW: int, stride: int, pad: int, *, bias_n=None, stats=None,
                    ksplit: int = 1, mx=None):
    """Split-precision convolution: x ~= x_hi + x_lo, w ~= w_hi + w_lo (16-bit halves), fp32 out =
    x_hi*w_hi + x_lo*w_hi + x_hi*w_lo (+ bias), accumulated in fp32 (the dropped x_lo*w_lo term is ~2^-22
    relative): one launch over a virtual 3K reduction on the large-tile kernel, else three accumulate passes."""
    if mx is None:
        _not_mx("conv_gemm_split", x_lo, w_lo)
    Bn, H, W, Cin = x_hi.shape
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    Cout = w_hi.shape[0]
    if _fused_split(Bn * OH * OW, Cout, Cin):
        return conv_gemm(x_hi, w_hi, KH, KW, stride, pad, bias_n=bias_n, stats=stats, x_lo=x_lo, w_lo=w_lo, ksplit=ksplit, mx=mx)
    if mx is not None:
        raise ValueError("conv_gemm_split: MX operands need the fused large-tile path (mx_conv_ok)")
    out = conv_gemm(x_hi, w_hi, KH, KW, stride, pad, bias_n=bias_n)
    conv_gemm(x_lo, w_hi, KH, KW, stride, pad, out=out, accumulate=True)
    conv_gemm(x_hi, w_lo, KH, KW, stride, pad, out=out, accumulate=True, stats=stats)
    return out


def conv_halo_ok(x_hi: torch.Tensor, Cout: int, stride: int, pad: int, force: bool = False) -> bool:
    """shapes ``conv3x3_halo_mx`` covers: float16, stride 1, pad 1, Cin % 64 == 0, Cout 64 / 128 (csrc/convhalo.hip); ``force``:
    whatever the ASIS_CONV_HALO switch says"""
    return ((CONV_HALO or force) and x_hi.dtype == torch.float16 and stride == 1 and pad == 1 and x_hi.shape[3] % 64 == 0 and Cout in (64, 128)
            and x_hi.is_contiguous())


def conv3x3_halo_mx(x_hi, x_mx, w_hi, w_mx, mx, *, bias_n=None, want_stats: bool = False):
    """3x3 / stride 1 / pad 1 convolution of the MX operand planes on the halo-tile kernel (include/asis_hip.h:
    asis_conv3x3_halo_mx) -> fp32 NHWC out, or (out, stats [tiles, 2, Cout]) with ``want_stats``."""
    _dev(x_hi, x_mx, w_hi, w_mx, bias_n, mx[0], mx[1])
    Bn, H, W, Cin = x_hi.shape
    Cout = w_hi.shape[0]
    if not (x_hi.is_contiguous() and x_mx.is_contiguous() and w_hi.is_contiguous() and w_mx.is_contiguous() and w_hi.shape[1] == 9 * Cin):
        raise ValueError("conv3x3_halo_mx: contiguous NHWC planes and [Cout, 9 Cin] packed weights expected")
    out = torch.empty((Bn, H, W, Cout), device=x_hi.device, dtype=torch.float32)
    stats = None
    if want_stats:
        stats = torch.empty((lib().asis_conv3x3_halo_mx_tiles(Bn, H, W), 2, Cout), device=x_hi.device, dtype=torch.float32)
    check(lib().asis_conv3x3_halo_mx(_stream(), _dt(x_hi.dtype), x_hi.data_ptr(), x_mx.data_ptr(), w_hi.data_ptr(), w_mx.data_ptr(),
                                     _p(_f32c(bias_n)), mx[0].data_ptr(), mx[1].data_ptr(), out.data_ptr(), _p(stats), Bn, H, W, Cin, Cout),
          "asis_conv3x3_halo_mx")
    return (out, stats) if want_stats else out


def gemm_split(a_hi, a_lo, b_hi, b_lo, *, out: torch.Tensor, bias_n=None):
    """Split-precision ``out = (a_hi + a_lo) @ (b_hi + b_lo).T + bias`` into an fp32 ``out``."""
    M, K, N = a_hi.shape[-2], a_hi.shape[-1], b_hi.shape[-2]
    if _fused_split(M, N, K):
        return gemm(a_hi, b_hi, out=out, bias_n=bias_n, a_lo=a_lo, b_lo=b_lo)
    gemm(a_hi, b_hi, out=out, bias_n=bias_n)
    gemm(a_lo, b_hi, out=out, res=out)
    gemm(a_hi, b_lo, out=out, res=out)
    return out


def ln_fold_supported(M: int, N: int, K: int, batch: int = 1, producer: bool = False) -> bool:
    """True when ``asis_gemm`` dispatches this dense shape to a kernel that implements the LayerNorm-fold epilogue fields (it
    refuses them elsewhere): consumers (``ln=``) the persistent 8-phase kernel or the one-tile-per-workgroup 8-phase form,
    producers (``out_lo`` / ``rowstats`` / ``res16``, unbatched) the latter only.  Follows the dispatcher's switches, the
    run-time ``"p8"`` option included (after ``gemm_set_option("p8", 0)`` a K = 512 consumer is unsupported, as it is in ``asis_gemm``)."""
    return _shape_plan(M, N, K, batch=1 if producer else batch, ln=not producer, producer=producer) is not None


def ln_stats_finalize(rowstats: torch.Tensor, D: int, eps: float = 1e-6) -> torch.Tensor:
    """per-row partial sums of a GEMM epilogue (``gemm(..., rowstats=)``) -> mr fp32 [rows, 2] = (mean, rstd) of nn.LayerNorm
    (8 spare rows behind it: a V^T GEMM with a rounded-up token count reads a few statistics past the last row)"""
    _dev(rowstats)
    rows, groups = rowstats.shape[0], rowstats.shape[1]
    mr = torch.empty((rows + 8, 2), device=rowstats.device, dtype=torch.float32)[:rows]
    check(lib().asis_ln_stats_finalize(_stream(), _f32c(rowstats).data_ptr(), rows, groups, D, float(eps), mr.data_ptr()),
          "asis_ln_stats_finalize")
    return mr


def split_stats(x: torch.Tensor, dtype: torch.dtype, eps: float = 1e-6):
    """fp32 [rows, D] -> (hi, lo 16-bit planes, mr fp32 [rows, 2]): entry into the folded-LayerNorm chain"""
    _dev(x)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("split_stats: x must be float32 [rows, D] contiguous in D")
    rows, D = x.shape
    hi = torch.empty((rows + 8, D), device=x.device, dtype=dtype)[:rows]     # spare rows: Attention.attend_rows reads past the end
    lo = torch.empty((rows, D), device=x.device, dtype=dtype)
    mr = torch.empty((rows + 8, 2), device=x.device, dtype=torch.float32)[:rows]
    check(lib().asis_split_stats(_stream(), _dt(dtype), x.data_ptr(), x.stride(0), hi.data_ptr(), lo.data_ptr(), D, mr.data_ptr(),
                                 rows, D, float(eps)), "asis_split_stats")
    return hi, lo, mr


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-6,
              out_dtype: torch.dtype = T16_DEFAULT, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Row LayerNorm of a float32 [..., D] tensor -> ``out_dtype`` (16-bit GEMM operand or float32)."""
    _dev(x, w, b, out)
    if x.dtype != torch.float32 or x.stride(-1) != 1:
        raise ValueError("layernorm: x must be float32 with a contiguous last dim")
    D = x.shape[-1]
    x2 = x.reshape(-1, D)
    if out is None:
        out = torch.empty(x.shape, device=x.device, dtype=out_dtype)
    o2 = out.view(-1, D)
    f32 = out.dtype == torch.float32
    check(lib().asis_layernorm(_stream(), _dt(out.dtype) if not f32 else 0, x2.data_ptr(), x2.stride(0),
                               _f32c(w).data_ptr(), _f32c(b).data_ptr(), float(eps), o2.data_ptr(), o2.stride(0),
                               int(f32), x2.shape[0], D), "asis_layernorm")
    return out


def layernorm_mx(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, out_dtype: torch.dtype, amax: torch.Tensor):
    """Row LayerNorm of a float32 [rows, D] tensor -> (16-bit output, its MX plane) in one pass; ``amax``: device float, an upper
    bound of |output| (include/asis_hip.h: asis_layernorm_mx)."""
    _dev(x, w, b, amax)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("layernorm_mx: x must be float32 [rows, D] with contiguous columns")
    R, D = x.shape
    hi = torch.empty((R, D), device=x.device, dtype=out_dtype)
    mx = torch.empty_like(hi)
    check(lib().asis_layernorm_mx(_stream(), _dt(out_dtype), x.data_ptr(), x.stride(0), _f32c(w).data_ptr(), _f32c(b).data_ptr(), float(eps),
                                  hi.data_ptr(), mx.data_ptr(), D, amax.data_ptr(), R, D), "asis_layernorm_mx")
    return hi, mx


def _check_out_lo(out: torch.Tensor, out_lo: Optional[torch.Tensor]) -> None:
    if out_lo is not None and (out_lo.shape != out.shape or out_lo.stride() != out.stride() or out_lo.dtype != out.dtype):
        raise ValueError("attention_fwd: out_lo must share the shape, layout and dtype of out")


def _attention_launch(q, k, vt, out, out_lo, B1, N1, B2, N2, H, scale, lse):
    """``scale`` None: q already carries scale * log2(e) (folded into the projection weights) -> the folded kernel"""
    if scale is None:
        check(lib().asis_attention_fwd_prescaled(_stream(), _dt(q.dtype), q.data_ptr(), k.data_ptr(), q.stride(0), vt.data_ptr(),
                                                 vt.stride(1), out.data_ptr(), _p(out_lo), out.stride(0), B1, N1, B2, N2, H,
                                                 _p(lse)), "asis_attention_fwd_prescaled")
    else:
        check(lib().asis_attention_fwd_split(_stream(), _dt(q.dtype), q.data_ptr(), k.data_ptr(), q.stride(0), vt.data_ptr(),
                                             vt.stride(1), out.data_ptr(), _p(out_lo), out.stride(0), B1, N1, B2, N2, H,
                                             float(scale), _p(lse)), "asis_attention_fwd")


def attention_fwd_qkv(qkv: torch.Tensor, segs, H: int, scale: Optional[float], out: torch.Tensor,
                      out_lo: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None,
                      mx_amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """qkv: 16-bit [rows, 3*H*64] = q | k | v of ONE projection GEMM (V row-major: no transposed copy); ``segs`` one or two
    (B, N) token batches stacked along the rows; ``scale`` None = q carries scale * log2(e) (folded projection).
    ``mx_amax`` (device float >= max |v|, e.g. ``absmax16`` of the v columns): ``out_lo`` receives the MX form of the output's lo
    half instead of the 16-bit residual (include/asis_hip.h: asis_attention_fwd_qkv_mx)."""
    _dev(qkv, out, out_lo, lse, mx_amax)
    D = H * 64
    if qkv.dim() != 2 or qkv.shape[1] < 3 * D or qkv.stride(1) != 1 or len(segs) not in (1, 2):
        raise ValueError("attention_fwd_qkv: qkv must be [rows, >= 3*H*64] with contiguous rows, one or two segments")
    (B1, N1), (B2, N2) = (segs[0], segs[1]) if len(segs) == 2 else (segs[0], (0, 0))
    if qkv.shape[0] != B1 * N1 + B2 * N2:
        raise ValueError("attention_fwd_qkv: segments do not cover the rows")
    _check_out_lo(out, out_lo)
    es = qkv.element_size()
    if mx_amax is not None:
        if out_lo is None:
            raise ValueError("attention_fwd_qkv: mx_amax needs the second output plane")
        check(lib().asis_attention_fwd_qkv_mx(_stream(), _dt(qkv.dtype), qkv.data_ptr(), qkv.data_ptr() + D * es,
                                              qkv.data_ptr() + 2 * D * es, qkv.stride(0), out.data_ptr(), out_lo.data_ptr(), out.stride(0),
                                              B1, N1, B2, N2, H, 0.0 if scale is None else float(scale), int(scale is None), _p(lse),
                                              mx_amax.data_ptr()), "asis_attention_fwd_qkv_mx")
        return out
    check(lib().asis_attention_fwd_qkv(_stream(), _dt(qkv.dtype), qkv.data_ptr(), qkv.data_ptr() + D * es,
                                       qkv.data_ptr() + 2 * D * es, qkv.stride(0), out.data_ptr(), _p(out_lo), out.stride(0),
                                       B1, N1, B2, N2, H, 0.0 if scale is None else float(scale), int(scale is None), _p(lse)),
          "asis_attention_fwd_qkv")
    return out


def attention_fwd(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, B: int, H: int, N: int, scale: Optional[float],
                  out: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None,
                  out_lo: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q, k: [B*N, >=H*64] views (same row stride); vt: [B, H*64, ldvt]; returns o [B*N, H*64].
    ``scale`` None = q was produced with scale * log2(e) folded into its projection (``Attention._qkv_folded``).
    ``lse``: optional fp32 [B,H,N] receiving the per-query log2-sum-exp (training forward).
    ``out_lo``: optional tensor laid out like ``out`` receiving the rounding residual of the 16-bit output (o ~= out + out_lo:
    the projection GEMM's split A operand, config.split_attn_out)."""
    _dev(q, k, vt, out, lse, out_lo)
    if q.stride(0) != k.stride(0) or q.stride(1) != 1 or k.stride(1) != 1:
        raise ValueError("attention_fwd: q and k must share a row stride and be contiguous in the last dim")
    if out is None:
        out = torch.empty((B * N, H * 64), device=q.device, dtype=q.dtype)
    if lse is not None and (lse.dtype != torch.float32 or lse.numel() != B * H * N or not lse.is_contiguous()):
        raise ValueError("attention_fwd: lse must be contiguous float32 [B,H,N]")
    _check_out_lo(out, out_lo)
    _attention_launch(q, k, vt, out, out_lo, B, N, 0, 0, H, scale, lse)
    return out


def attention_fwd_seg(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, B1: int, N1: int, B2: int, N2: int, H: int,
                      scale: Optional[float], out: torch.Tensor, out_lo: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Two stacked token batches in one launch: q, k [B1*N1 + B2*N2, >=H*64] row views, vt [B1+B2, H*64, ldvt]."""
    _dev(q, k, vt, out, out_lo)
    _check_out_lo(out, out_lo)
    if q.stride(0) != k.stride(0) or q.stride(1) != 1 or k.stride(1) != 1 or q.shape[0] != B1 * N1 + B2 * N2:
        raise ValueError("attention_fwd_seg: q and k must be row views over both batches with one row stride")
    _attention_launch(q, k, vt, out, out_lo, B1, N1, B2, N2, H, scale, None)
    return out


def token_ld(N: int) -> int:
    """row stride of the token-contiguous (transposed) attention operands: N rounded up to 64"""
    return (N + 63) // 64 * 64


def transpose_tokens(src: torch.Tensor, B: int, N: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """16-bit [B*N, C] view (row stride free) -> [B, C, token_ld(N)], tokens contiguous, zero padded."""
    _dev(src, out)
    Cc = src.shape[1]
    if src.stride(1) != 1 or src.shape[0] != B * N:
        raise ValueError("transpose_tokens: expected a [B*N, C] row view")
    ldt = token_ld(N)
    if out is None:
        out = torch.empty((B, Cc, ldt), device=src.device, dtype=src.dtype)
    check(lib().asis_transpose_tokens(_stream(), _dt(src.dtype), src.data_ptr(), src.stride(0), out.data_ptr(), ldt, B, N,
                                      Cc), "asis_transpose_tokens")
    return out


def attention_bwd_rows(q, k, v, o, dO, lse, segs, H: int, scale: float, dqkv: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> dqkv 16-bit [R, 3*H*64] = [dQ | dK | dV] for one or two stacked token batches ``segs`` = [(B1, N1)] or
    [(B1, N1), (B2, N2)] (rows of batch 2 behind batch 1 in every operand).  q, k, v: [R, H*64] views with one row stride
    (the three column blocks of the qkv projection); o, dO: [R, H*64]; lse: fp32, the forward's log-sum-exp of each batch
    ([B1, H, N1] then [B2, H, N2]) in one contiguous buffer.  No transposed operands (csrc/attn_bwd_pipe.hip)."""
    _dev(q, k, v, o, dO, lse, dqkv)
    Wd = H * 64
    if len(segs) not in (1, 2):
        raise ValueError("attention_bwd_rows: one or two stacked token batches")
    (B1, N1), (B2, N2) = segs[0], (segs[1] if len(segs) == 2 else (0, 0))
    R = B1 * N1 + B2 * N2
    if not (q.stride(0) == k.stride(0) == v.stride(0)) or q.stride(1) != 1 or q.shape[0] != R:
        raise ValueError("attention_bwd_rows: q, k, v must be [R, H*64] views sharing a row stride")
    if lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() != R * H:
        raise ValueError("attention_bwd_rows: lse must be one contiguous float32 buffer of R * H values")
    if dqkv is None:
        dqkv = torch.empty((R, 3 * Wd), device=q.device, dtype=q.dtype)
    D = torch.empty(R * H, device=q.device, dtype=torch.float32)
    es = dqkv.element_size()
    check(lib().asis_attention_bwd_rows(_stream(), _dt(q.dtype), q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0),
                                        o.data_ptr(), o.stride(0), dO.data_ptr(), dO.stride(0), lse.data_ptr(), D.data_ptr(),
                                        dqkv.data_ptr(), dqkv.data_ptr() + Wd * es, dqkv.data_ptr() + 2 * Wd * es,
                                        dqkv.stride(0), B1, N1, B2, N2, H, float(scale)), "asis_attention_bwd_rows")
    return dqkv


def layernorm_bwd(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float = 1e-6,
                  res: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
    """fp32 [R, D] row views -> (dx = res + LN^T(dy), partial fp32 [nblk, 2, D] = (d weight, d bias) sums)."""
    _dev(dy, x, w, res, out)
    R, D = x.shape
    for t in (dy, x, res, out):
        if t is not None and (t.dtype != torch.float32 or t.stride(-1) != 1 or t.shape != x.shape):
            raise ValueError("layernorm_bwd: float32 [R, D] row views of one shape expected")
    if out is None:
        out = torch.empty((R, D), device=x.device, dtype=torch.float32)
    nblk = lib().asis_rowblock_nblk(R)
    partial = torch.empty((nblk, 2, D), device=x.device, dtype=torch.float32)
    check(lib().asis_layernorm_bwd(_stream(), dy.data_ptr(), dy.stride(0), x.data_ptr(), x.stride(0), _f32c(w).data_ptr(),
                                   float(eps), _p(res), res.stride(0) if res is not None else 0, out.data_ptr(),
                                   out.stride(0), partial.data_ptr(), R, D), "asis_layernorm_bwd")
    return out, partial


def gelu16(pre: torch.Tensor, dpost: Optional[torch.Tensor] = None) -> torch.Tensor:
    """16-bit contiguous: gelu(pre), or with dpost the backward dpost * gelu'(pre)."""
    _dev(pre, dpost)
    if not pre.is_contiguous() or (dpost is not None and (not dpost.is_contiguous() or dpost.shape != pre.shape)):
        raise ValueError("gelu16: contiguous operands of one shape expected")
    out = torch.empty_like(pre)
    check(lib().asis_gelu16(_stream(), _dt(pre.dtype), pre.data_ptr(), _p(dpost), out.data_ptr(), pre.numel()), "asis_gelu16")
    return out


def gelu_split(x: torch.Tensor, dtype: torch.dtype, split: bool = True):
    """fp32 contiguous -> (16-bit gelu(x), its rounding residual | None): a split-precision operand pair."""
    _dev(x)
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("gelu_split: contiguous float32 expected")
    hi = torch.empty(x.shape, device=x.device, dtype=dtype)
    lo = torch.empty_like(hi) if split else None
    check(lib().asis_gelu_split(_stream(), _dt(dtype), x.data_ptr(), hi.data_ptr(), _p(lo), x.numel()), "asis_gelu_split")
    return hi, lo


def swiglu_bwd(x12: torch.Tensor, dh: torch.Tensor) -> torch.Tensor:
    """x12 fp32 [R, 2*Hd], dh 16-bit [R, Hd] -> 16-bit [R, 2*Hd] = [d x1 | d x2]."""
    _dev(x12, dh)
    R, H2 = x12.shape
    if dh.shape != (R, H2 // 2) or not dh.is_contiguous():
        raise ValueError("swiglu_bwd: shape mismatch")
    out = torch.empty((R, H2), device=x12.device, dtype=dh.dtype)
    check(lib().asis_swiglu_bwd(_stream(), _dt(dh.dtype), _f32c(x12).data_ptr(), dh.data_ptr(), out.data_ptr(), R, H2 // 2),
          "asis_swiglu_bwd")
    return out


def colsum(x: torch.Tensor) -> torch.Tensor:
    """[R, C] row view (16-bit or float32) -> partial fp32 [nblk, C] column sums (finish with reduce_rows)."""
    _dev(x)
    R, Cc = x.shape
    if x.stride(1) != 1:
        raise ValueError("colsum: rows must be contiguous")
    dt = _lib.ASIS_F32 if x.dtype == torch.float32 else _dt(x.dtype)
    partial = torch.empty((lib().asis_rowblock_nblk(R), Cc), device=x.device, dtype=torch.float32)
    check(lib().asis_colsum(_stream(), dt, x.data_ptr(), x.stride(0), partial.data_ptr(), R, Cc), "asis_colsum")
    return partial


def cast_colsum(x: torch.Tensor, dtype: torch.dtype, scale: float = 1.0):
    """fp32 [R, D] row view -> (16-bit [R, D], partial fp32 [nblk, D] column sums of x) in one pass."""
    _dev(x)
    R, D = x.shape
    if x.dtype != torch.float32 or x.stride(1) != 1:
        raise ValueError("cast_colsum: float32 rows expected")
    out = torch.empty((R, D), device=x.device, dtype=dtype)
    partial = torch.empty((lib().asis_rowblock_nblk(R), D), device=x.device, dtype=torch.float32)
    check(lib().asis_cast_colsum(_stream(), _dt(dtype), x.data_ptr(), x.stride(0), out.data_ptr(), D, float(scale),
                                 partial.data_ptr(), R, D), "asis_cast_colsum")
    return out, partial


# ---- stochastic depth (csrc/droppath.hip): the row kernels above behind a sample indirection.  ``keep`` = a
# droppath.BranchKeep: .tab (int32 device table), .K kept of .S samples, .rows full-stream rows, .rows_c compact rows ------------
def _keep_check(name: str, keep, x: torch.Tensor) -> None:
    _dev(x, keep.tab)
    if keep.tab.dtype != torch.int32 or not keep.tab.is_contiguous() or keep.tab.numel() != 3 * keep.K + 3 * keep.S + 2:
        raise ValueError(f"{name}: keep.tab must be a contiguous int32 table of 3K + 3S + 2 words")
    if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1 or x.shape[0] != keep.rows:
        raise ValueError(f"{name}: float32 [{keep.rows}, D] rows of the full stream expected")


def layernorm_gather(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, out_dtype: torch.dtype, keep) -> torch.Tensor:
    """LayerNorm of the kept samples' rows of the fp32 [R, D] stream -> compact 16-bit [R', D] (``ops.layernorm`` of a gather)."""
    _keep_check("layernorm_gather", keep, x)
    _dev(w, b)
    D = x.shape[1]
    out = torch.empty((keep.rows_c, D), device=x.device, dtype=out_dtype)
    check(lib().asis_layernorm_gather(_stream(), _dt(out_dtype), x.data_ptr(), x.stride(0), _f32c(w).data_ptr(), _f32c(b).data_ptr(),
                                      float(eps), out.data_ptr(), D, keep.tab.data_ptr(), keep.K, keep.S, keep.rows_c, D),
          "asis_layernorm_gather")
    return out


def scaled_index_add(x: torch.Tensor, res: torch.Tensor, keep) -> torch.Tensor:
    """fp32: out [R, D] = x, and x + alpha * res [R', D] on the rows of the kept samples (plain stores: reproducible)."""
    _keep_check("scaled_index_add", keep, x)
    _dev(res)
    D = x.shape[1]
    if res.dtype != torch.float32 or res.shape != (keep.rows_c, D) or res.stride(1) != 1:
        raise ValueError("scaled_index_add: res must be the compact float32 [R', D] branch output")
    out = torch.empty((keep.rows, D), device=x.device, dtype=torch.float32)
    check(lib().asis_scaled_index_add(_stream(), x.data_ptr(), x.stride(0), res.data_ptr() if keep.rows_c else None,
                                      res.stride(0) if keep.rows_c else 0, out.data_ptr(), D, keep.tab.data_ptr(), keep.K, keep.S,
                                      keep.rows, D), "asis_scaled_index_add")
    return out


def gather_cast_colsum(x: torch.Tensor, dtype: torch.dtype, keep, colsum: bool = True):
    """fp32 [R, D] -> (compact 16-bit [R', D] = alpha * x on the kept rows, partial fp32 [nblk(R'), D] column sums of alpha * x, or
    None without ``colsum``): ``cast_colsum`` with the sample's own scale, behind the gather."""
    _keep_check("gather_cast_colsum", keep, x)
    D = x.shape[1]
    out = torch.empty((keep.rows_c, D), device=x.device, dtype=dtype)
    partial = None
    if colsum:
        nblk = lib().asis_rowblock_nblk(keep.rows_c)
        partial = (torch.empty if keep.rows_c else torch.zeros)((nblk, D), device=x.device, dtype=torch.float32)
    check(lib().asis_gather_cast_colsum(_stream(), _dt(dtype), x.data_ptr(), x.stride(0), out.data_ptr() if keep.rows_c else None, D,
                                        _p(partial), keep.tab.data_ptr(), keep.K, keep.S, keep.rows_c, D), "asis_gather_cast_colsum")
    return out, partial


def layernorm_bwd_scatter(dy: torch.Tensor, x: torch.Tensor, w: torch.Tensor, eps: float, res: torch.Tensor, keep):
    """dy fp32 [R', D] (compact), x / res fp32 [R, D] -> (dx [R, D] = res + LN^T(dy) on the kept rows, res elsewhere;
    partial fp32 [nblk(R'), 2, D] = (d weight, d bias) sums over the R' rows)."""
    _keep_check("layernorm_bwd_scatter", keep, x)
    _dev(dy, res, w)
    D = x.shape[1]
    if res.dtype != torch.float32 or res.shape != x.shape or res.stride(1) != 1:
        raise ValueError("layernorm_bwd_scatter: res must be float32 [R, D] like x")
    if dy.dtype != torch.float32 or dy.shape != (keep.rows_c, D) or dy.stride(1) != 1:
        raise ValueError("layernorm_bwd_scatter: dy must be the compact float32 [R', D] gradient")
    out = torch.empty((keep.rows, D), device=x.device, dtype=torch.float32)
    nblk = lib().asis_rowblock_nblk(keep.rows_c)
    partial = (torch.empty if keep.rows_c else torch.zeros)((nblk, 2, D), device=x.device, dtype=torch.float32)   # nothing kept: no partial is written
    check(lib().asis_layernorm_bwd_scatter(_stream(), dy.data_ptr() if keep.rows_c else None, dy.stride(0) if keep.rows_c else 0,
                                           x.data_ptr(), x.stride(0), _f32c(w).data_ptr(), float(eps), res.data_ptr(), res.stride(0),
                                           out.data_ptr(), D, partial.data_ptr(), keep.tab.data_ptr(), keep.K, keep.S, keep.rows,
                                           keep.rows_c, D), "asis_layernorm_bwd_scatter")
    return out, partial


def ls_linear_finish(G: torch.Tensor, W: Optional[torch.Tensor], bias, gamma, cs, grad_scale: float, dW: torch.Tensor,
                     db: Optional[torch.Tensor], dgamma: Optional[torch.Tensor]) -> None:
    """See include/asis_hip.h: (G, cs) -> dW, db, dgamma of ``x + gamma * (A W^T + b)`` (gamma None: plain Linear)."""
    _dev(G, W, bias, gamma, cs, dW, db, dgamma)
    N, K = G.shape
    check(lib().asis_ls_linear_finish(_stream(), _f32c(G).data_ptr(), _p(_f32c(W)), _p(_f32c(bias)), _p(_f32c(gamma)),
                                      _p(_f32c(cs)), float(grad_scale), _f32c(dW).data_ptr(), _p(db), _p(dgamma), N, K),
          "asis_ls_linear_finish")


def im2col_patch(img: torch.Tensor, P: int, ldk: int, dtype: torch.dtype = T16_DEFAULT, split: bool = False):
    """fp32 [B,3,H,W] -> 16-bit [B*(H/P)*(W/P), ldk] (k = c*P*P + i*P + j, pad columns zero); ``split``: -> (hi, lo)."""
    _dev(img)
    if img.dtype != torch.float32 or not img.is_contiguous() or img.dim() != 4 or img.shape[1] != 3:
        raise ValueError("im2col_patch: img must be contiguous float32 [B,3,H,W]")
    B, _, Hi, Wi = img.shape
    if Hi % P or Wi % P:
        # error text mirrors dinov2/layers/patch_embed.py:72-73
        raise AssertionError(f"Input image height {Hi} / width {Wi} is not a multiple of patch size {P}")
    out = torch.empty((B * (Hi // P) * (Wi // P), ldk), device=img.device, dtype=dtype)
    lo = torch.empty_like(out) if split else None
    check(lib().asis_im2col_patch_split(_stream(), _dt(dtype), img.data_ptr(), B, Hi, Wi, P, out.data_ptr(), _p(lo), ldk),
          "asis_im2col_patch")
    return (out, lo) if split else out


def cast_pad(src: torch.Tensor, ld_dst: Optional[int] = None, dtype: torch.dtype = T16_DEFAULT,
             scale: float = 1.0, part: int = 0) -> torch.Tensor:
    """float32 [rows, cols] -> 16-bit [rows, ld_dst] with zero-filled pad columns (weight packing)."""
    _dev(src)
    if src.dtype != torch.float32 or src.dim() != 2 or src.stride(1) != 1:
        raise ValueError("cast_pad: src must be float32 [rows, cols] contiguous in cols")
    rows, cols = src.shape
    ld = ld_dst if ld_dst is not None else (cols + 7) // 8 * 8
    out = torch.empty((rows, ld), device=src.device, dtype=dtype)
    check(lib().asis_cast_pad(_stream(), _dt(dtype), src.data_ptr(), src.stride(0), out.data_ptr(), ld, rows, cols,
                              float(scale), int(part)),
          "asis_cast_pad")
    return out


def add_cls_pos(x: torch.Tensor, cls: torch.Tensor, pos: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [B,N,D] f32, cls [D], pos [N+1,D] -> [B,N+1,D] (vision_transformer.py:196-197)."""
    _dev(x, cls, pos, out)
    B, N, D = x.shape
    if out is None:
        out = torch.empty((B, N + 1, D), device=x.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != (B, N + 1, D) or not out.is_contiguous():
        raise ValueError("add_cls_pos: out must be a contiguous float32 [B, N+1, D] tensor")
    check(lib().asis_add_cls_pos(_stream(), _f32c(x).data_ptr(), _f32c(cls).data_ptr(), _f32c(pos).data_ptr(),
                                 out.data_ptr(), B, N, D), "asis_add_cls_pos")
    return out


# --------------------------------------------------------------------------------------------
# adapters
# --------------------------------------------------------------------------------------------
def msda_fwd(value: torch.Tensor, offaw: torch.Tensor, ref: torch.Tensor, shapes_i32: torch.Tensor,
             starts_i32: torch.Tensor, B: int, Lq: int, M: int, L: int, P: int, split: bool = False):
    """value 16-bit [B, Lin, D]; offaw fp32 [B*Lq, >= M*L*P*3]; ref fp32 [Lq, 2] -> out 16-bit [B*Lq, D]; ``split``: -> (out,
    out_lo) with out_lo the rounding residuals (a split-precision operand pair for output_proj)."""
    _dev(value, offaw, ref, shapes_i32, starts_i32)
    Lin, D = value.shape[1], value.shape[2]
    if not value.is_contiguous() or offaw.stride(1) != 1:
        raise ValueError("msda_fwd: value must be contiguous and offaw contiguous in its last dim")
    out = torch.empty((B * Lq, D), device=value.device, dtype=value.dtype)
    lo = torch.empty_like(out) if split else None
    check(lib().asis_msda_fwd_split(_stream(), _dt(value.dtype), value.data_ptr(), offaw.data_ptr(), offaw.stride(0),
                                    _f32c(ref).data_ptr(), shapes_i32.data_ptr(), starts_i32.data_ptr(), out.data_ptr(), _p(lo), B,
                                    Lq, Lin, M, L, P, D // M), "asis_msda_fwd")
    return (out, lo) if split else out


def dwconv_gelu(x: torch.Tensor, w9: torch.Tensor, bias: torch.Tensor, shapes_i32: torch.Tensor,
                starts_i32: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """x fp32 [B, Ntok, C] -> gelu(dwconv3x3(x)) 16-bit [B, Ntok, C] over the L token grids."""
    _dev(x, w9, bias, shapes_i32, starts_i32)
    B, Ntok, Cc = x.shape
    out = torch.empty((B, Ntok, Cc), device=x.device, dtype=dtype)
    check(lib().asis_dwconv_gelu(_stream(), _dt(dtype), _f32c(x).data_ptr(), _f32c(w9).data_ptr(), _f32c(bias).data_ptr(),
                                 shapes_i32.data_ptr(), starts_i32.data_ptr(), shapes_i32.shape[0], out.data_ptr(), B,
                                 Ntok, Cc), "asis_dwconv_gelu")
    return out


# --------------------------------------------------------------------------------------------
# CNN encoder / decoder companions
# --------------------------------------------------------------------------------------------
_ST_CACHE = {}
# d value of MSDeformAttn as a gather over taps bucketed by destination pixel (round 4); ASIS_MSDA_SORTED=0: the dense sampling
# matrix + batched GEMMs of round 2 (a 2.4 GB matrix at the headline batch)
MSDA_SORTED = os.environ.get("ASIS_MSDA_SORTED", "1") not in ("0", "")


def msda_bwd(value: torch.Tensor, offaw: torch.Tensor, ref: torch.Tensor, shapes_i32: torch.Tensor, starts_i32: torch.Tensor,
             dout: torch.Tensor, B: int, Lq: int, M: int, L: int, P: int, dense: bool = True):
    """value 16-bit [B, Lin, D]; offaw fp32 [B*Lq, M*L*P*3]; dout fp32 [B*Lq, D] ->
    (dvalue fp32 [B, Lin, D], doffaw fp32 like offaw).
    ``dense`` (default): d value through the dense sampling matrix and batched MFMA GEMMs (deterministic);
    otherwise the scatter kernels (LDS tile / global atomics)."""
    _dev(value, offaw, ref, shapes_i32, starts_i32, dout)
    _, Lin, D = value.shape
    Dh = D // M
    doffaw = torch.empty_like(offaw)
    use_dense = dense and Dh % 8 == 0 and D % 64 == 0   # token transpose works on 64-column tiles
    dvalue = torch.empty((B, Lin, D), device=value.device, dtype=torch.float32) if use_dense else \
        zeros((B, Lin, D), value.device)
    check(lib().asis_msda_bwd(_stream(), _dt(value.dtype), value.data_ptr(), _f32c(offaw).data_ptr(), offaw.stride(0),
                              _f32c(ref).data_ptr(), shapes_i32.data_ptr(), starts_i32.data_ptr(), _f32c(dout).data_ptr(),
                              None if use_dense else dvalue.data_ptr(), doffaw.data_ptr(), B, Lq, Lin, M, L, P, Dh),
          "asis_msda_bwd")
    if use_dense and MSDA_SORTED:
        # taps bucketed by destination pixel + one wave per (image, head, pixel) (csrc/adapter_bwd.hip): no dense matrix
        dt = value.dtype
        d16 = cast_pad(dout, D, dt)
        amax = absmax_f32(dout)
        cap = lib().asis_msda_vgrad_cap(Lq, L, P)
        key = ("sorted", B, M, Lin, cap, value.device)
        ws = _ST_CACHE.get(key)
        if ws is None:
            for k in [k for k in _ST_CACHE if k[0] != "sorted"]:
                del _ST_CACHE[k]
            ws = (torch.empty(B * M * Lin, device=value.device, dtype=torch.int32),
                  torch.empty(B * M * (Lin + 1), device=value.device, dtype=torch.int32),
                  torch.empty((B * M * cap, 2), device=value.device, dtype=torch.int32))
            _ST_CACHE[key] = ws
        check(lib().asis_msda_value_grad(_stream(), _dt(dt), offaw.data_ptr(), offaw.stride(0), ref.data_ptr(), shapes_i32.data_ptr(),
                                         starts_i32.data_ptr(), d16.data_ptr(), amax.data_ptr(), ws[0].data_ptr(), ws[1].data_ptr(),
                                         ws[2].data_ptr(), dvalue.data_ptr(), B, Lq, Lin, M, L, P, Dh), "asis_msda_value_grad")
    elif use_dense:
        dt = value.dtype
        ldt = token_ld(Lq)
        key = (B, M, Lin, ldt, dt, value.device)
        ST = _ST_CACHE.get(key)
        if ST is None:
            _ST_CACHE.clear()          # one resident sampling matrix (2.4 GB at B = 12, 588^2): the call shapes alternate
            ST = torch.empty((B * M, Lin, ldt), device=value.device, dtype=dt)
            _ST_CACHE[key] = ST
        check(lib().asis_zero(_stream(), ST.data_ptr(), ST.numel() * ST.element_size()), "asis_zero")
        check(lib().asis_msda_sampling_matrix(_stream(), _dt(dt), offaw.data_ptr(), offaw.stride(0), ref.data_ptr(),
                                              shapes_i32.data_ptr(), starts_i32.data_ptr(), ST.data_ptr(), ldt, B, Lq, Lin, M, L,
                                              P), "asis_msda_sampling_matrix")
        doutT = transpose_tokens(cast_pad(dout, D, dt), B, Lq)                     # [B, D, ldt]
        st4 = ST.view(B, M, Lin, ldt)
        for m in range(M):   # out[b, pix, m*Dh + d] = sum_q ST[b, m, pix, q] * doutT[b, m*Dh + d, q]
            gemm(st4[:, m], doutT[:, m * Dh:(m + 1) * Dh], out=dvalue[:, :, m * Dh:(m + 1) * Dh], out_f32=True)
    return dvalue, doffaw


def dwconv_gelu_bwd(x: torch.Tensor, w9: torch.Tensor, bias: torch.Tensor, shapes_i32: torch.Tensor, starts_i32: torch.Tensor,
                    dy: torch.Tensor, dtype: torch.dtype):
    """x, dy fp32 [B, Ntok, C] -> (dx 16-bit [B, Ntok, C], partial fp32 [nblk, 10, C] = d w9 (9 rows) and d bias)."""
    _dev(x, w9, bias, shapes_i32, starts_i32, dy)
    B, Ntok, Cc = x.shape
    g = torch.empty_like(x)
    partial = torch.empty((lib().asis_dwconv_bwd_nblk(B * Ntok), 10, Cc), device=x.device, dtype=torch.float32)
    dx = torch.empty((B, Ntok, Cc), device=x.device, dtype=dtype)
    check(lib().asis_dwconv_gelu_bwd(_stream(), _dt(dtype), _f32c(x).data_ptr(), _f32c(w9).data_ptr(), _f32c(bias).data_ptr(),
                                     shapes_i32.data_ptr(), starts_i32.data_ptr(), shapes_i32.shape[0], _f32c(dy).data_ptr(),
                                     g.data_ptr(), partial.data_ptr(), dx.data_ptr(), B, Ntok, Cc), "asis_dwconv_gelu_bwd")
    return dx, partial


def conv3x3_c3(img: torch.Tensor, w: torch.Tensor, stride: int, pad: int) -> torch.Tensor:
    _dev(img, w)
    B, _, H, W = img.shape
    Cout = w.shape[0]
    OH, OW = (H + 2 * pad - 3) // stride + 1, (W + 2 * pad - 3) // stride + 1
    out = torch.empty((B, OH, OW, Cout), device=img.device, dtype=torch.float32)
    check(lib().asis_conv3x3_c3(_stream(), _f32c(img).data_ptr(), _f32c(w).data_ptr(), out.data_ptr(), B, H, W, Cout,
                                stride, pad), "asis_conv3x3_c3")
    return out


def conv3x3_smallcout_fwd(x_hi: torch.Tensor, x_lo: Optional[torch.Tensor], w: torch.Tensor,
                          bias: Optional[torch.Tensor]) -> torch.Tensor:
    """Direct fp32 3x3/s1/p1 conv for <= 16 output channels: x (hi [+lo]) 16-bit NHWC, w fp32 [Cout,Cin,3,3]."""
    _dev(x_hi, x_lo, w, bias)
    B, H, W, Cin = x_hi.shape
    Cout = w.shape[0]
    out = torch.empty((B, H, W, Cout), device=x_hi.device, dtype=torch.float32)
    check(lib().asis_conv3x3_smallcout_fwd(_stream(), _dt(x_hi.dtype), x_hi.data_ptr(), _p(x_lo), _f32c(w).data_ptr(),
                                           _p(_f32c(bias)), out.data_ptr(), B, H, W, Cin, Cout),
          "asis_conv3x3_smallcout_fwd")
    return out


# classifier conv with BatchNorm + ReLU + x2 upsampling evaluated on load (csrc/smallconv.hip): OFF by default — it removes 1.4 GB of
# writes and 2.1 GB of reads per step, but the on-load blend costs the two kernels as much as the removed pass took
# (profiles/r04_cls_upsample_on_load_ab.txt: 211.7 / 211.1 img/s without, 211.7 / 211.4 with)
FUSE_CLS_UP = os.environ.get("ASIS_FUSE_CLS_UP", "0") not in ("0", "")


def cls_up_ok(raw: torch.Tensor, Cout: int) -> bool:
    """shapes the upsample-on-load classifier kernels cover (csrc/smallconv.hip): fp32 NHWC raw map with 64 channels, <= 8 classes"""
    return bool(raw.dtype == torch.float32 and raw.dim() == 4 and raw.shape[3] == 64 and raw.is_contiguous()
                and Cout <= 8 and raw.shape[1] >= 4 and raw.shape[2] >= 8)


def conv3x3_smallcout_fwd_up(raw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, w: torch.Tensor,
                             bias: Optional[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """conv3x3(upsample2(relu(raw * scale + shift))) with the upsampled map evaluated on load (include/asis_hip.h:
    asis_conv3x3_smallcout_fwd_up): raw fp32 NHWC [B, H, W, 64] -> fp32 [B, 2H, 2W, Cout]; ``dtype``: the 16-bit operand type."""
    _dev(raw, scale, shift, w, bias)
    B, H, W, Cin = raw.shape
    Cout = w.shape[0]
    out = torch.empty((B, 2 * H, 2 * W, Cout), device=raw.device, dtype=torch.float32)
    check(lib().asis_conv3x3_smallcout_fwd_up(_stream(), _dt(dtype), raw.data_ptr(), _f32c(scale).data_ptr(), _f32c(shift).data_ptr(),
                                              _f32c(w).data_ptr(), _p(_f32c(bias)), out.data_ptr(), B, H, W, Cin, Cout),
          "asis_conv3x3_smallcout_fwd_up")
    return out


def conv3x3_smallcout_wgrad_up(dy: torch.Tensor, raw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, Cout: int,
                               inv_scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """weight gradient of the same fused classifier conv: dy 16-bit [B, 2H, 2W, 8], raw fp32 [B, H, W, 64] -> dW fp32 [Cout, 64, 3, 3]"""
    _dev(dy, raw, scale, shift, out)
    B, H, W, Cin = raw.shape
    if not dy.is_contiguous() or dy.shape[:3] != (B, 2 * H, 2 * W):
        raise ValueError("conv3x3_smallcout_wgrad_up: dy must be contiguous [B, 2H, 2W, CoP]")
    nblk = 1024
    slabs = torch.empty((nblk, Cout * 9 * Cin), device=dy.device, dtype=torch.float32)
    check(lib().asis_conv3x3_smallcout_wgrad_up(_stream(), _dt(dy.dtype), dy.data_ptr(), dy.shape[3], raw.data_ptr(), _f32c(scale).data_ptr(),
                                                _f32c(shift).data_ptr(), slabs.data_ptr(), nblk, B, H, W, Cin, Cout),
          "asis_conv3x3_smallcout_wgrad_up")
    if out is None:
        out = torch.empty((Cout, Cin, 3, 3), device=dy.device, dtype=torch.float32)
    reduce_rows(slabs, inv_scale, out.view(-1))
    return out


# stage-4 tail + classifier with the conv commuted with the x2 upsampling (csrc/clslowres.hip): ON by default — the 64-channel map
# is never written at the classifier's resolution, forward (the 16-bit operand pair) or backward (the fp32 dU);
# ASIS_CLS_LOWRES=0 keeps bn_relu_upsample -> smallcout_fwd / smallcout_dgrad -> upsample_bn_relu_bwd + wgrad
CLS_LOWRES = os.environ.get("ASIS_CLS_LOWRES", "1") not in ("0", "")


def cls_lowres_ok(raw: torch.Tensor, C: int) -> bool:
    """shapes the commuted classifier kernels cover: fp32 NHWC raw map with 64 channels, at least 2 x 2, and 2..4 classes"""
    return bool(raw.dtype == torch.float32 and raw.dim() == 4 and raw.shape[3] == 64 and raw.is_contiguous()
                and 2 <= C <= 4 and raw.shape[1] >= 2 and raw.shape[2] >= 2)


def cls_lowres_fwd(raw: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, w: torch.Tensor,
                   bias: Optional[torch.Tensor]) -> torch.Tensor:
    """conv3x3(upsample2(relu(raw * scale + shift))) + bias, the conv's 1x1 parts evaluated before the upsampling
    (include/asis_hip.h: asis_cls_lowres_fwd): raw fp32 NHWC [B, H, W, 64], w fp32 [C, 64, 3, 3] -> fp32 [B, 2H, 2W, C]."""
    _dev(raw, scale, shift, w, bias)
    B, H, W, Cin = raw.shape
    Cout = w.shape[0]
    z = torch.empty((B, H, 9, W, Cout), device=raw.device, dtype=torch.float32)
    out = torch.empty((B, 2 * H, 2 * W, Cout), device=raw.device, dtype=torch.float32)
    check(lib().asis_cls_lowres_fwd(_stream(), raw.data_ptr(), _f32c(scale).data_ptr(), _f32c(shift).data_ptr(), _f32c(w).data_ptr(),
                                    _p(_f32c(bias)), z.data_ptr(), out.data_ptr(), B, H, W, Cin, Cout), "asis_cls_lowres_fwd")
    return out


def cls_lowres_bwd(d16: torch.Tensor, d_lo: Optional[torch.Tensor], raw: torch.Tensor, scale, shift, mean, invstd, w: torch.Tensor,
                   inv_scale: float = 1.0, out: Optional[torch.Tensor] = None, reduce: bool = True):
    """backward of the same: d16 (+ d_lo) 16-bit [B, 2H, 2W, CP] (loss-scaled) -> (g fp32 [B, H, W, 64], partial [nblk, 2, 64],
    dW fp32 [C, 64, 3, 3] = inv_scale * the reduced slabs).  ``reduce=False``: the third item is the slab tensor [nblk, C*64*9] and
    the caller runs ``reduce_rows(slabs, inv_scale, out)`` itself (on the weight-gradient stream)."""
    _dev(d16, d_lo, raw, w, out)
    B, H, W, Cin = raw.shape
    Cout = w.shape[0]
    if not d16.is_contiguous() or tuple(d16.shape[:3]) != (B, 2 * H, 2 * W) or (d_lo is not None and d_lo.shape != d16.shape):
        raise ValueError("cls_lowres_bwd: d16 / d_lo must be contiguous [B, 2H, 2W, CP]")
    nblk = lib().asis_cls_lowres_nblk(B, H, W)
    g = torch.empty_like(raw)
    partial = torch.empty((nblk, 2, Cin), device=raw.device, dtype=torch.float32)
    slabs = torch.empty((nblk, Cout * Cin * 9), device=raw.device, dtype=torch.float32)
    check(lib().asis_cls_lowres_bwd(_stream(), _dt(d16.dtype), d16.data_ptr(), _p(d_lo), d16.shape[3], raw.data_ptr(),
                                    _f32c(scale).data_ptr(), _f32c(shift).data_ptr(), _f32c(mean).data_ptr(), _f32c(invstd).data_ptr(),
                                    _f32c(w).data_ptr(), g.data_ptr(), partial.data_ptr(), slabs.data_ptr(), nblk, B, H, W, Cin, Cout),
          "asis_cls_lowres_bwd")
    if not reduce:
        return g, partial, slabs
    if out is None:
        out = torch.empty((Cout, Cin, 3, 3), device=raw.device, dtype=torch.float32)
    reduce_rows(slabs, inv_scale, out.view(-1))
    return g, partial, out


# decoder input gradients with the conv commuted with the transposed x2 upsampling of the stage below (csrc/dgradlowres.hip).  The
# switch: a set of stage keys ("d2", "d3", "d4": the conv whose input gradient it is) from ASIS_DGRAD_LOWRES (config.dgrad_lowres),
# or True / False for all / none
DGRAD_LOWRES = config.dgrad_lowres


def dgrad_lowres_on(key: str) -> bool:
    return bool(DGRAD_LOWRES) if isinstance(DGRAD_LOWRES, bool) else key in DGRAD_LOWRES


def dgrad_lowres_ok(Co: int, Ck: int, H: int, W: int) -> bool:
    """shapes asis_dgrad_lowres covers: Co (the conv's output channels) a multiple of 16, Ck (its input channels = the channels of
    the stage below) 128, 256 or 512, the low-resolution map H x W at least 2 x 2"""
    return bool(Co >= 16 and Co % 16 == 0 and Co <= 4096 and Ck in (128, 256, 512) and H >= 2 and W >= 2 and H * W * Co < (1 << 27))


def dgrad_lowres_pack(w: torch.Tensor, dtype: torch.dtype):
    """fp32 conv weight [Co, Ck, 3, 3] -> (hi, lo) 16-bit operand planes of asis_dgrad_lowres: [Co / 16, 5, Ck, 32] each"""
    _dev(w)
    Co, Ck = w.shape[0], w.shape[1]
    if w.dtype != torch.float32 or not w.is_contiguous() or tuple(w.shape[2:]) != (3, 3):
        raise ValueError("dgrad_lowres_pack: contiguous float32 [Co, Ck, 3, 3] expected")
    hi = torch.empty((max(Co // 16, 1), 5, Ck, 32), device=w.device, dtype=dtype)
    lo = torch.empty_like(hi)
    check(lib().asis_dgrad_lowres_pack(_stream(), _dt(dtype), w.data_ptr(), hi.data_ptr(), lo.data_ptr(), Co, Ck),
          "asis_dgrad_lowres_pack")
    return hi, lo


def dgrad_lowres(d16: torch.Tensor, d_lo: Optional[torch.Tensor], wpack, raw: torch.Tensor, scale, shift, mean, invstd):
    """d16 (+ d_lo) 16-bit [B, 2H, 2W, Co]: the output gradient of a 3x3 / pad 1 conv whose input is the x2-upsampled BatchNorm + ReLU
    of ``raw`` fp32 [B, H, W, Ck]; ``wpack`` = dgrad_lowres_pack of its weight -> (g fp32 [B, H, W, Ck], partial [nblk, 2, Ck]), the
    pair ops.upsample_bn_relu_bwd would return for the conv's input gradient (include/asis_hip.h: asis_dgrad_lowres)."""
    _dev(d16, d_lo, raw)
    _not_mx("dgrad_lowres", d_lo)
    B, H, W, Ck = raw.shape
    Co = d16.shape[3]
    w_hi, w_lo = wpack
    if not d16.is_contiguous() or tuple(d16.shape[:3]) != (B, 2 * H, 2 * W) or (d_lo is not None and
                                                                                 (d_lo.shape != d16.shape or not d_lo.is_contiguous())):
        raise ValueError("dgrad_lowres: d16 / d_lo must be contiguous [B, 2H, 2W, Co]")
    if raw.dtype != torch.float32 or not raw.is_contiguous() or w_hi.dtype != d16.dtype or w_hi.numel() != (Co // 16) * 5 * Ck * 32:
        raise ValueError("dgrad_lowres: raw must be contiguous float32 [B, H, W, Ck] and the weight pack that of a [Co, Ck, 3, 3] conv")
    nblk = lib().asis_dgrad_lowres_nblk(B, H, W)
    g = torch.empty_like(raw)
    partial = torch.empty((nblk, 2, Ck), device=raw.device, dtype=torch.float32)
    check(lib().asis_dgrad_lowres(_stream(), _dt(d16.dtype), d16.data_ptr(), _p(d_lo), w_hi.data_ptr(), w_lo.data_ptr(), raw.data_ptr(),
                                  _f32c(scale).data_ptr(), _f32c(shift).data_ptr(), _f32c(mean).data_ptr(), _f32c(invstd).data_ptr(),
                                  g.data_ptr(), partial.data_ptr(), nblk, B, H, W, Co, Ck), "asis_dgrad_lowres")
    return g, partial


def conv3x3_smallcout_dgrad(dy_hi: torch.Tensor, dy_lo: Optional[torch.Tensor], w: torch.Tensor) -> torch.Tensor:
    """Input gradient of the small-Cout conv: dy 16-bit [B,H,W,CoP] (hi [+lo]) -> dx fp32 [B,H,W,Cin]."""
    _dev(dy_hi, dy_lo, w)
    B, H, W, CoP = dy_hi.shape
    Cout, Cin = w.shape[0], w.shape[1]
    dx = torch.empty((B, H, W, Cin), device=dy_hi.device, dtype=torch.float32)
    check(lib().asis_conv3x3_smallcout_dgrad(_stream(), _dt(dy_hi.dtype), dy_hi.data_ptr(), _p(dy_lo), CoP,
                                             _f32c(w).data_ptr(), dx.data_ptr(), B, H, W, Cin, Cout),
          "asis_conv3x3_smallcout_dgrad")
    return dx


def colstats(x: torch.Tensor) -> torch.Tensor:
    """fp32 [..., C] -> partial [nparts, 2, C] column sums / sums of squares."""
    _dev(x)
    Cc = x.shape[-1]
    R = x.numel() // Cc
    nparts = lib().asis_colstats_nparts(R)
    partial = torch.empty((nparts, 2, Cc), device=x.device, dtype=torch.float32)
    check(lib().asis_colstats(_stream(), _f32c(x).data_ptr(), R, Cc, partial.data_ptr()), "asis_colstats")
    return partial


def reduce_partials(partial: torch.Tensor) -> torch.Tensor:
    """partial fp32 [nparts, 2, C] -> sums float64 [2, C]."""
    _dev(partial)
    nparts, _, Cc = partial.shape
    sums = torch.empty((2, Cc), device=partial.device, dtype=torch.float64)
    check(lib().asis_reduce_partials(_stream(), _f32c(partial).data_ptr(), nparts, Cc, sums.data_ptr()),
          "asis_reduce_partials")
    return sums


def bn_finalize(sums: torch.Tensor, count: float, gamma, beta, eps: float, momentum: float, running_mean=None,
                running_var=None, num_batches_tracked=None):
    """-> (scale, shift, mean, invstd) fp32 [C]; updates the running buffers in place when given."""
    _dev(sums, gamma, beta, running_mean, running_var, num_batches_tracked)
    Cc = sums.shape[1]
    out = torch.empty((4, Cc), device=sums.device, dtype=torch.float32)
    check(lib().asis_bn_finalize(_stream(), sums.data_ptr(), float(count), Cc, _p(_f32c(gamma)), _p(_f32c(beta)),
                                 float(eps), float(momentum), _p(running_mean), _p(running_var), _p(num_batches_tracked),
                                 out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr()),
          "asis_bn_finalize")
    return out[0], out[1], out[2], out[3]


class MxPlane(torch.Tensor):
    """The lo half of a split-precision operand in the MX form (two fp8 bytes per element, scaled by the tensor's absolute
    maximum) instead of a 16-bit rounding residual.  The producers (bn_act, bn_relu_upsample, decoder_input, bn_bwd_apply) tag it
    with that maximum (``_asis_mx_amax``); the TYPE survives views, slices and copies, the attribute does not, so a consumer
    that meets an MxPlane without its maximum (``mx_amax_of``), or as a 16-bit lo operand (``_not_mx``), raises instead of
    reading the fp8 pair as an fp16 residual."""

    @staticmethod
    def tag(t: torch.Tensor, amax: torch.Tensor) -> "MxPlane":
        p = t.as_subclass(MxPlane)
        p._asis_mx_amax = amax
        return p


def mx_amax_of(lo: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """the absolute maximum an MX-form lo plane was scaled by; None for a 16-bit residual (or no lo plane at all)"""
    if lo is None:
        return None
    amax = getattr(lo, "_asis_mx_amax", None)
    if amax is None and isinstance(lo, MxPlane):
        raise ValueError("an MX-form lo plane reached its consumer without its absolute maximum (a view / slice / copy of the "
                         "producer's tensor drops the tag): pass the producer's tensor itself")
    return amax


def _not_mx(what: str, *planes) -> None:
    for t in planes:
        if isinstance(t, MxPlane):
            raise ValueError(f"{what}: an MX-form lo plane was passed where a 16-bit rounding residual is expected")


def _lo(out: torch.Tensor, split: bool):
    return torch.empty_like(out) if split else None


def bn_eval_affine(bn) -> tuple:
    """(scale, shift) of an eval-mode nn.BatchNorm2d from its running statistics."""
    Cc = bn.running_mean.numel()
    _dev(bn.running_mean)
    out = torch.empty((2, Cc), device=bn.running_mean.device, dtype=torch.float32)
    check(lib().asis_bn_eval_affine(_stream(), _p(bn.weight.detach() if bn.weight is not None else None),
                                    _p(bn.bias.detach() if bn.bias is not None else None), bn.running_mean.data_ptr(),
                                    bn.running_var.data_ptr(), float(bn.eps), Cc, out[0].data_ptr(), out[1].data_ptr()),
          "asis_bn_eval_affine")
    return out[0], out[1]


def bn_act(x: torch.Tensor, scale, shift, relu: bool, dtype: torch.dtype, split: bool = False, mx_amax: Optional[torch.Tensor] = None):
    """-> out (and (out, out_lo) when split: the two halves of a split-precision operand).  ``mx_amax`` (device float, the output's
    absolute maximum: ``bn_relu_absmax``): the lo half in the MX form, tagged ``_asis_mx_amax`` for the consuming convolution."""
    _dev(x, scale, shift, mx_amax)
    Cc = x.shape[-1]
    out = torch.empty(x.shape, device=x.device, dtype=dtype)
    lo = _lo(out, split)
    if mx_amax is not None and split:
        check(lib().asis_bn_act_mx(_stream(), _dt(dtype), _f32c(x).data_ptr(), scale.data_ptr(), shift.data_ptr(), int(relu),
                                   out.data_ptr(), lo.data_ptr(), mx_amax.data_ptr(), x.numel() // Cc, Cc), "asis_bn_act_mx")
        return out, MxPlane.tag(lo, mx_amax)
    check(lib().asis_bn_act(_stream(), _dt(dtype), _f32c(x).data_ptr(), scale.data_ptr(), shift.data_ptr(), int(relu),
                            out.data_ptr(), _p(lo), x.numel() // Cc, Cc), "asis_bn_act")
    return (out, lo) if split else out


def bn_relu_maxpool(x: torch.Tensor, scale, shift, dtype: torch.dtype, split: bool = False):
    _dev(x, scale, shift)
    B, H, W, Cc = x.shape
    out = torch.empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Cc), device=x.device, dtype=dtype)
    lo = _lo(out, split)
    check(lib().asis_bn_relu_maxpool(_stream(), _dt(dtype), _f32c(x).data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                     out.data_ptr(), _p(lo), B, H, W, Cc), "asis_bn_relu_maxpool")
    return (out, lo) if split else out


def mx_conv_ok(P: int, Cin: int, Cout: int) -> bool:
    """a split 3x3 convolution with P output pixels can take MX lo operands (csrc/gemm.hip: the fused large-tile conv forms)"""
    return _fused_split(P, Cout, Cin)


def absmax_f32(x: torch.Tensor, amax: Optional[torch.Tensor] = None) -> torch.Tensor:
    """|x| maximum of an fp32 tensor whose rows are contiguous ([..., cols] with ONE outer stride) -> device float [1];
    ``amax`` given: accumulate into it (maximum over several tensors)."""
    _dev(x, amax)
    if x.dtype != torch.float32 or x.stride(-1) != 1:
        raise ValueError("absmax_f32: float32 tensor with a contiguous last dim")
    if x.is_contiguous():
        rows, cols, ld = 1, x.numel(), x.numel()
        if cols % 4:
            raise ValueError("absmax_f32: element count must be a multiple of 4")
        if cols >= 1 << 31:    # rows of 2^16 .. 2^20 elements (the kernel's column index is an int)
            cols = next((c for c in (1 << 20, 1 << 18, 1 << 16) if x.numel() % c == 0), x.shape[-1] if x.dim() > 1 else x.numel())
            rows, ld = x.numel() // cols, cols
    elif x.dim() == 3 and x[0].is_contiguous():
        rows, cols, ld = x.shape[0], x.shape[1] * x.shape[2], x.stride(0)
    elif x.dim() == 2:
        rows, cols, ld = x.shape[0], x.shape[1], x.stride(0)
    else:
        raise ValueError("absmax_f32: unsupported layout")
    reset = amax is None
    if amax is None:
        amax = torch.empty(1, device=x.device, dtype=torch.float32)
    check(lib().asis_absmax_f32(_stream(), x.data_ptr(), rows, cols, ld, amax.data_ptr(), int(reset)), "asis_absmax_f32")
    return amax


def bn_relu_absmax(x: torch.Tensor, scale, shift, relu: bool = True) -> torch.Tensor:
    """max of relu(x * scale + shift) over fp32 NHWC x -> device float [1] (the MX scale of the tensor bn_relu_upsample writes)"""
    _dev(x, scale, shift)
    C = x.shape[-1]
    amax = torch.empty(1, device=x.device, dtype=torch.float32)
    check(lib().asis_bn_relu_absmax(_stream(), _f32c(x).data_ptr(), _f32c(scale).data_ptr(), _f32c(shift).data_ptr(), x.numel() // C, C,
                                    int(relu), amax.data_ptr()), "asis_bn_relu_absmax")
    return amax


def bn_relu_upsample(x: torch.Tensor, scale, shift, factor: int, dtype: torch.dtype, split: bool = False, mx_amax=None):
    _dev(x, scale, shift)
    B, H, W, Cc = x.shape
    out = torch.empty((B, H * factor, W * factor, Cc), device=x.device, dtype=dtype)
    lo = _lo(out, split)
    if mx_amax is not None:    # lo in the MX form (two fp8 bytes per element), tagged with the tensor's absolute maximum
        if lo is None:
            raise ValueError("bn_relu_upsample: mx_amax needs split=True")
        check(lib().asis_bn_relu_upsample_mx(_stream(), _dt(dtype), _f32c(x).data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                             out.data_ptr(), lo.data_ptr(), _f32c(mx_amax).data_ptr(), B, H, W, Cc, factor),
              "asis_bn_relu_upsample_mx")
        return out, MxPlane.tag(lo, mx_amax)
    check(lib().asis_bn_relu_upsample(_stream(), _dt(dtype), _f32c(x).data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                      out.data_ptr(), _p(lo), B, H, W, Cc, factor), "asis_bn_relu_upsample")
    return (out, lo) if split else out


def pack_conv_weight(w: torch.Tensor, mode: int, dtype: torch.dtype, part: int = 0) -> torch.Tensor:
    """fp32 [Cout,Cin,KH,KW] -> mode 0: [Cout, KH*KW*Cin]; mode 1 (dgrad): [Cin, KH*KW*CoP].
    part=1 returns the rounding residual (second half of a split-precision operand)."""
    _dev(w)
    Cout, Cin, KH, KW = w.shape
    CoP = (Cout + 7) // 8 * 8
    rows, K = (Cout, KH * KW * Cin) if mode == 0 else (Cin, KH * KW * CoP)
    ld = (K + 7) // 8 * 8
    out = torch.empty((rows, ld), device=w.device, dtype=dtype)
    check(lib().asis_pack_conv_weight(_stream(), _dt(dtype), _f32c(w).data_ptr(), out.data_ptr(), Cout, Cin, KH, KW,
                                      mode, ld, int(part)), "asis_pack_conv_weight")
    return out[:, :K] if ld != K else out


def absmax16(x: torch.Tensor) -> torch.Tensor:
    """|x| maximum of a 16-bit [rows, cols] tensor (contiguous columns, cols % 8 == 0) -> device float [1]"""
    _dev(x)
    if x.dtype not in (torch.float16, torch.bfloat16) or x.dim() != 2 or x.stride(1) != 1:
        raise ValueError("absmax16: 16-bit [rows, cols] tensor with contiguous columns")
    amax = torch.empty(1, device=x.device, dtype=torch.float32)
    check(lib().asis_absmax_16(_stream(), _dt(x.dtype), x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), amax.data_ptr()), "asis_absmax_16")
    return amax


def mx_from_pair(hi: torch.Tensor, lo: torch.Tensor, wside: bool = False, amax: Optional[torch.Tensor] = None):
    """(hi, lo) 16-bit planes of a split-precision operand -> (its MX plane with the layout of ``hi``, amax [1]): the ``a_lo`` /
    ``b_lo`` (``wside``) + ``mx`` operands of a dense ``gemm`` (include/asis_hip.h: asis_mx_from_pair)."""
    _dev(hi, lo, amax)
    if hi.dtype != lo.dtype or hi.dim() != 2 or hi.stride() != lo.stride() or hi.stride(1) != 1 or hi.shape != lo.shape:
        raise ValueError("mx_from_pair: two 16-bit [rows, cols] planes with equal layout")
    if amax is None:
        amax = absmax16(hi)
    out = torch.empty_strided(hi.shape, hi.stride(), device=hi.device, dtype=hi.dtype) if hi.stride(0) != hi.shape[1] else torch.empty_like(hi)
    check(lib().asis_mx_from_pair(_stream(), _dt(hi.dtype), hi.data_ptr(), lo.data_ptr(), hi.stride(0), out.data_ptr(), out.stride(0),
                                  hi.shape[0], hi.shape[1], amax.data_ptr(), int(wside)), "asis_mx_from_pair")
    return out, amax


def pack_conv_weight_mx(w: torch.Tensor, mode: int, dtype: torch.dtype):
    """-> (MX form of the weight's lo operand (weight side: (lo8, hi8) per element), same shape as pack_conv_weight's, and the
    weight's absolute maximum as a device float [1])"""
    _dev(w)
    Cout, Cin, KH, KW = w.shape
    CoP = (Cout + 7) // 8 * 8
    rows, K = (Cout, KH * KW * Cin) if mode == 0 else (Cin, KH * KW * CoP)
    ld = (K + 7) // 8 * 8
    wf = _f32c(w)
    amax = absmax_f32(wf.view(Cout, -1) if (Cin * KH * KW) % 4 == 0 else wf.view(1, -1))
    out = torch.empty((rows, ld), device=w.device, dtype=dtype)
    check(lib().asis_pack_conv_weight_mx(_stream(), _dt(dtype), wf.data_ptr(), out.data_ptr(), Cout, Cin, KH, KW, mode, ld,
                                         amax.data_ptr()), "asis_pack_conv_weight_mx")
    return (out[:, :K] if ld != K else out), amax


def conv_weight_absmax(w: torch.Tensor) -> torch.Tensor:
    """absolute maximum of an OIHW fp32 convolution weight -> device float [1] (the MX planes' scale)"""
    wf = _f32c(w)
    return absmax_f32(wf.view(w.shape[0], -1) if (wf.numel() // w.shape[0]) % 4 == 0 else wf.view(1, -1))


def pack_conv_weight_pair(w: torch.Tensor, mode: int, dtype: torch.dtype, mx: bool = False, amax: Optional[torch.Tensor] = None):
    """-> (16-bit weight, its lo operand, amax | None) in ONE pass over the fp32 weight: lo = the rounding residual, or (``mx``)
    the MX form scaled by the weight's absolute maximum (``amax`` if the caller holds it, else one reduction pass).  Same
    layouts as ``pack_conv_weight``."""
    _dev(w, amax)
    Cout, Cin, KH, KW = w.shape
    CoP = (Cout + 7) // 8 * 8
    rows, K = (Cout, KH * KW * Cin) if mode == 0 else (Cin, KH * KW * CoP)
    ld = (K + 7) // 8 * 8
    wf = _f32c(w)
    if mx and amax is None:
        amax = conv_weight_absmax(wf)
    elif not mx:
        amax = None
    hi = torch.empty((rows, ld), device=w.device, dtype=dtype)
    lo = torch.empty((rows, ld), device=w.device, dtype=dtype)
    check(lib().asis_pack_conv_weight_pair(_stream(), _dt(dtype), wf.data_ptr(), hi.data_ptr(), lo.data_ptr(), Cout, Cin, KH, KW, mode, ld,
                                           _p(amax)), "asis_pack_conv_weight_pair")
    if ld != K:
        hi, lo = hi[:, :K], lo[:, :K]
    return hi, lo, amax


def _rows3(t: torch.Tensor, D: int, what: str):
    if t.dtype != torch.float32 or t.dim() != 3 or t.stride(2) != 1 or t.stride(1) != D:
        raise ValueError(f"{what}: expected float32 [B, n, {D}] with contiguous rows (batch stride free)")


def decoder_input(xs: torch.Tensor, c4: torch.Tensor, vit: torch.Tensor, hw, c4_hw, dtype: torch.dtype,
                  split: bool = False, mx: bool = False):
    """train.py:389-406: xs, vit fp32 [B, h*w, D]; c4 fp32 [B, h4*w4, D] (batch strides free) -> [B,h,w,3D]."""
    _dev(xs, c4, vit)
    B, _, D = xs.shape
    h, w = hw
    h4, w4 = c4_hw
    for t, n in ((xs, "xs"), (c4, "c4"), (vit, "vit")):
        _rows3(t, D, "decoder_input " + n)
    out = torch.empty((B, h, w, 3 * D), device=xs.device, dtype=dtype)
    lo = _lo(out, split)
    if mx and split:           # lo in the MX form: one absolute maximum over the three sources
        amax = absmax_f32(xs)
        absmax_f32(c4, amax)
        absmax_f32(vit, amax)
        check(lib().asis_decoder_input_mx(_stream(), _dt(dtype), xs.data_ptr(), xs.stride(0), c4.data_ptr(), c4.stride(0),
                                          vit.data_ptr(), vit.stride(0), out.data_ptr(), lo.data_ptr(), amax.data_ptr(), B, h, w,
                                          h4, w4, D), "asis_decoder_input_mx")
        return out, MxPlane.tag(lo, amax)
    check(lib().asis_decoder_input(_stream(), _dt(dtype), xs.data_ptr(), xs.stride(0), c4.data_ptr(), c4.stride(0),
                                   vit.data_ptr(), vit.stride(0), out.data_ptr(), _p(lo), B, h, w, h4, w4, D),
          "asis_decoder_input")
    return (out, lo) if split else out


def swiglu_rows(Hd: int, device) -> torch.Tensor:
    """row order of w12 (and its bias) for the ACT_SILU_MUL epilogue of ``gemm``: groups of 16 x1 rows followed by the 16 x2 rows
    of the same hidden columns (include/asis_hip.h) -> int64 [2 * Hd]"""
    if Hd % 16:
        raise ValueError("swiglu_rows: the hidden width must be a multiple of 16")
    g = torch.arange(Hd, device=device).view(Hd // 16, 1, 16)
    return torch.cat((g, g + Hd), 1).reshape(-1)


def swiglu_fused_ok(M: int, Hd: int, K: int, split: bool, mx: bool) -> bool:
    """shapes / operand forms the SwiGLU epilogue covers: ``asis_gemm`` takes an ASIS_ACT_SILU_MUL launch of them (include/asis_hip.h),
    under the dispatcher's switches as they stand; ASIS_SWIGLU_FUSED=0: never"""
    return _SWIGLU_FUSED and _shape_plan(M, 2 * Hd, K, act=ACT_SILU_MUL, split=split, mx=mx) is not None


_SWIGLU_FUSED = os.environ.get("ASIS_SWIGLU_FUSED", "1") not in ("0", "")


def swiglu(x12: torch.Tensor, dtype: torch.dtype, split: bool = False):
    """fp32 [R, 2*Hd] = [x1 | x2] -> 16-bit [R, Hd] = silu(x1) * x2 (dinov2/layers/swiglu_ffn.py:30-34); ``split``: -> (hi, lo)
    with lo the rounding residual (a split-precision operand pair)."""
    _dev(x12)
    R, two = x12.shape
    out = torch.empty((R, two // 2), device=x12.device, dtype=dtype)
    lo = torch.empty_like(out) if split else None
    check(lib().asis_swiglu_split(_stream(), _dt(dtype), _f32c(x12).data_ptr(), out.data_ptr(), _p(lo), R, two // 2), "asis_swiglu")
    return (out, lo) if split else out


def copy_channels(src: torch.Tensor, dst: torch.Tensor) -> None:
    """dst[..., :] = src[..., :] for 2-D views [rows, C] whose rows are contiguous but strided (concat / split)."""
    _dev(src, dst)
    if src.dim() != 2 or dst.dim() != 2 or src.shape != dst.shape or src.stride(1) != 1 or dst.stride(1) != 1 \
            or src.dtype != dst.dtype:
        raise ValueError("copy_channels: expected matching 2-D row views")
    es = src.element_size()
    check(lib().asis_copy_channels(_stream(), src.data_ptr(), src.stride(0) * es, dst.data_ptr(), dst.stride(0) * es,
                                   src.shape[0], src.shape[1] * es), "asis_copy_channels")


def add_f32(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a + b for float32 [B, n, D] tensors with contiguous rows and free batch strides."""
    _dev(a, b, out)
    B, n, D = a.shape
    if out is None:
        out = torch.empty((B, n, D), device=a.device, dtype=torch.float32)
    for t, nm in ((a, "a"), (b, "b"), (out, "out")):
        _rows3(t, D, "add_f32 " + nm)
    check(lib().asis_add_f32(_stream(), a.data_ptr(), b.data_ptr(), out.data_ptr(), n * D, B, a.stride(0), b.stride(0),
                             out.stride(0)), "asis_add_f32")
    return out


# --------------------------------------------------------------------------------------------
# loss
# --------------------------------------------------------------------------------------------
def maxpool2_fwd(x: torch.Tensor, x_lo: Optional[torch.Tensor], save_idx: bool = True):
    """MaxPool2d(2) on a split-precision NHWC map: (hi, lo|None) [B,H,W,C] -> (hi, lo|None) [B,H/2,W/2,C], idx uint8."""
    _dev(x, x_lo)
    _not_mx("maxpool2_fwd", x_lo)
    B, H, W, Cc = x.shape
    if not x.is_contiguous() or (x_lo is not None and (not x_lo.is_contiguous() or x_lo.shape != x.shape)):
        raise ValueError("maxpool2_fwd: contiguous NHWC operands of one shape expected")
    out = torch.empty((B, H // 2, W // 2, Cc), device=x.device, dtype=x.dtype)
    out_lo = torch.empty_like(out) if x_lo is not None else None
    idx = torch.empty((B, H // 2, W // 2, Cc), device=x.device, dtype=torch.uint8) if save_idx else None
    check(lib().asis_maxpool2_fwd(_stream(), _dt(x.dtype), x.data_ptr(), _p(x_lo), out.data_ptr(), _p(out_lo), _p(idx), B, H,
                                  W, Cc), "asis_maxpool2_fwd")
    return out, out_lo, idx


def maxpool2_bwd(dy: torch.Tensor, idx: torch.Tensor, dx: torch.Tensor) -> torch.Tensor:
    """dx fp32 [B,H,W,C] += scatter of dy fp32 [B,H/2,W/2,C] at the saved argmax."""
    _dev(dy, idx, dx)
    B, H, W, Cc = dx.shape
    if dy.shape != (B, H // 2, W // 2, Cc) or idx.shape != dy.shape or not dx.is_contiguous():
        raise ValueError("maxpool2_bwd: shape mismatch")
    check(lib().asis_maxpool2_bwd(_stream(), _f32c(dy).data_ptr(), idx.data_ptr(), _f32c(dx).data_ptr(), B, H, W, Cc),
          "asis_maxpool2_bwd")
    return dx



def cls_l2norm(x: torch.Tensor, B: int, N: int, C: int):
    """class rows of the stacked fp32 [B*(N+C), D] matrix -> (chat fp32 [B,C,D] = x / ||x||, inv_c fp32 [B*C])."""
    _dev(x)
    D = x.shape[1]
    if x.dtype != torch.float32 or not x.is_contiguous() or x.shape[0] != B * (N + C):
        raise ValueError("cls_l2norm: contiguous float32 [B*(N+C), D] expected")
    chat = torch.empty((B, C, D), device=x.device, dtype=torch.float32)
    inv = torch.empty((B * C,), device=x.device, dtype=torch.float32)
    check(lib().asis_cls_l2norm(_stream(), x.data_ptr(), chat.data_ptr(), inv.data_ptr(), B, N, C, D), "asis_cls_l2norm")
    return chat, inv


def cls_l2norm_bwd(dchat: torch.Tensor, chat: torch.Tensor, inv_c: torch.Tensor, dx: torch.Tensor, N: int) -> None:
    """writes the class rows of dx (stacked fp32 [B*(N+C), D]); the patch rows are left as they are."""
    _dev(dchat, chat, inv_c, dx)
    B, C, D = chat.shape
    if dx.dtype != torch.float32 or not dx.is_contiguous() or tuple(dx.shape) != (B * (N + C), D) or dchat.shape != chat.shape:
        raise ValueError("cls_l2norm_bwd: shape mismatch")
    check(lib().asis_cls_l2norm_bwd(_stream(), _f32c(dchat).data_ptr(), chat.data_ptr(), inv_c.data_ptr(), dx.data_ptr(), B, N, C, D),
          "asis_cls_l2norm_bwd")


def mask_logits_fwd(P: torch.Tensor, chat: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, N: int):
    """stacked P fp32 [B*(N+C), D] (patch rows), chat [B,C,D] -> (logits fp32 [B*N, C] = LayerNorm_C(cosines), cosm, inv_p)."""
    _dev(P, chat, gamma, beta)
    B, C, D = chat.shape
    if P.dtype != torch.float32 or not P.is_contiguous() or tuple(P.shape) != (B * (N + C), D):
        raise ValueError("mask_logits_fwd: contiguous float32 [B*(N+C), D] expected")
    logits = torch.empty((B * N, C), device=P.device, dtype=torch.float32)
    cosm = torch.empty((B * N, C), device=P.device, dtype=torch.float32)
    inv_p = torch.empty((B * N,), device=P.device, dtype=torch.float32)
    check(lib().asis_mask_logits_fwd(_stream(), P.data_ptr(), chat.data_ptr(), _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(),
                                     float(eps), logits.data_ptr(), cosm.data_ptr(), inv_p.data_ptr(), B, N, C, D),
          "asis_mask_logits_fwd")
    return logits, cosm, inv_p


def mask_logits_bwd(dlogits: torch.Tensor, cosm: torch.Tensor, inv_p: torch.Tensor, P: torch.Tensor, chat: torch.Tensor,
                    gamma: torch.Tensor, eps: float, dP: torch.Tensor, N: int):
    """-> (dcos fp32 [B*N, C], partial fp32 [nblk, 2, C]); writes the patch rows of dP (stacked, same shape as P)."""
    _dev(dlogits, cosm, inv_p, P, chat, gamma, dP)
    B, C, D = chat.shape
    if dP.shape != P.shape or dP.dtype != torch.float32 or not dP.is_contiguous() or tuple(dlogits.shape) != (B * N, C):
        raise ValueError("mask_logits_bwd: shape mismatch")
    dcos = torch.empty((B * N, C), device=P.device, dtype=torch.float32)
    part = torch.empty((lib().asis_mask_logits_nblk(B, N), 2, C), device=P.device, dtype=torch.float32)
    check(lib().asis_mask_logits_bwd(_stream(), _f32c(dlogits).data_ptr(), cosm.data_ptr(), inv_p.data_ptr(), P.data_ptr(),
                                     chat.data_ptr(), _f32c(gamma).data_ptr(), float(eps), dP.data_ptr(), dcos.data_ptr(),
                                     part.data_ptr(), B, N, C, D), "asis_mask_logits_bwd")
    return dcos, part


def mask_dchat(dcos: torch.Tensor, P: torch.Tensor, inv_p: torch.Tensor, B: int, N: int, C: int) -> torch.Tensor:
    _dev(dcos, P, inv_p)
    D = P.shape[1]
    out = torch.empty((B, C, D), device=P.device, dtype=torch.float32)
    check(lib().asis_mask_dchat(_stream(), dcos.data_ptr(), P.data_ptr(), inv_p.data_ptr(), out.data_ptr(), B, N, C, D),
          "asis_mask_dchat")
    return out


def nearest_tables(src: int, dst: int, device) -> tuple:
    """F.interpolate(mode='nearest') index tables for one axis: (src index of every dst index int32 [dst], first dst index of
    every src index int32 [src + 1]).  ATen (UpSample.h nearest_idx): identity when equal, dst >> 1 for an exact doubling,
    else min(floor(dst_index * float32(src / dst)), src - 1) in float32 arithmetic."""
    import numpy as np
    d = np.arange(dst, dtype=np.int64)
    if dst == src:
        idx = d
    elif dst == 2 * src:
        idx = d >> 1
    else:
        scale = np.float32(src) / np.float32(dst)
        idx = np.minimum(np.floor(d.astype(np.float32) * scale).astype(np.int64), src - 1)
    first = np.searchsorted(idx, np.arange(src + 1), side="left")
    return (torch.from_numpy(idx.astype(np.int32)).to(device), torch.from_numpy(first.astype(np.int32)).to(device))


def nearest_add_relu(x: torch.Tensor, x_lo: Optional[torch.Tensor], r: torch.Tensor, r_lo: Optional[torch.Tensor],
                     ys: torch.Tensor, xs: torch.Tensor) -> None:
    """x (+x_lo) 16-bit NHWC [B,H,W,C] <- relu(x + nearest-resized r [B,h,w,C]) in place (FCUUp + FusionModel)."""
    _dev(x, x_lo, r, r_lo, ys, xs)
    B, H, W, C = x.shape
    _, h, w, Cr = r.shape
    if Cr != C or r.shape[0] != B or ys.numel() != H or xs.numel() != W or ys.dtype != torch.int32 or xs.dtype != torch.int32:
        raise ValueError("nearest_add_relu: shape / table mismatch")
    if not (x.is_contiguous() and r.is_contiguous()) or r.dtype != x.dtype:
        raise ValueError("nearest_add_relu: contiguous maps of one 16-bit dtype expected")
    check(lib().asis_nearest_add_relu(_stream(), _dt(x.dtype), x.data_ptr(), _p(x_lo), r.data_ptr(), _p(r_lo), ys.data_ptr(),
                                      xs.data_ptr(), B, H, W, h, w, C), "asis_nearest_add_relu")


def nearest_sum(g: torch.Tensor, h: int, w: int, y0: torch.Tensor, x0: torch.Tensor) -> torch.Tensor:
    """Transpose of the nearest resize: g fp32 [B,H,W,C] -> fp32 [B,h,w,C] (sums over each source pixel's destination block)."""
    _dev(g, y0, x0)
    B, H, W, C = g.shape
    if g.dtype != torch.float32 or not g.is_contiguous() or y0.numel() != h + 1 or x0.numel() != w + 1:
        raise ValueError("nearest_sum: fp32 contiguous gradient and [h+1] / [w+1] int32 tables expected")
    out = torch.empty((B, h, w, C), device=g.device, dtype=torch.float32)
    check(lib().asis_nearest_sum(_stream(), g.data_ptr(), out.data_ptr(), y0.data_ptr(), x0.data_ptr(), B, H, W, h, w, C),
          "asis_nearest_sum")
    return out

def convt2x2_scatter(G: torch.Tensor, dst: torch.Tensor, dst_lo: Optional[torch.Tensor], B: int, H: int, W: int, coff: int,
                     padT: int = 0, padL: int = 0) -> None:
    """G fp32 [B*H*W, 4*Cout] (ConvTranspose2d k=2 s=2 as a GEMM) -> channels [coff, coff+Cout) of the NHWC 16-bit
    buffer(s) dst [B,H2,W2,Ctot] at pixel offset (padT, padL)."""
    _dev(G, dst, dst_lo)
    Cout = G.shape[1] // 4
    _, H2, W2, Ctot = dst.shape
    if G.shape[0] != B * H * W or not dst.is_contiguous():
        raise ValueError("convt2x2_scatter: shape mismatch")
    check(lib().asis_convt2x2_scatter(_stream(), _dt(dst.dtype), _f32c(G).data_ptr(), dst.data_ptr(), _p(dst_lo), B, H, W,
                                      Cout, H2, W2, Ctot, coff, padT, padL), "asis_convt2x2_scatter")


def conv1x1_dgrad_small(d_hi: torch.Tensor, d_lo: Optional[torch.Tensor], w: torch.Tensor, C: int) -> torch.Tensor:
    """input gradient of a 1x1 convolution with C <= 8 output channels: (d_hi + d_lo)[M, :C] @ w[C, Cq] -> fp32 [M, Cq]"""
    _dev(d_hi, d_lo, w)
    _not_mx("conv1x1_dgrad_small", d_lo)
    M, ldd = d_hi.shape[0], d_hi.stride(0)
    Cq = w.shape[1]
    if d_hi.dim() != 2 or d_hi.stride(1) != 1 or (d_lo is not None and (d_lo.stride() != d_hi.stride() or d_lo.dtype != d_hi.dtype)) \
            or w.dtype != torch.float32 or w.shape[0] != C or not w.is_contiguous():
        raise ValueError("conv1x1_dgrad_small: d_hi / d_lo 16-bit [M, >= C] row views with one layout, w contiguous float32 [C, Cq]")
    out = torch.empty((M, Cq), device=d_hi.device, dtype=torch.float32)
    check(lib().asis_conv1x1_dgrad_small(_stream(), _dt(d_hi.dtype), d_hi.data_ptr(), _p(d_lo), ldd, w.data_ptr(), out.data_ptr(), M, Cq, C),
          "asis_conv1x1_dgrad_small")
    return out


def convt2x2_gather(dcat: torch.Tensor, B: int, H: int, W: int, Cout: int, coff: int, padT: int, padL: int,
                    dtype: torch.dtype, split: bool):
    """d cat fp32 [B,H2,W2,Ctot] -> (dG hi, dG lo|None 16-bit [B*H*W, 4*Cout], d bias partial sums fp32 [nblk, Cout])."""
    _dev(dcat)
    _, H2, W2, Ctot = dcat.shape
    dG = torch.empty((B * H * W, 4 * Cout), device=dcat.device, dtype=dtype)
    dG_lo = torch.empty_like(dG) if split else None
    check(lib().asis_convt2x2_gather(_stream(), _dt(dtype), _f32c(dcat).data_ptr(), dG.data_ptr(), _p(dG_lo), B, H, W, Cout,
                                     H2, W2, Ctot, coff, padT, padL), "asis_convt2x2_gather")
    nblk = lib().asis_convt2x2_bias_nblk(B * 4 * H * W)
    partial = torch.empty((nblk, Cout), device=dcat.device, dtype=torch.float32)
    check(lib().asis_convt2x2_bias_grad(_stream(), dcat.data_ptr(), partial.data_ptr(), B, H, W, Cout, H2, W2, Ctot, coff,
                                        padT, padL), "asis_convt2x2_bias_grad")
    return dG, dG_lo, partial


LOSS_DICE, LOSS_IOU, LOSS_SOFTDICE, LOSS_TVERSKY, LOSS_NONE = 0, 1, 2, 3, 4
LOSS_LOVASZ = 5  # not a mode of asis_seg_loss_fwd: the engines route it to lovasz_softmax (asis_lovasz_softmax)
LOSS_TOPK, LOSS_FOCAL = 6, 7  # likewise: routed to hardpixel_loss (asis_hardpixel_loss), kind 0 / kind 1


def seg_loss_fwd(logits: torch.Tensor, target: torch.Tensor, n_region: int, mode: int = LOSS_DICE, eps: float = 1e-19,
                 n_ce: int = 0, ce_weight: Optional[torch.Tensor] = None, grad_scale: float = 1.0):
    """logits fp32 NHWC [B,h,w,C]; target int64 [B,H,W] -> (loss [1], coef [B*C*2+1], sums [B,C,3]).
    Region term `mode` on softmax^n_region(resize(logits)) plus (n_ce > 0) the cross entropy of
    log softmax(softmax^(n_ce-1)(resize(logits))) — see include/asis_hip.h for the reference losses each case is."""
    _dev(logits, target, ce_weight)
    B, h, w, Cc = logits.shape
    H, W = target.shape[-2:]
    if target.dtype != torch.int64 or not target.is_contiguous():
        raise ValueError("seg_loss_fwd: target must be contiguous int64 [B,H,W]")
    if ce_weight is not None and (ce_weight.numel() != Cc or ce_weight.dtype != torch.float32):
        raise ValueError("seg_loss_fwd: ce_weight must be float32 [C]")
    nblk = lib().asis_dice_nblk(H, W)
    partial = torch.empty((B, nblk, Cc * 3 + 2), device=logits.device, dtype=torch.float32)
    sums = torch.empty((B, Cc, 3), device=logits.device, dtype=torch.float32)
    loss = torch.empty((1,), device=logits.device, dtype=torch.float32)
    coef = torch.empty((B * Cc * 2 + 1,), device=logits.device, dtype=torch.float32)
    check(lib().asis_seg_loss_fwd(_stream(), _f32c(logits).data_ptr(), target.data_ptr(), _p(_f32c(ce_weight)), B, h, w, H, W,
                                  Cc, int(n_region), int(mode), float(eps), int(n_ce), float(grad_scale), partial.data_ptr(),
                                  sums.data_ptr(), loss.data_ptr(), coef.data_ptr()), "asis_seg_loss_fwd")
    return loss, coef, sums


def seg_loss_bwd(logits: torch.Tensor, target: torch.Tensor, coef: torch.Tensor, n_region: int, mode: int = LOSS_DICE,
                 n_ce: int = 0, ce_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> dz fp32 [B,H,W,C] = d loss / d resized logits (times the grad_scale given to the forward)."""
    _dev(logits, target, coef, ce_weight)
    B, h, w, Cc = logits.shape
    H, W = target.shape[-2:]
    if coef.numel() != B * Cc * 2 + 1:
        raise ValueError("seg_loss_bwd: coef must be the B*C*2+1 floats of seg_loss_fwd")
    dz = torch.empty((B, H, W, Cc), device=logits.device, dtype=torch.float32)
    check(lib().asis_seg_loss_bwd(_stream(), _f32c(logits).data_ptr(), target.data_ptr(), coef.data_ptr(),
                                  _p(_f32c(ce_weight)), B, h, w, H, W, Cc, int(n_region), int(mode), int(n_ce),
                                  dz.data_ptr()), "asis_seg_loss_bwd")
    return dz


def seg_loss_ignore(logits: torch.Tensor, target: torch.Tensor, ignore_index: int, n_region: int, mode: int = LOSS_DICE,
                    eps: float = 1e-19, n_ce: int = 0, ce_weight: Optional[torch.Tensor] = None, grad_scale: float = 1.0):
    """``seg_loss_fwd`` + ``seg_loss_bwd`` with an ignore label, in one call (csrc/semi.hip, libasis_semi.so; include/asis_semi.h
    states the semantics): pixels whose label is ``ignore_index`` (an int outside 0..C-1) take part in no sum and get a dz of
    exactly 0, their logits are not read; a sample without a valid pixel is left out of the mean of the region term.
    -> (loss [1], dz fp32 [B,H,W,C] (times grad_scale), valid int32 [B] = the valid pixels per sample, sums fp32 [B,C,3])."""
    from . import _lib_semi
    op = "seg_loss_ignore"
    _dev(logits, target, ce_weight)
    B, h, w, Cc = logits.shape
    H, W = target.shape[-2:]
    if target.dtype != torch.int64 or not target.is_contiguous():
        raise ValueError(f"{op}: target must be contiguous int64 [B,H,W]")
    if ce_weight is not None and (ce_weight.numel() != Cc or ce_weight.dtype != torch.float32):
        raise ValueError(f"{op}: ce_weight must be float32 [C]")
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or 0 <= ignore_index < Cc \
            or not -2 ** 31 <= ignore_index < 2 ** 31:
        raise ValueError(f"{op}: ignore_index={ignore_index!r} must be an int outside the classes 0..{Cc - 1}")
    semi = _lib_semi.lib()
    nblk = lib().asis_dice_nblk(H, W)
    dev = logits.device
    partial = torch.empty((B, nblk, semi.asis_semi_partial_stride(Cc)), device=dev, dtype=torch.float32)
    sums = torch.empty((B, Cc, 3), device=dev, dtype=torch.float32)
    loss = torch.empty((1,), device=dev, dtype=torch.float32)
    coef = torch.empty((B * Cc * 2 + 1,), device=dev, dtype=torch.float32)
    valid = torch.empty((B,), device=dev, dtype=torch.int32)
    dz = torch.empty((B, H, W, Cc), device=dev, dtype=torch.float32)
    check(semi.asis_semi_loss(_stream(), _f32c(logits).data_ptr(), target.data_ptr(), _p(_f32c(ce_weight)), B, h, w, H, W, Cc,
                              ignore_index, int(n_region), int(mode), float(eps), int(n_ce), float(grad_scale), partial.data_ptr(),
                              sums.data_ptr(), loss.data_ptr(), coef.data_ptr(), valid.data_ptr(), dz.data_ptr()), "asis_semi_loss")
    return loss, dz, valid, sums


def dice_fwd(logits: torch.Tensor, target: torch.Tensor, n_softmax: int, eps: float = 1e-19, grad_scale: float = 1.0,
             mode: int = 0):
    """Region-only shorthand: mode 0 = Dice (segloss/dice.py), mode 1 = soft IoU (segloss/iou_multi.py, eps = smooth)."""
    return seg_loss_fwd(logits, target, n_softmax, mode, eps, 0, None, grad_scale)


def ce_acc(logits: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor] = None, counts: bool = False):
    """logits fp32 NHWC [B,h,w,C], target int64 [B,H,W] -> fp32 [3] = (sum w*nll, sum w, #correct); with ``counts``
    also int32 [C,3] = #(target == c), #(argmax == c), #(both) (the inputs of ch_iou / isi_iou)."""
    _dev(logits, target, weight)
    B, h, w, Cc = logits.shape
    H, W = target.shape[-2:]
    nblk = lib().asis_ce_acc_nblk(B * H * W)
    partial = torch.empty((nblk, 3), device=logits.device, dtype=torch.float32)
    cnt = torch.empty((Cc, 3), device=logits.device, dtype=torch.int32) if counts else None
    check(lib().asis_ce_acc_counts(_stream(), _f32c(logits).data_ptr(), target.data_ptr(), _p(_f32c(weight)), B, h, w, H, W,
                                   Cc, partial.data_ptr(), _p(cnt)), "asis_ce_acc")
    red = reduce_rows(partial)
    return (red, cnt) if counts else red


def dice_bwd(logits: torch.Tensor, target: torch.Tensor, coef: torch.Tensor, n_softmax: int) -> torch.Tensor:
    return seg_loss_bwd(logits, target, coef, n_softmax, LOSS_DICE, 0, None)


def resize_bilinear_fwd(x: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """fp32 NHWC [B,h,w,C] -> [B,H,W,C], F.interpolate(mode="bilinear", align_corners=False)."""
    _dev(x)
    B, h, w, Cc = x.shape
    out = torch.empty((B, H, W, Cc), device=x.device, dtype=torch.float32)
    check(lib().asis_resize_bilinear_fwd(_stream(), _f32c(x).data_ptr(), B, h, w, H, W, Cc, out.data_ptr()),
          "asis_resize_bilinear_fwd")
    return out


def resize_bilinear_bwd(dz: torch.Tensor, h: int, w: int, dtype: torch.dtype, split: bool = False):
    """dz fp32 [B,H,W,C] -> (d 16-bit [B,h,w,CP], partial [nblk, C]) (+ d_lo inserted second when split)."""
    _dev(dz)
    B, H, W, Cc = dz.shape
    f32 = dtype == torch.float32
    CP = Cc if f32 else (Cc + 7) // 8 * 8
    nblk = lib().asis_resize_bwd_nblk(B * h * w)
    out = torch.empty((B, h, w, CP), device=dz.device, dtype=dtype)
    partial = torch.empty((nblk, Cc), device=dz.device, dtype=torch.float32)
    lo = _lo(out, split and not f32)
    check(lib().asis_resize_bilinear_bwd(_stream(), 2 if f32 else _dt(dtype), _f32c(dz).data_ptr(), B, H, W, h, w, Cc, CP,
                                         out.data_ptr(), _p(lo), partial.data_ptr()), "asis_resize_bilinear_bwd")
    return (out, lo, partial) if split else (out, partial)


def reduce_rows(partial: torch.Tensor, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """partial fp32 [n, K] -> out fp32 [K] = scale * column sums (double accumulate, fixed order)."""
    _dev(partial, out)
    n, K = partial.shape[0], partial.numel() // partial.shape[0]
    if out is None:
        out = torch.empty((K,), device=partial.device, dtype=torch.float32)
    check(lib().asis_reduce_rows(_stream(), _f32c(partial).data_ptr(), n, K, float(scale), out.data_ptr()),
          "asis_reduce_rows")
    return out


LOVASZ_REDUCTIONS = {"mean": 0, "sum": 1, "none": 2}


def _pixel_loss_args(op: str, logits: torch.Tensor, target: torch.Tensor, need, dz, scratch):
    """The argument checks and buffers ``lovasz_softmax`` and ``hardpixel_loss`` share: logits NHWC against an int64 target,
    the scratch (``need(N, C)`` bytes; checked, or a fresh one) and dz (checked and added into, or a fresh one).
    -> (B, h, w, H, W, C, N, scratch, dz, accumulate)"""
    if logits.dim() != 4 or target.dim() != 3:
        raise ValueError(f"{op}: logits must be NHWC [B,h,w,C] and target [B,H,W]")
    B, h, w, Cc = logits.shape
    H, W = target.shape[-2:]
    if target.dtype != torch.int64 or not target.is_contiguous() or target.shape[0] != B:
        raise ValueError(f"{op}: target must be contiguous int64 [B,H,W]")
    return (B, h, w, H, W, Cc) + _pixel_loss_buffers(op, logits, H, W, need, dz, scratch)


def _pixel_loss_buffers(op: str, logits: torch.Tensor, H: int, W: int, need, dz, scratch):
    """The scratch / dz convention of the per-pixel losses for logits NHWC [B,h,w,C] evaluated at H x W -> (N, scratch, dz, accumulate)"""
    B, Cc = logits.shape[0], logits.shape[3]
    N = B * H * W
    nbytes = need(N, Cc)
    if scratch is None:
        scratch = torch.empty((nbytes,), device=logits.device, dtype=torch.uint8)
    elif scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < nbytes:
        raise ValueError(f"{op}: scratch must be a contiguous uint8 buffer of at least {nbytes} bytes")
    accumulate = dz is not None
    if dz is None:
        dz = torch.empty((B, H, W, Cc), device=logits.device, dtype=torch.float32)
    elif tuple(dz.shape) != (B, H, W, Cc) or dz.dtype != torch.float32 or not dz.is_contiguous():
        raise ValueError(f"{op}: dz must be contiguous float32 [B,H,W,C]")
    return N, scratch, dz, accumulate


def lovasz_scratch_bytes(n_pixels: int, num_classes: int) -> int:
    """bytes of caller-owned scratch ``asis_lovasz_softmax`` needs for ``n_pixels`` = B*H*W (needs no GPU)."""
    nb = lib().asis_lovasz_scratch_bytes(int(n_pixels), int(num_classes))
    if nb < 0:
        check(int(nb), "asis_lovasz_scratch_bytes")
    return int(nb)


def lovasz_softmax(logits: torch.Tensor, target: torch.Tensor, n_softmax: int = 1, reduction: str = "mean",
                   grad_scale: float = 1.0, dz: Optional[torch.Tensor] = None, return_order: bool = False,
                   scratch: Optional[torch.Tensor] = None):
    """Lovasz-Softmax (`segloss/lovasz_loss.py:39-60`) of softmax^n_softmax(resize(logits)) against the labels, forward and
    gradient in one call.  logits fp32 NHWC [B,h,w,C]; target int64 [B,H,W] -> (loss [1], per_class [C], dz fp32 [B,H,W,C]) with
    dz = grad_scale * d loss / d resized logits; a given ``dz`` is added into (and returned).  reduction "none": the losses are
    ``per_class``, ``loss`` is their sum and dz the gradient of that sum.  ``return_order`` appends keys fp32 [C,N] (the errors
    in pixel order) and order int32 [C,N] (pixel index at each sorted position: descending error, ties by ascending index).
    ``scratch``: a uint8 buffer of at least ``lovasz_scratch_bytes(B*H*W, C)`` to reuse between calls (default: a fresh one)."""
    _dev(logits, target, dz, scratch)
    if reduction not in LOVASZ_REDUCTIONS:
        raise ValueError(f"lovasz_softmax: reduction must be one of {sorted(LOVASZ_REDUCTIONS)}")
    B, h, w, H, W, Cc, N, scratch, dz, accumulate = _pixel_loss_args("lovasz_softmax", logits, target, lovasz_scratch_bytes, dz,
                                                                     scratch)
    loss = torch.empty((1,), device=logits.device, dtype=torch.float32)
    per_class = torch.empty((Cc,), device=logits.device, dtype=torch.float32)
    keys = torch.empty((Cc, N), device=logits.device, dtype=torch.float32) if return_order else None
    order = torch.empty((Cc, N), device=logits.device, dtype=torch.int32) if return_order else None
    check(lib().asis_lovasz_softmax(_stream(), _f32c(logits).data_ptr(), target.data_ptr(), B, h, w, H, W, Cc, int(n_softmax),
                                    LOVASZ_REDUCTIONS[reduction], float(grad_scale), int(accumulate), scratch.data_ptr(),
                                    loss.data_ptr(), per_class.data_ptr(), dz.data_ptr(), _p(keys), _p(order)),
          "asis_lovasz_softmax")
    return (loss, per_class, dz, keys, order) if return_order else (loss, per_class, dz)


HARDPIXEL_CE, HARDPIXEL_FOCAL = 0, 1


def hardpixel_scratch_bytes(n_pixels: int) -> int:
    """bytes of caller-owned scratch ``asis_hardpixel_loss`` needs for ``n_pixels`` = B*H*W (needs no GPU)."""
    nb = lib().asis_hardpixel_scratch_bytes(int(n_pixels))
    if nb < 0:
        check(int(nb), "asis_hardpixel_scratch_bytes")
    return int(nb)


def hardpixel_loss(logits: torch.Tensor, target: torch.Tensor, kind: int, K: int, *, n_softmax: int = 0, gamma: float = 2.0,
                   smooth: float = 1e-5, class_weight: Optional[torch.Tensor] = None, size_average: bool = True,
                   grad_scale: float = 1.0, dz: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None,
                   return_selection: bool = False):
    """Mean (``size_average``) or sum of the ``K`` largest per-pixel losses of the whole batch, forward and gradient in one call:
    ``kind`` 0 the cross entropy of resize(logits) (`segloss/ND_Crossentropy.py:34-47`, K = int(N k / 100)), 1 the focal loss of
    softmax^n_softmax(resize(logits)) (`segloss/focal_loss.py:7-91`, K = N).  logits fp32 NHWC [B,h,w,C]; target int64 [B,H,W];
    ``class_weight`` fp32 [C] (the cross-entropy weight / the focal alpha) -> (loss [1], dz fp32 [B,H,W,C]) with
    dz = grad_scale * d loss / d resized logits, exactly 0 on pixels that are not selected; a given ``dz`` is added into on the
    selected ones (and returned).  ``return_selection`` appends (values fp32 [N], selected uint8 [N]).  Ties at the K-th value go
    to the lower pixel index.  ``scratch``: a uint8 buffer of at least ``hardpixel_scratch_bytes(B*H*W)`` to reuse between calls
    (default: a fresh one).  No host sync."""
    _dev(logits, target, class_weight, dz, scratch)
    B, h, w, H, W, Cc, N, scratch, dz, accumulate = _pixel_loss_args("hardpixel_loss", logits, target,
                                                                     lambda n, c: hardpixel_scratch_bytes(n), dz, scratch)
    if class_weight is not None and (class_weight.numel() != Cc or class_weight.dtype != torch.float32):
        raise ValueError("hardpixel_loss: class_weight must be float32 [C]")
    if not 1 <= int(K) <= N:
        raise ValueError(f"hardpixel_loss: K={K} must be in 1..B*H*W={N}")
    loss = torch.empty((1,), device=logits.device, dtype=torch.float32)
    values = torch.empty((N,), device=logits.device, dtype=torch.float32) if return_selection else None
    selected = torch.empty((N,), device=logits.device, dtype=torch.uint8) if return_selection else None
    check(lib().asis_hardpixel_loss(_stream(), _f32c(logits).data_ptr(), target.data_ptr(), _p(_f32c(class_weight)), B, h, w, H, W,
                                    Cc, int(kind), int(n_softmax), float(gamma), float(smooth), int(K), int(bool(size_average)),
                                    float(grad_scale), int(accumulate), scratch.data_ptr(), loss.data_ptr(), dz.data_ptr(),
                                    _p(values), _p(selected)), "asis_hardpixel_loss")
    return (loss, dz, values, selected) if return_selection else (loss, dz)


DISTILL_MAX_VIEWS = 8


def _soft_scratch_bytes(binding, nblk_fn: str, n_pixels: int, doubles: int) -> int:
    """``doubles`` doubles per workgroup of the side library ``binding`` (loaded on first use, beside libasis_hip.so)"""
    nb = getattr(binding.lib(), nblk_fn)(int(n_pixels))
    if nb < 0:
        check(int(nb), nblk_fn)
    return 8 * doubles * int(nb)


def distill_scratch_bytes(n_pixels: int) -> int:
    """bytes of caller-owned scratch ``asis_distill_loss`` needs for ``n_pixels`` = B*H*W: one double per workgroup (needs no GPU)."""
    from . import _lib_distill
    return _soft_scratch_bytes(_lib_distill, "asis_distill_nblk", n_pixels, 1)


def distill_loss(logits: torch.Tensor, teacher_logits, size_or_target, *, flips=None, temperature: float = 1.0,
                 grad_scale: float = 1.0, dz: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None):
    """Knowledge distillation in one pass (csrc/distill.hip, libasis_distill.so): the KL divergence of the student from the mean distribution of a
    teacher's views, forward and gradient.  ``logits`` fp32 NHWC [B,h,w,C] (the student); ``teacher_logits`` a tensor or a list of
    1..8 contiguous fp32 NHWC maps [B,h_k,w_k,C], each of its own size; ``flips[k]`` true = map k was predicted from the mirrored
    frame and is read through mirrored columns (bit for bit the un-mirrored map ``v.flip(2)``, as in ``predict_mask_views``; None =
    no map is).  ``size_or_target``: (H, W), an int, or a tensor whose last two dimensions are H, W (the target of the hard loss).
    Per native pixel: p = softmax(resize(logits) / T), q = mean_k softmax(resize(teacher_k) / T), T = ``temperature``;
    -> (loss [1] = T^2 mean_pixels KL(q || p), dz fp32 [B,H,W,C] = grad_scale (T / N) (p - q) = grad_scale * d loss / d resized
    logits); a given ``dz`` is added into (and returned).  Nothing else of size [B,H,W,C] is written however many maps there are.
    ``scratch``: a uint8 buffer of at least ``distill_scratch_bytes(B*H*W)`` to reuse between calls (default: a fresh one).
    No host sync; bit-identical from call to call."""
    from . import _lib_distill
    op = "distill_loss"
    B, h, w, V, H, W, Cc, dev, ptrs, hs, ws, fl = _distill_args(op, logits, teacher_logits, size_or_target, flips, temperature, dz,
                                                                scratch)
    N, scratch, dz, accumulate = _pixel_loss_buffers(op, logits, H, W, lambda n, c: distill_scratch_bytes(n), dz, scratch)
    loss = torch.empty((1,), device=dev, dtype=torch.float32)
    check(_lib_distill.lib().asis_distill_loss(_stream(), logits.data_ptr(), B, h, w, ptrs, hs, ws, fl, V, H, W, Cc, float(temperature),
                                  float(grad_scale), int(accumulate), scratch.data_ptr(), loss.data_ptr(), dz.data_ptr()),
          "asis_distill_loss")
    return loss, dz


def _distill_args(op: str, logits, teacher_logits, size_or_target, flips, temperature, dz, scratch):
    """The argument checks ``distill_loss`` and ``consistency_loss`` share: the student, the teacher maps, their flips, the size
    and the temperature -> (B, h, w, V, H, W, C, device, ptrs, hs, ws, flips): the last four are the ctypes arrays of the ABI."""
    import ctypes
    maps = [teacher_logits] if torch.is_tensor(teacher_logits) else teacher_logits
    V, B, Cc, dev, ptrs, hs, ws = _predict_maps(op, "views", DISTILL_MAX_VIEWS, maps)
    flips = [False] * V if flips is None else [bool(f) for f in flips]
    if len(flips) != V:
        raise ValueError(f"{op}: flips has {len(flips)} entries for {V} teacher maps")
    if not torch.is_tensor(logits) or logits.dim() != 4 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError(f"{op}: logits must be a contiguous float32 NHWC tensor [B,h,w,C]")
    if logits.shape[0] != B or logits.shape[3] != Cc or logits.device != dev:
        raise ValueError(f"{op}: logits are {list(logits.shape)} on {logits.device}, the teacher maps have B={B}, C={Cc} on {dev}")
    if not float(temperature) > 0.0:
        raise ValueError(f"{op}: temperature={temperature} must be > 0")
    if torch.is_tensor(size_or_target):
        size = tuple(size_or_target.shape[-2:])
    else:
        size = (size_or_target, size_or_target) if isinstance(size_or_target, int) else tuple(size_or_target)
    if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
        raise ValueError(f"{op}: size must be a positive int, (H, W) or a tensor [..., H, W], got {size_or_target!r}")
    _dev(logits, maps[0], dz, scratch)
    fl = (ctypes.c_int * V)(*[int(f) for f in flips])
    return B, int(logits.shape[1]), int(logits.shape[2]), V, int(size[0]), int(size[1]), Cc, dev, ptrs, hs, ws, fl


def consistency_scratch_bytes(n_pixels: int) -> int:
    """bytes of caller-owned scratch ``asis_consist_loss`` needs for ``n_pixels`` = B*H*W: two doubles per workgroup (needs no GPU)."""
    from . import _lib_consist
    return _soft_scratch_bytes(_lib_consist, "asis_consist_nblk", n_pixels, 2)


def consistency_loss(logits: torch.Tensor, teacher_logits, size_or_target, *, flips=None, temperature: float = 1.0,
                     threshold: Optional[float] = None, sample_weight: Optional[torch.Tensor] = None, grad_scale: float = 1.0,
                     dz: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None, mix=None,
                     class_threshold: Optional[torch.Tensor] = None):
    """The consistency term of teacher-student training in one pass (csrc/consist.hip, libasis_consist.so): ``distill_loss`` with a
    per-pixel confidence gate, a per-sample weight and the count of the pixels the gate let through.  ``logits``,
    ``teacher_logits``, ``size_or_target``, ``flips``, ``temperature`` as there.  ``threshold`` (None or <= 0: every pixel is
    kept; at most 1): a pixel takes part where conf = max_c q_c >= threshold, q the teacher's mean distribution at THIS
    temperature.  ``sample_weight``: fp32 [B] on the device, finite and >= 0 (not checked on the device); None = all 1.
    -> (loss [1] = T^2 sum_i w_b m_i KL_i(q || p) / N, normalised by N = B*H*W and not by the kept count; kept int32 [1] = the
    pixels with m_i = 1 in samples with w_b > 0; dz fp32 [B,H,W,C] = grad_scale (T / N) w_b m_i (p - q)).  A fresh ``dz`` holds
    zeros on the dropped pixels; a given ``dz`` is added into on the kept pixels and neither read nor written on the others (and
    returned).  A sample of weight 0 reads none of its maps.  ``scratch``: a uint8 buffer of at least
    ``consistency_scratch_bytes(B*H*W)`` to reuse between calls (default: a fresh one).  No host sync; bit-identical from call to
    call.
    ``mix`` = (sel, donor) (default None: the call above, libasis_mix.so is not opened): the loss over a batch mixed by
    ``mix_batch`` (csrc/mix.hip).  ``sel`` contiguous uint8 [B,H,W] on the logits' device; ``donor`` a host int32 tensor or a
    sequence of B samples in 0..B-1 (checked here, on the host).  For pixel i of sample b every teacher map is read from sample
    donor[b] where sel[i] is set and from b elsewhere, at the same (y, x) and through the same flips; the student, the weight, the
    gate (on the confidence of the mixed q), kept, N and dz are as above.
    ``class_threshold`` (default None: the call above, libasis_adapt.so is not opened; not together with ``threshold``): a contiguous
    fp32 [C] tensor on the logits' device, one threshold per class (csrc/adapt.hip).  A pixel takes part where conf >=
    class_threshold[a], a = the class that holds conf (the lowest index among equal values); an entry <= 0 keeps every pixel of
    its class, one above 1 drops them all.  With or without ``mix``; a tensor filled with t gives the bits of ``threshold=t``."""
    op = "consistency_loss"
    if class_threshold is not None and threshold is not None:
        raise ValueError(f"{op}: threshold and class_threshold exclude each other")
    if class_threshold is not None and (not torch.is_tensor(class_threshold) or class_threshold.dtype != torch.float32
                                        or class_threshold.dim() != 1 or not class_threshold.is_contiguous()):
        raise ValueError(f"{op}: class_threshold must be a contiguous float32 tensor [C]")
    B, h, w, V, H, W, Cc, dev, ptrs, hs, ws, fl = _distill_args(op, logits, teacher_logits, size_or_target, flips, temperature, dz,
                                                                scratch)
    thr = 0.0 if threshold is None else float(threshold)
    if not thr <= 1.0:
        raise ValueError(f"{op}: threshold={threshold} must be at most 1 (None or <= 0 keeps every pixel)")
    if sample_weight is not None:
        _dev(sample_weight)
        if sample_weight.dtype != torch.float32 or not sample_weight.is_contiguous() or tuple(sample_weight.shape) != (B,) \
                or sample_weight.device != dev:
            raise ValueError(f"{op}: sample_weight must be a contiguous float32 tensor [B={B}] on {dev}")
    gate = thr
    if class_threshold is not None:
        _dev(class_threshold)
        if tuple(class_threshold.shape) != (Cc,) or class_threshold.device != dev:
            raise ValueError(f"{op}: class_threshold must be a contiguous float32 tensor [C={Cc}] on {dev}")
        gate = class_threshold.data_ptr()
    if mix is None:
        if class_threshold is None:
            from . import _lib_consist as binding
            nblk, entry, gather = "asis_consist_nblk", "asis_consist_loss", ()
        else:
            from . import _lib_adapt as binding
            nblk, entry, gather = "asis_adapt_nblk", "asis_adapt_consist_loss", ()
    else:
        if class_threshold is None:
            from . import _lib_mix as binding
            nblk, entry = "asis_mix_consist_nblk", "asis_mix_consist_loss"
        else:
            from . import _lib_adapt as binding
            nblk, entry = "asis_adapt_nblk", "asis_adapt_mix_consist_loss"
        sel, donor = _mix_gate_args(op, mix, B, H, W, dev)
        gather = (sel.data_ptr(), donor.data_ptr())
    N, scratch, dz, accumulate = _pixel_loss_buffers(op, logits, H, W, lambda n, c: _soft_scratch_bytes(binding, nblk, n, 2), dz,
                                                     scratch)
    if scratch.data_ptr() % 8:
        raise ValueError(f"{op}: scratch must be 8-byte aligned")
    loss = torch.empty((1,), device=dev, dtype=torch.float32)
    kept = torch.empty((1,), device=dev, dtype=torch.int32)
    check(getattr(binding.lib(), entry)(_stream(), logits.data_ptr(), B, h, w, ptrs, hs, ws, fl, V, H, W, Cc, float(temperature), gate,
                                        _p(sample_weight), *gather, float(grad_scale), int(accumulate), scratch.data_ptr(),
                                        loss.data_ptr(), kept.data_ptr(), dz.data_ptr()), entry)
    return loss, kept, dz


# --------------------------------------------------------------------------------------------
# class-adaptive thresholds of the consistency term (csrc/adapt.hip, libasis_adapt.so)
# --------------------------------------------------------------------------------------------
ADAPT_MAX_CLASSES = 16


def confidence_stats_scratch_bytes(n_pixels: int) -> int:
    """bytes of caller-owned scratch ``asis_adapt_stats`` needs for ``n_pixels`` = B*H*W at any class count: C + 2 <= 18 doubles
    per workgroup (needs no GPU)."""
    from . import _lib_adapt
    return _soft_scratch_bytes(_lib_adapt, "asis_adapt_stats_nblk", n_pixels, ADAPT_MAX_CLASSES + 2)


def confidence_stats(teacher_logits, size_or_target, *, flips=None, temperature: float = 1.0,
                     sample_weight: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                     scratch: Optional[torch.Tensor] = None) -> torch.Tensor:
    """What the adaptive thresholds follow (csrc/adapt.hip, libasis_adapt.so): over the native pixels of the samples with
    ``sample_weight[b]`` > 0 (None: every sample; each pixel counts 1 whatever the weight's size), with q the teacher's mean
    distribution as ``consistency_loss`` forms it from ``teacher_logits``, ``size_or_target``, ``flips``, ``temperature``:
    -> float64 [C + 2] on the device = S_0..S_{C-1} (S_c = sum_i q_i[c]), S_conf = sum_i max_c q_i[c], cnt = the pixels counted.
    A sample of weight 0 reads none of its maps.  ``out``: a contiguous float64 [C + 2] tensor to write (and return); ``scratch``: a
    uint8 buffer of at least ``confidence_stats_scratch_bytes(B*H*W)``, 8-byte aligned (default: a fresh one).  No host sync, no
    atomics: bit-identical from call to call."""
    import ctypes
    from . import _lib_adapt
    op = "confidence_stats"
    maps = [teacher_logits] if torch.is_tensor(teacher_logits) else teacher_logits
    V, B, Cc, dev, ptrs, hs, ws = _predict_maps(op, "views", DISTILL_MAX_VIEWS, maps)
    if not 1 <= Cc <= ADAPT_MAX_CLASSES:
        raise ValueError(f"{op}: C={Cc} must be in 1..{ADAPT_MAX_CLASSES}")
    flips = [False] * V if flips is None else [bool(f) for f in flips]
    if len(flips) != V:
        raise ValueError(f"{op}: flips has {len(flips)} entries for {V} teacher maps")
    if not float(temperature) > 0.0:
        raise ValueError(f"{op}: temperature={temperature} must be > 0")
    if torch.is_tensor(size_or_target):
        size = tuple(size_or_target.shape[-2:])
    else:
        size = (size_or_target, size_or_target) if isinstance(size_or_target, int) else tuple(size_or_target)
    if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
        raise ValueError(f"{op}: size must be a positive int, (H, W) or a tensor [..., H, W], got {size_or_target!r}")
    H, W = int(size[0]), int(size[1])
    if sample_weight is not None and (not torch.is_tensor(sample_weight) or sample_weight.dtype != torch.float32 or not sample_weight.is_contiguous()
                                      or tuple(sample_weight.shape) != (B,) or sample_weight.device != dev):
        raise ValueError(f"{op}: sample_weight must be a contiguous float32 tensor [B={B}] on {dev}")
    if out is not None and (out.dtype != torch.float64 or not out.is_contiguous() or tuple(out.shape) != (Cc + 2,) or out.device != dev):
        raise ValueError(f"{op}: out must be a contiguous float64 tensor [C + 2 = {Cc + 2}] on {dev}")
    _dev(maps[0], sample_weight, out, scratch)
    nbytes = confidence_stats_scratch_bytes(B * H * W)
    if scratch is None:
        scratch = torch.empty((nbytes,), device=dev, dtype=torch.uint8)
    elif scratch.dtype != torch.uint8 or not scratch.is_contiguous() or scratch.numel() < nbytes or scratch.device != dev \
            or scratch.data_ptr() % 8:
        raise ValueError(f"{op}: scratch must be a contiguous, 8-byte aligned uint8 buffer of at least {nbytes} bytes on {dev}")
    if out is None:
        out = torch.empty((Cc + 2,), device=dev, dtype=torch.float64)
    fl =(ctypes.c_int * V)(*[int(f) for f in flips])
    check(_lib_adapt.lib().asis_adapt_stats(_stream(), B, ptrs, hs, ws, fl, V, H, W, Cc, float(temperature), _p(sample_weight),
                                            scratch.data_ptr(), out.data_ptr()), "asis_adapt_stats")
    return out


def adaptive_threshold_update(sums: torch.Tensor, state: torch.Tensor, thr: torch.Tensor, momentum: float = 0.999) -> torch.Tensor:
    """One step of self-adaptive thresholding on the device (csrc/adapt.hip): ``sums`` float64 [C + 2] as ``confidence_stats``
    gives them, ``state`` float64 [C + 2] = tau, n_updates, ptilde[C] (updated in place), ``thr`` fp32 [C] (written; returned).  With
    cnt = sums[C + 1] > 0: tau <- m tau + (1 - m) S_conf / cnt, ptilde_c <- m ptilde_c + (1 - m) S_c / cnt, thr_c = fp32(tau
    ptilde_c / max ptilde); with cnt == 0 state and thr keep their bits.  ``momentum`` m in [0, 1).  No host sync."""
    from . import _lib_adapt
    op = "adaptive_threshold_update"
    if not torch.is_tensor(thr) or thr.dim() != 1 or thr.dtype != torch.float32 or not thr.is_contiguous():
        raise ValueError(f"{op}: thr must be a contiguous float32 tensor [C]")
    Cc = int(thr.shape[0])
    if not 1 <= Cc <= ADAPT_MAX_CLASSES:
        raise ValueError(f"{op}: C={Cc} must be in 1..{ADAPT_MAX_CLASSES}")
    for name, t in (("sums", sums), ("state", state)):
        if not torch.is_tensor(t) or t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != (Cc + 2,) \
                or t.device != thr.device:
            raise ValueError(f"{op}: {name} must be a contiguous float64 tensor [C + 2 = {Cc + 2}] on {thr.device}")
    if not 0.0 <= float(momentum) < 1.0:
        raise ValueError(f"{op}: momentum={momentum} must be in [0, 1)")
    _dev(sums, state, thr)
    check(_lib_adapt.lib().asis_adapt_update(_stream(), sums.data_ptr(), state.data_ptr(), thr.data_ptr(), Cc, float(momentum)),
          "asis_adapt_update")
    return thr


# --------------------------------------------------------------------------------------------
# batch mixing (csrc/mix.hip, libasis_mix.so)
# --------------------------------------------------------------------------------------------
MIX_MAX_CLASSES = 16
MIX_TABLES = {"donor": (torch.int32, ()), "kind": (torch.int32, ()), "box": (torch.int32, (4,)), "order": (torch.uint8, (16,))}


def _host_donor(op: str, donor, B: int) -> torch.Tensor:
    """``donor`` as a host int32 tensor [B] with every entry in 0..B-1: a bad table raises here and never reaches the device"""
    if torch.is_tensor(donor):
        if donor.is_cuda or donor.dtype != torch.int32:
            raise ValueError(f"{op}: donor must be a host (CPU) int32 tensor or a sequence of ints")
        d = donor.contiguous()
    else:
        d = torch.tensor([int(v) for v in donor], dtype=torch.int32)
    if tuple(d.shape) != (B,):
        raise ValueError(f"{op}: donor has shape {list(d.shape)}, the batch has B={B} samples")
    if int(d.min()) < 0 or int(d.max()) >= B:
        raise ValueError(f"{op}: donor={d.tolist()} must lie in 0..B-1={B - 1}")
    return d


def _upload_i32(parts, dev) -> torch.Tensor:
    """host int32 tensors, concatenated, on ``dev`` through a pinned staging tensor and a non-blocking copy (the idiom of
    droppath.py): the host does not wait for the stream"""
    stage = torch.empty(sum(p.numel() for p in parts), dtype=torch.int32, pin_memory=torch.device(dev).type == "cuda")
    torch.cat([p.reshape(-1) for p in parts], out=stage)
    return stage.to(dev, non_blocking=True)


def _mix_gate_args(op: str, mix, B: int, H: int, W: int, dev):
    """(sel, donor) of ``consistency_loss(mix=)`` checked -> (sel, donor on the device)"""
    if not isinstance(mix, (tuple, list)) or len(mix) != 2:
        raise ValueError(f"{op}: mix must be (sel, donor)")
    sel, donor = mix
    if not torch.is_tensor(sel) or sel.dtype != torch.uint8 or not sel.is_contiguous() or tuple(sel.shape) != (B, H, W):
        raise ValueError(f"{op}: mix sel must be a contiguous uint8 tensor [B={B},H={H},W={W}]")
    if sel.device != dev:
        raise ValueError(f"{op}: mix sel is on {sel.device}, the logits on {dev}")
    return sel, _upload_i32([_host_donor(op, donor, B)], dev)


def mix_batch(inp: torch.Tensor, target: torch.Tensor, tables: dict, num_classes: int, background: bool = False):
    """CutMix / ClassMix over the samples of one batch (csrc/mix.hip, libasis_mix.so): sample b receives pixels of sample
    donor[b].  ``inp`` contiguous fp32 [B,3,H,W], ``target`` contiguous int64 [B,H,W], both on the device; ``tables`` the host
    (CPU) tensors of ``tools.mix.MixSampler.draw``: donor int32 [B] (0..B-1, checked here), kind int32 [B] (0 not mixed, 1 CutMix,
    2 ClassMix), box int32 [B,4] (y0, x0, y1, x1; half-open), order uint8 [B,16].  They are uploaded in one non-blocking copy from pinned memory.
    -> (inp', target', sel uint8 [B,H,W], pasted int32 [B]), fresh buffers: sel is 1 inside the box (kind 1) or where the donor's
    label is one of the classes pasted (kind 2: the first half, rounded up, of the donor's classes present in 0..num_classes-1, in
    the order order[b]; class 0 only with ``background``); inp'[b] = sel ? inp[donor[b]] : inp[b], target' likewise (copies of
    bits); pasted[b] = the pixels with sel = 1.  No host sync; bit-identical from call to call."""
    from . import _lib_mix
    op = "mix_batch"
    _dev(inp, target)
    if inp.dim() != 4 or inp.shape[1] != 3 or inp.dtype != torch.float32 or not inp.is_contiguous():
        raise ValueError(f"{op}: inp must be a contiguous float32 tensor [B,3,H,W]")
    B, _, H, W = (int(v) for v in inp.shape)
    if target.dtype != torch.int64 or not target.is_contiguous() or tuple(target.shape) != (B, H, W) or target.device != inp.device:
        raise ValueError(f"{op}: target must be a contiguous int64 tensor [B={B},H={H},W={W}] on {inp.device}")
    if not 1 <= int(num_classes) <= MIX_MAX_CLASSES:
        raise ValueError(f"{op}: num_classes={num_classes} must be in 1..{MIX_MAX_CLASSES}")
    if B * H * W >= 1 << 31:
        raise ValueError(f"{op}: B*H*W={B * H * W} must be < 2^31")
    if not isinstance(tables, dict) or set(MIX_TABLES) - set(tables):
        raise ValueError(f"{op}: tables must hold {sorted(MIX_TABLES)}")
    for name, (dtype, tail) in MIX_TABLES.items():
        t = tables[name]
        if not torch.is_tensor(t) or t.is_cuda or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != (B,) + tail:
            raise ValueError(f"{op}: tables[{name!r}] must be a contiguous host (CPU) {dtype} tensor {[B, *tail]}")
    _host_donor(op, tables["donor"], B)
    # one upload: donor | kind | box | order, every section on a 4-byte boundary
    packed = _upload_i32([tables["donor"], tables["kind"], tables["box"], tables["order"].reshape(-1).view(torch.int32)], inp.device)
    donor, kind, box, order = packed[:B], packed[B:2 * B], packed[2 * B:6 * B], packed[6 * B:]
    lib_ = _lib_mix.lib()
    sets = None
    if bool((tables["kind"] == 2).any()):  # on the host copy
        sets = torch.empty((2, B), device=inp.device, dtype=torch.int32)
        check(lib_.asis_mix_class_sets(_stream(), target.data_ptr(), donor.data_ptr(), kind.data_ptr(), order.data_ptr(), B, H, W,
                                       int(num_classes), int(bool(background)), sets.data_ptr()), "asis_mix_class_sets")
    out, tout = torch.empty_like(inp), torch.empty_like(target)
    sel = torch.empty((B, H, W), device=inp.device, dtype=torch.uint8)
    pasted = torch.empty((B,), device=inp.device, dtype=torch.int32)
    check(lib_.asis_mix_apply(_stream(), inp.data_ptr(), target.data_ptr(), donor.data_ptr(), kind.data_ptr(), box.data_ptr(),
                              None if sets is None else sets[1].data_ptr(), B, H, W, out.data_ptr(), tout.data_ptr(), sel.data_ptr(),
                              pasted.data_ptr()), "asis_mix_apply")
    return out, tout, sel, pasted


# --------------------------------------------------------------------------------------------
# backward / optimizer
# --------------------------------------------------------------------------------------------
def upsample_bn_relu_bwd(dU: torch.Tensor, x: torch.Tensor, scale, shift, mean, invstd, factor: int):
    """-> (g fp32 [B,H,W,C], partial [nblk, 2, C])."""
    _dev(dU, x)
    B, H, W, Cc = x.shape
    nblk = lib().asis_bn_bwd_nblk(B * H * W, Cc)
    g = torch.empty_like(x)
    partial = torch.empty((nblk, 2, Cc), device=x.device, dtype=torch.float32)
    check(lib().asis_upsample_bn_relu_bwd(_stream(), _f32c(dU).data_ptr(), _f32c(x).data_ptr(), scale.data_ptr(),
                                          shift.data_ptr(), mean.data_ptr(), invstd.data_ptr(), g.data_ptr(),
                                          partial.data_ptr(), B, H, W, Cc, factor), "asis_upsample_bn_relu_bwd")
    return g, partial


def maxpool_bn_relu_bwd(dy: torch.Tensor, x: torch.Tensor, scale, shift, mean, invstd):
    """dy fp32 [B,OH,OW,C] (gradient of BN+ReLU+MaxPool(3,2,1) output), x raw [B,H,W,C] -> (g, partial [nblk,2,C])."""
    _dev(dy, x)
    B, H, W, Cc = x.shape
    g = torch.empty_like(x)
    partial = torch.empty((lib().asis_bn_bwd_nblk(B * H * W, Cc), 2, Cc), device=x.device, dtype=torch.float32)
    check(lib().asis_maxpool_bn_relu_bwd(_stream(), _f32c(dy).data_ptr(), _f32c(x).data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                         mean.data_ptr(), invstd.data_ptr(), g.data_ptr(), partial.data_ptr(), B, H, W, Cc),
          "asis_maxpool_bn_relu_bwd")
    return g, partial


def dilate2(x: torch.Tensor, x_lo: Optional[torch.Tensor], Hd: int, Wd: int):
    """16-bit NHWC [B,OH,OW,C] (+lo) -> [B,Hd,Wd,C] with the input at even positions, zeros elsewhere."""
    _dev(x, x_lo)
    _not_mx("dilate2", x_lo)
    B, OH, OW, Cc = x.shape
    out = torch.empty((B, Hd, Wd, Cc), device=x.device, dtype=x.dtype)
    out_lo = torch.empty_like(out) if x_lo is not None else None
    check(lib().asis_dilate2(_stream(), _dt(x.dtype), x.data_ptr(), _p(x_lo), out.data_ptr(), _p(out_lo), B, OH, OW, Hd, Wd, Cc),
          "asis_dilate2")
    return out, out_lo


def bn_bwd_apply(g: torch.Tensor, x: torch.Tensor, mean, invstd, gamma, dgamma, dbeta, count: float,
                 dtype: torch.dtype, split: bool = False, mx: bool = False):
    """-> (dx 16-bit same shape as x, [dx_lo when split,] partial [nblk, C] column sums of dx).  ``mx`` (with ``split``): dx_lo in
    the MX form, scaled by max |dx| from one extra pass over g and x (asis_bn_bwd_absmax), tagged ``_asis_mx_amax``."""
    _dev(g, x)
    Cc = x.shape[-1]
    R = x.numel() // Cc
    nblk = lib().asis_bn_bwd_nblk(R, Cc)
    out = torch.empty(x.shape, device=x.device, dtype=dtype)
    partial = torch.empty((nblk, Cc), device=x.device, dtype=torch.float32)
    lo = _lo(out, split)
    args = (_f32c(g).data_ptr(), _f32c(x).data_ptr(), mean.data_ptr(), invstd.data_ptr(), _f32c(gamma).data_ptr(), dgamma.data_ptr(),
            dbeta.data_ptr(), float(count))
    if mx and split:
        amax = torch.empty(1, device=x.device, dtype=torch.float32)
        check(lib().asis_bn_bwd_absmax(_stream(), *args, amax.data_ptr(), R, Cc), "asis_bn_bwd_absmax")
        check(lib().asis_bn_bwd_apply_mx(_stream(), _dt(dtype), *args, out.data_ptr(), lo.data_ptr(), amax.data_ptr(), partial.data_ptr(),
                                         R, Cc), "asis_bn_bwd_apply_mx")
        return out, MxPlane.tag(lo, amax), partial
    check(lib().asis_bn_bwd_apply(_stream(), _dt(dtype), *args, out.data_ptr(), _p(lo), partial.data_ptr(), R, Cc), "asis_bn_bwd_apply")
    return (out, lo, partial) if split else (out, partial)


# ASIS_WGRAD_HALO=0: the implicit-GEMM form of asis_wgrad for the narrow 3x3 decoder stages too (A/B: profiles/r05_wgrad_halo_ab.txt)
WGRAD_HALO = int(os.environ.get("ASIS_WGRAD_HALO", "1") or 0)


def wgrad(dy: torch.Tensor, x_nhwc: torch.Tensor, Cout: int, KH: int, KW: int, stride: int, pad: int,
          inv_scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dy 16-bit [B,OH,OW,CoP]; x 16-bit [B,H,W,Cin] -> dW fp32 [Cout,Cin,KH,KW] (scaled by inv_scale)."""
    _dev(dy, x_nhwc, out)
    if not dy.is_contiguous() or not x_nhwc.is_contiguous():
        raise ValueError("wgrad: dy and x must be contiguous NHWC")
    Bn, H, W, Cin = x_nhwc.shape
    _, OH, OW, CoP = dy.shape
    P = Bn * OH * OW
    Ntot = KH * KW * Cin
    if (KH == 3 and KW == 3 and stride == 1 and pad == 1 and Cout <= 4 and Cin in (8, 16, 32, 64)
            and os.environ.get("ASIS_WGRAD_SMALLCOUT", "1") != "0"):
        # classifier convs: a handful of output channels -> direct fp32 kernel instead of an MFMA tile that is mostly padding
        nblk = 1024
        slabs = torch.empty((nblk, Cout * Ntot), device=dy.device, dtype=torch.float32)
        check(lib().asis_conv3x3_smallcout_wgrad(_stream(), _dt(dy.dtype), dy.data_ptr(), CoP, x_nhwc.data_ptr(),
                                                 slabs.data_ptr(), nblk, Bn, H, W, Cin, Cout), "asis_conv3x3_smallcout_wgrad")
        if out is None:
            out = torch.empty((Cout, Cin, KH, KW), device=dy.device, dtype=torch.float32)
        reduce_rows(slabs, inv_scale, out.view(-1))
        return out
    if WGRAD_HALO and KH == 3 and KW == 3 and stride == 1 and pad == 1 and Cout % 64 == 0 and Cin % 128 == 0 and H >= 8 and W >= 16:
        # every 3x3 / stride-1 decoder stage: halo-tile kernel, pixels as the MFMA K index through transposing LDS reads, x fetched
        # once per tile instead of once per tap (csrc/convwgrad.hip; at 12 images: 128 -> 64 at 336^2 718 -> 286 us, 256 -> 128 at
        # 168^2 494 -> 244, 512 -> 256 at 84^2 329 -> 240, 3072 -> 512 at 42^2 982 -> 781: profiles/r05_wgrad_halo_ab.txt)
        nblk = lib().asis_conv3x3_wgrad_halo_nblk(Bn, H, W, Cin, Cout)
        slabs = torch.empty((nblk, Cout * Ntot), device=dy.device, dtype=torch.float32)
        check(lib().asis_conv3x3_wgrad_halo(_stream(), _dt(dy.dtype), dy.data_ptr(), CoP, x_nhwc.data_ptr(), slabs.data_ptr(), nblk,
                                            Bn, H, W, Cin, Cout), "asis_conv3x3_wgrad_halo")
        if out is None:
            out = torch.empty((Cout, Cin, KH, KW), device=dy.device, dtype=torch.float32)
        reduce_rows(slabs, inv_scale, out.view(-1))
        return out
    splits = lib().asis_wgrad_splits(P, Cout, Ntot)
    if KH == 1 and KW == 1 and stride == 1 and pad == 0 and Cout % 256 == 0 and Cin % 128 == 0 and CoP == Cout and P >= 1024:
        # nn.Linear weight gradients on the 256 x 128 LDS-DMA form (csrc/wgrad.hip: wgrad_dense_big_kernel, two workgroups per
        # CU): one round of the 512 workgroup slots, e.g. qkv 96 tiles x 5 pixel splits (6 would spill into a second round)
        splits = max(1, min(512 // ((Cout // 256) * (Cin // 128)), P // 256))
    elif stride == 1 and Cout % 256 == 0 and Cin % 128 == 0 and CoP == Cout and P >= 1024:
        # stride-1 convolutions on the same form (wgrad_dense_big_kernel<CONV>): (Cout / 256) x (taps * Cin / 128) tiles
        splits = max(1, min(512 // ((Cout // 256) * (Ntot // 128)), P // 1024))
    slabs = torch.empty((splits, Cout * Ntot), device=dy.device, dtype=torch.float32)
    d = _lib.WgradDesc()
    d.dy, d.x, d.out = dy.data_ptr(), x_nhwc.data_ptr(), slabs.data_ptr()
    d.ld_dy, d.P, d.dtype = CoP, P, _dt(dy.dtype)
    d.Cout, d.CoP, d.Cin = Cout, CoP, Cin
    d.B_, d.H, d.W, d.OH, d.OW, d.KH, d.KW, d.stride, d.pad = Bn, H, W, OH, OW, KH, KW, stride, pad
    d.splits = splits
    check(lib().asis_wgrad(_stream(), C.byref(d)), "asis_wgrad")
    if out is None:
        out = torch.empty((Cout, Cin, KH, KW), device=dy.device, dtype=torch.float32)
    reduce_rows(slabs, inv_scale, out.view(-1))
    return out


LORA_PAD = 64   # padded width of the stacked rank dimension (q | v): 2 r <= 64 (csrc/lora.hip)


def _lora_args(op: str, x: torch.Tensor, segs, u: torch.Tensor):
    """checks shared by ``lora_down`` / ``lora_wgrad`` -> (col0a, lena, col0b, lenb, R)"""
    segs = [(int(c), int(n)) for c, n in segs]
    if len(segs) not in (1, 2):
        raise ValueError(f"{op}: one or two column segments (col0, len)")
    if x.dim() != 2 or u.dim() != 2 or x.dtype != u.dtype or x.stride(1) != 1 or u.stride(1) != 1:
        raise ValueError(f"{op}: x and u must be 2-D 16-bit matrices of one dtype with contiguous rows")
    _dt(x.dtype)
    (c0a, lena), (c0b, lenb) = segs[0], (segs[1] if len(segs) == 2 else (0, 0))
    if any(n < 64 or n % 64 for _, n in segs) or any(c < 0 or c % 8 for c, _ in segs) or (len(segs) == 2 and c0b < c0a + lena):
        raise ValueError(f"{op}: segments must have len % 64 == 0 and col0 % 8 == 0, in order and not overlapping: {segs}")
    if segs[-1][0] + segs[-1][1] > x.shape[1]:
        raise ValueError(f"{op}: segments {segs} reach past the {x.shape[1]} columns of x")
    R = x.shape[0]
    if R < 1 or u.shape[0] < R or u.shape[1] != LORA_PAD:
        raise ValueError(f"{op}: u must be a [>= {R}, {LORA_PAD}] view, got {tuple(u.shape)}")
    if x.stride(0) % 8 or u.stride(0) % 8 or x.data_ptr() % 16 or u.data_ptr() % 16:
        raise ValueError(f"{op}: x and u must be 16-byte aligned with row strides that are multiples of 8")
    return c0a, lena, c0b, lenb, R


def lora_down(x: torch.Tensor, segs, wd: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``out[R, 0:64] = round16(x_seg @ wd.T)``: x 16-bit [R, C] (any row stride), ``segs`` = [(col0, len)] or two of them (the
    columns in between are never read), wd 16-bit [64, sum(len)] contiguous.  ``out``: a 16-bit [R, 64] view (e.g. the last 64
    columns of a wider buffer); all 64 columns are written, nothing else is touched."""
    _dev(x, wd, out)
    if out is None:
        out = torch.empty((x.shape[0], LORA_PAD), device=x.device, dtype=x.dtype)
    c0a, lena, c0b, lenb, R = _lora_args("lora_down", x, segs, out)
    if wd.dtype != x.dtype or tuple(wd.shape) != (LORA_PAD, lena + lenb) or not wd.is_contiguous() or wd.data_ptr() % 16:
        raise ValueError(f"lora_down: wd must be a contiguous 16-byte aligned [{LORA_PAD}, {lena + lenb}] matrix of x's dtype")
    Kt = lena + lenb
    check(_launch_timed("lora_down", 2.0 * R * LORA_PAD * Kt,
                        lambda: lib().asis_lora_down(_stream(), _dt(x.dtype), x.data_ptr(), x.stride(0), c0a, lena, c0b, lenb,
                                                     wd.data_ptr(), out.data_ptr(), out.stride(0), R),
                        2.0 * (R * Kt + LORA_PAD * Kt + R * LORA_PAD)), "asis_lora_down")
    return out


def lora_wgrad_nblk(R: int, Nt: int) -> int:
    return lib().asis_lora_wgrad_nblk(int(R), int(Nt))


def lora_wgrad(u: torch.Tensor, x: torch.Tensor, segs, scale: float = 1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> fp32 [64, Nt] = scale * u[:R].T @ x_seg, R = rows of x: u 16-bit [>= R, 64] and x 16-bit [R, C], both row-strided,
    ``segs`` as in ``lora_down`` (Nt = sum(len)).  Per-row-block fp32 slabs summed by ``reduce_rows`` in a fixed order: two runs
    are bit-identical."""
    _dev(u, x, out)
    c0a, lena, c0b, lenb, R = _lora_args("lora_wgrad", x, segs, u)
    Nt = lena + lenb
    if out is None:
        out = torch.empty((LORA_PAD, Nt), device=x.device, dtype=torch.float32)
    elif out.dtype != torch.float32 or tuple(out.shape) != (LORA_PAD, Nt) or not out.is_contiguous():
        raise ValueError(f"lora_wgrad: out must be a contiguous float32 [{LORA_PAD}, {Nt}] tensor")
    nblk = lora_wgrad_nblk(R, Nt)
    slabs = torch.empty((nblk, LORA_PAD * Nt), device=x.device, dtype=torch.float32)
    check(_launch_timed("lora_wgrad", 2.0 * R * LORA_PAD * Nt,
                        lambda: lib().asis_lora_wgrad(_stream(), _dt(x.dtype), u.data_ptr(), u.stride(0), x.data_ptr(), x.stride(0),
                                                      c0a, lena, c0b, lenb, slabs.data_ptr(), nblk, R),
                        2.0 * R * (Nt + LORA_PAD) + 4.0 * nblk * LORA_PAD * Nt), "asis_lora_wgrad")
    reduce_rows(slabs, scale, out.view(-1))
    return out


def grad_guard(g: torch.Tensor, guard: torch.Tensor, reset: bool) -> None:
    """guard int32[2]: guard[0] |= any non-finite element of ``g`` (cleared first when ``reset``)."""
    _dev(g, guard)
    if guard.dtype != torch.int32 or guard.numel() < 2:
        raise ValueError("guard must be an int32 tensor of 2 elements")
    check(lib().asis_grad_guard(_stream(), _f32c(g).data_ptr(), g.numel(), guard.data_ptr(), int(reset)), "asis_grad_guard")


def grad_pack_bf16(g: torch.Tensor, out: torch.Tensor) -> None:
    """fp32 gradient range -> its bf16 transport form (parallel.StageReducer(compress="bf16"))"""
    _dev(g, out)
    if out.dtype != torch.bfloat16 or out.numel() != g.numel() or not out.is_contiguous():
        raise ValueError("grad_pack_bf16: out must be a contiguous bfloat16 tensor of the same length")
    check(lib().asis_grad_pack_bf16(_stream(), _f32c(g).data_ptr(), g.numel(), out.data_ptr()), "asis_grad_pack_bf16")


def grad_unpack_bf16(src: torch.Tensor, g: torch.Tensor) -> None:
    _dev(g, src)
    if src.dtype != torch.bfloat16 or src.numel() != g.numel() or not src.is_contiguous():
        raise ValueError("grad_unpack_bf16: src must be a contiguous bfloat16 tensor of the same length")
    check(lib().asis_grad_unpack_bf16(_stream(), src.data_ptr(), g.numel(), _f32c(g).data_ptr()), "asis_grad_unpack_bf16")


def zeros(shape, device, dtype=torch.float32) -> torch.Tensor:
    """zero-filled device tensor through hipMemsetAsync (asis_zero) instead of an ATen fill kernel (165 us per 173 MB in the
    config-4 step against ~30 us): the few buffers of the step that kernels ACCUMULATE into or only partly write"""
    t = torch.empty(shape, device=device, dtype=dtype)
    if t.is_cuda:
        check(lib().asis_zero(_stream(), t.data_ptr(), t.numel() * t.element_size()), "asis_zero")
    else:
        t.zero_()
    return t


def sgd_momentum(p: torch.Tensor, g: torch.Tensor, buf: torch.Tensor, lr: float, momentum: float, weight_decay: float,
                 inv_scale: float, first_step: bool, guard: Optional[torch.Tensor] = None, count_skip: bool = True) -> None:
    _dev(p, g, buf)
    if guard is not None:
        _dev(guard)
        check(lib().asis_sgd_momentum_guarded(_stream(), _f32c(p).data_ptr(), _f32c(g).data_ptr(), _f32c(buf).data_ptr(),
                                              p.numel(), float(lr), float(momentum), float(weight_decay), float(inv_scale),
                                              int(first_step), guard.data_ptr(), int(count_skip)), "asis_sgd_momentum_guarded")
        return
    check(lib().asis_sgd_momentum(_stream(), _f32c(p).data_ptr(), _f32c(g).data_ptr(), _f32c(buf).data_ptr(), p.numel(),
                                  float(lr), float(momentum), float(weight_decay), float(inv_scale), int(first_step)),
          "asis_sgd_momentum")


def grad_sumsq_blocks(n: int) -> int:
    """partials ``grad_sumsq`` writes for a bucket of ``n`` elements (host arithmetic)"""
    return int(lib().asis_grad_sumsq_blocks(int(n)))


def grad_sumsq(g: torch.Tensor, partials: torch.Tensor) -> None:
    """partials fp32 [grad_sumsq_blocks(g.numel())] = per-workgroup sums of g^2 (fixed order: bit-identical between calls);
    a non-finite element makes its partial non-finite.  ``partials``: a bucket's slice of the step's partials buffer."""
    _dev(g, partials)
    if _f32c(partials).numel() != grad_sumsq_blocks(g.numel()):
        raise ValueError(f"grad_sumsq: partials must hold {grad_sumsq_blocks(g.numel())} elements, got {partials.numel()}")
    check(lib().asis_grad_sumsq(_stream(), _f32c(g).data_ptr(), g.numel(), partials.data_ptr()), "asis_grad_sumsq")


def _adamw_state(guard: torch.Tensor, rec: torch.Tensor) -> None:
    if guard.dtype != torch.int32 or guard.numel() != 3 or not guard.is_contiguous():
        raise ValueError("guard must be a contiguous int32 tensor of 3 elements (skip flag, skipped steps, step count)")
    if _f32c(rec).numel() != 4:
        raise ValueError("rec must be a float32 tensor of 4 elements (clip coefficient, two bias corrections, norm)")


def adamw_prepare(partials: torch.Tensor, guard: torch.Tensor, rec: torch.Tensor, inv_scale: float, max_norm: Optional[float],
                  beta1: float, beta2: float) -> None:
    """Once per step, behind the ``grad_sumsq`` of every bucket: overflow decision, step count, clip coefficient (``max_norm``
    None or <= 0: no clipping) and bias corrections, all on the device (include/asis_hip.h)."""
    _dev(partials, guard, rec)
    _adamw_state(guard, rec)
    check(lib().asis_adamw_prepare(_stream(), _f32c(partials).data_ptr(), partials.numel(), guard.data_ptr(), rec.data_ptr(),
                                   float(inv_scale), float(max_norm or 0.0), float(beta1), float(beta2)), "asis_adamw_prepare")


def adamw_step(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, codes: torch.Tensor, lr_scale: torch.Tensor,
               weight_decay: torch.Tensor, lr: float, beta1: float, beta2: float, eps: float, inv_scale: float,
               guard: torch.Tensor, rec: torch.Tensor) -> None:
    """torch.optim.AdamW on one flat bucket; ``codes`` uint8 [numel / 4] picks (lr_scale, weight_decay) per 4 elements."""
    _dev(p, g, m, v, codes, lr_scale, weight_decay, guard, rec)
    _adamw_state(guard, rec)
    n = _f32c(p).numel()
    if _f32c(g).numel() != n or _f32c(m).numel() != n or _f32c(v).numel() != n:
        raise ValueError("adamw_step: p, g, m and v must have the same length")
    if codes.dtype != torch.uint8 or not codes.is_contiguous() or codes.numel() * 4 != n:
        raise ValueError(f"adamw_step: codes must be a contiguous uint8 tensor of numel / 4 = {n // 4} elements")
    if _f32c(lr_scale).numel() != _f32c(weight_decay).numel():
        raise ValueError("adamw_step: the lr_scale and weight_decay tables must have the same length")
    check(lib().asis_adamw_step(_stream(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, codes.data_ptr(),
                                lr_scale.data_ptr(), weight_decay.data_ptr(), lr_scale.numel(), float(lr), float(beta1),
                                float(beta2), float(eps), float(inv_scale), guard.data_ptr(), rec.data_ptr()), "asis_adamw_step")


# launch geometry of asis_ema_update (csrc/ema.hip): lanes per workgroup, grid cap, elements one workgroup covers per tile
EMA_BLOCK, EMA_GRID_CAP = 256, 2048
EMA_TILE = 16 * EMA_BLOCK      # four 16-byte quads per lane


def _ema_state(state: torch.Tensor, rec: torch.Tensor) -> None:
    if state.dtype != torch.int32 or state.numel() != 1:
        raise ValueError("state must be an int32 tensor of 1 element (updates applied)")
    if _f32c(rec).numel() != 2:
        raise ValueError("rec must be a float32 tensor of 2 elements (1 - decay of this update, apply flag)")


def ema_prepare(guard: Optional[torch.Tensor], state: torch.Tensor, rec: torch.Tensor, decay: float, warmup: bool) -> None:
    """Once per update, behind the optimizer's step: ``guard[0] != 0`` (the step was skipped; ``guard`` None: never) clears the
    apply flag ``rec[1]``; otherwise ``t = ++state[0]``, ``rec = (1 - optim.ema_decay_at(t, decay, warmup), 1)``, all on the
    device (include/asis_hip.h)."""
    _dev(state, rec)
    _ema_state(state, rec)
    if guard is not None:
        _dev(guard)
        if guard.dtype != torch.int32 or guard.numel() < 1 or not guard.is_contiguous():
            raise ValueError("guard must be a contiguous int32 tensor whose first element is the skip flag")
    check(lib().asis_ema_prepare(_stream(), None if guard is None else guard.data_ptr(), state.data_ptr(), rec.data_ptr(),
                                 float(decay), int(bool(warmup))), "asis_ema_prepare")


def ema_update(ema: torch.Tensor, p: torch.Tensor, rec: torch.Tensor) -> None:
    """``ema += rec[0] * (p - ema)`` (one fused multiply-add per element) when ``rec[1]`` is set, nothing otherwise."""
    _dev(ema, p, rec)
    n = _f32c(ema).numel()
    if _f32c(p).numel() != n or _f32c(rec).numel() != 2:
        raise ValueError("ema_update: ema and p must have the same length and rec 2 elements")
    check(lib().asis_ema_update(_stream(), ema.data_ptr(), p.data_ptr(), n, rec.data_ptr()), "asis_ema_update")


# --------------------------------------------------------------------------------------------
# input pipeline
# --------------------------------------------------------------------------------------------
def augment(img_u8: torch.Tensor, mask_u8: torch.Tensor, tables: dict):
    """uint8 [B,S,S,3] / uint8 [B,S,S] + the per-sample tables of ``tools.augment.TrainAugment.tables`` ->
    (fp32 [B,3,S,S] in [0,1], int64 [B,S,S])."""
    _dev(img_u8, mask_u8, *[t for t in tables.values() if torch.is_tensor(t)])
    B, S = img_u8.shape[0], img_u8.shape[1]
    if img_u8.dtype != torch.uint8 or mask_u8.dtype != torch.uint8 or img_u8.shape != (B, S, S, 3) or mask_u8.shape != (B, S, S) \
            or not img_u8.is_contiguous() or not mask_u8.is_contiguous():
        raise ValueError("augment: img uint8 [B,S,S,3] and mask uint8 [B,S,S], contiguous")
    want = {"geo": (torch.int32, (B, 4)), "xofs": (torch.int32, (B, S)), "yofs": (torch.int32, (B, S)),
            "xa": (torch.int16, (B, S, 2)), "ya": (torch.int16, (B, S, 2)), "mx": (torch.int32, (B, S)),
            "my": (torch.int32, (B, S)), "lut": (torch.uint8, (B, 256))}
    for k, (dt, shp) in want.items():
        t = tables[k]
        if t.dtype != dt or tuple(t.shape) != shp or not t.is_contiguous():
            raise ValueError(f"augment: table {k} must be contiguous {dt} {shp}")
    out = torch.empty((B, 3, S, S), device=img_u8.device, dtype=torch.float32)
    mout = torch.empty((B, S, S), device=img_u8.device, dtype=torch.int64)
    cl = tables.get("clahe")
    nonrigid = bool(tables.get("nonrigid_any", False))
    if nonrigid or (cl is not None and tables.get("clahe_any", True)):
        # CLAHE samples in the batch (train.py:161): geometric stage -> uint8, tile LUTs, blend + Lab -> RGB + tables + / 255.
        # Non-rigid samples (train.py:151-158): map + remap between the two; the per-sample flag of the CLAHE kernels leaves a
        # sample without CLAHE to the tables and / 255
        from .tools import clahe as _cl
        if cl is None:
            cl = torch.zeros((B, 2), device=img_u8.device, dtype=torch.int32)
        if cl.dtype != torch.int32 or tuple(cl.shape) != (B, 2) or not cl.is_contiguous():
            raise ValueError("augment: table clahe must be contiguous int32 (B, 2)")
        _dev(cl)
        lt = _cl.lab_tables(img_u8.device)
        geo8 = torch.empty((B, S, S, 3), device=img_u8.device, dtype=torch.uint8)
        check(lib().asis_augment_geo_u8(_stream(), img_u8.data_ptr(), mask_u8.data_ptr(), tables["geo"].data_ptr(),
                                        tables["xofs"].data_ptr(), tables["yofs"].data_ptr(), tables["xa"].data_ptr(),
                                        tables["ya"].data_ptr(), tables["mx"].data_ptr(), tables["my"].data_ptr(),
                                        geo8.data_ptr(), mout.data_ptr(), B, S), "asis_augment_geo_u8")
        if nonrigid:
            geo8, mout = nonrigid_remap(geo8, mout, nonrigid_map(tables, S))
        luts = torch.empty((B, _cl.TILES, _cl.TILES, 256), device=img_u8.device, dtype=torch.uint8)
        check(lib().asis_clahe(_stream(), geo8.data_ptr(), cl.data_ptr(), lt["gamma"].data_ptr(), lt["cbrt"].data_ptr(),
                               lt["l2yf"].data_ptr(), lt["ab2xz"].data_ptr(), lt["invgamma"].data_ptr(),
                               lt["fwd"].ctypes.data, lt["inv"].ctypes.data, luts.data_ptr(), tables["lut"].data_ptr(),
                               out.data_ptr(), B, S, _cl.TILES), "asis_clahe")
        return out, mout
    check(lib().asis_augment(_stream(), img_u8.data_ptr(), mask_u8.data_ptr(), tables["geo"].data_ptr(),
                             tables["xofs"].data_ptr(), tables["yofs"].data_ptr(), tables["xa"].data_ptr(),
                             tables["ya"].data_ptr(), tables["mx"].data_ptr(), tables["my"].data_ptr(), tables["lut"].data_ptr(),
                             out.data_ptr(), mout.data_ptr(), B, S), "asis_augment")
    return out, mout


STRONG_RMAX = 6
STRONG_TABLES = {"st_ops": (torch.int32, (4,)), "st_fac": (torch.float32, (4,)), "st_flags": (torch.int32, (2,)),
                 "st_gauss": (torch.float32, (2 * STRONG_RMAX + 1,))}


def _strong_args(op: str, x: torch.Tensor, tables: dict, apply, out):
    """The arguments of ``strong_view`` checked, without a device -> (apply on x's device or None, the host flags strong_any,
    contrast_any, the largest radius).  Values are read from the host copies (``tables["st_host"]``, as ``TrainAugment.strong_tables``
    leaves them), from the tables themselves when they live on the CPU, and only for device tables without a host copy through
    a copy to the host."""
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError(f"{op}: x must be a contiguous float32 tensor [B,3,H,W]")
    B, _, H, W = (int(v) for v in x.shape)
    if B < 1 or H < 1 or W < 1 or B * 3 * H * W >= 1 << 31 or B > 65535:
        raise ValueError(f"{op}: need B, H, W >= 1, B <= 65535 and B*3*H*W < 2^31 (shape {list(x.shape)})")
    if not isinstance(tables, dict) or set(STRONG_TABLES) - set(tables):
        raise ValueError(f"{op}: tables must hold {sorted(STRONG_TABLES)}")
    for name, (dtype, tail) in STRONG_TABLES.items():
        t = tables[name]
        if not torch.is_tensor(t) or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != (B,) + tail:
            raise ValueError(f"{op}: tables[{name!r}] must be a contiguous {dtype} tensor {[B, *tail]}")
        if t.device != x.device:
            raise ValueError(f"{op}: tables[{name!r}] is on {t.device}, x on {x.device}")
    host = tables.get("st_host") or {}
    h = lambda name: (host[name] if name in host else tables[name].cpu()).numpy()   # small host arrays: numpy is the cheap way to ask
    codes, flags = h("st_ops"), h("st_flags")
    if codes.shape != (B, 4) or flags.shape != (B, 2):
        raise ValueError(f"{op}: the host copies of the tables do not have B={B} rows")
    if int(codes.min()) < -1 or int(codes.max()) > 3:
        raise ValueError(f"{op}: operation codes must lie in -1..3 (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none)")
    has_contrast = (codes == 1).sum(1)
    if int(has_contrast.max()) > 1:
        raise ValueError(f"{op}: a sample may hold the contrast operation once")
    rad = flags[:, 1]
    if int(rad.min()) < 0 or int(rad.max()) > STRONG_RMAX or int(rad.max()) >= min(H, W):
        raise ValueError(f"{op}: blur radius must lie in 0..{STRONG_RMAX} and below min(H, W) = {min(H, W)} (reflect border)")
    on = None
    if apply is None:
        apply = tables.get("st_apply")
        if apply is not None:
            on = h("st_apply") != 0
    elif torch.is_tensor(apply):
        on = apply.cpu().numpy() != 0
        apply = apply.to(device=x.device, dtype=torch.int32)
    else:
        on = torch.tensor([bool(a) for a in apply], dtype=torch.bool)
        apply = _upload_i32([on.to(torch.int32)], x.device)
        on = on.numpy()
    if (on is not None and on.shape != (B,)) or (apply is not None and (tuple(apply.shape) != (B,) or apply.dtype != torch.int32
                                                                        or not apply.is_contiguous() or apply.device != x.device)):
        raise ValueError(f"{op}: apply must hold B={B} entries (a contiguous int32 tensor on {x.device}, or a sequence)")
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.float32 or out.shape != x.shape or not out.is_contiguous() or out.device != x.device:
            raise ValueError(f"{op}: out must be a contiguous float32 tensor {list(x.shape)} on {x.device}")
        n = x.numel() * 4
        if out.data_ptr() < x.data_ptr() + n and x.data_ptr() < out.data_ptr() + n:
            raise ValueError(f"{op}: out must not alias x (the op is out of place: the input is the teacher's view)")
    todo = (codes >= 0).any(1) | (flags != 0).any(1)
    if on is not None:
        has_contrast, todo, rad = has_contrast * on, todo & on, rad * on
    return apply, bool(todo.any()), bool(has_contrast.any()), int(rad.max())


def strong_contrast_partials(x: torch.Tensor, tables: dict, apply=None) -> torch.Tensor:
    """``asis_strong_mean`` alone -> partial float64 [B, nblk]: per sample with a contrast operation the grey sums of its chunks of
    ``asis_strong_chunk()`` pixels under the operations in front of contrast (rows of other samples are zero); their sum in index
    order over H*W is the mean ``strong_view`` uses."""
    from . import _lib_strong
    op = "strong_contrast_partials"
    apply, _, _, _ = _strong_args(op, x, tables, apply, None)
    _dev(x)
    B, _, H, W = (int(v) for v in x.shape)
    lib_ = _lib_strong.lib()
    partial = torch.zeros((B, lib_.asis_strong_nblk(H * W)), device=x.device, dtype=torch.float64)
    check(lib_.asis_strong_mean(_stream(), x.data_ptr(), tables["st_ops"].data_ptr(), tables["st_fac"].data_ptr(), _p(apply), B, H, W,
                                partial.data_ptr()), "asis_strong_mean")
    return partial


def strong_view(x: torch.Tensor, tables: dict, apply=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The strong student view (csrc/strongaug.hip, libasis_strong.so) of ``x`` contiguous fp32 [B,3,H,W] in [0,1], the output of
    ``augment``: per sample colour jitter (brightness, contrast against the sample's grey mean, saturation, hue, in the order of
    ``st_ops``, each clamped to [0,1]), greyscale, Gaussian blur with a reflect border.  ``tables``: those of
    ``tools.augment.TrainAugment.strong_tables`` (st_ops int32 [B,4], st_fac fp32 [B,4], st_flags int32 [B,2] = (grey, radius),
    st_gauss fp32 [B,13], optionally st_apply int32 [B]) on x's device.  ``apply``: per sample, 0 = copied through (default: st_apply
    of the tables, or every sample).  -> fp32 [B,3,H,W], a fresh buffer or ``out``; never in place, the input survives as the
    pre-strong (teacher's) view.  A sample without a draw or with apply 0 is copied bit by bit.  At most two launches
    (``asis_strong_mean`` only with a contrast operation), no host sync, bit-identical from call to call.  When no sample has
    anything to do the result is ``x`` itself: nothing is launched and the library is not opened."""
    op = "strong_view"
    apply, strong, contrast, rmax = _strong_args(op, x, tables, apply, out)
    if not strong:
        return x
    from . import _lib_strong
    _dev(x)
    B, _, H, W = (int(v) for v in x.shape)
    lib_ = _lib_strong.lib()
    partial = None
    if contrast:
        partial = torch.empty((B, lib_.asis_strong_nblk(H * W)), device=x.device, dtype=torch.float64)
        check(lib_.asis_strong_mean(_stream(), x.data_ptr(), tables["st_ops"].data_ptr(), tables["st_fac"].data_ptr(), _p(apply), B, H,
                                    W, partial.data_ptr()), "asis_strong_mean")
    if out is None:
        out = torch.empty_like(x)
    check(lib_.asis_strong_view(_stream(), x.data_ptr(), tables["st_ops"].data_ptr(), tables["st_fac"].data_ptr(),
                                tables["st_flags"].data_ptr(), tables["st_gauss"].data_ptr(), _p(apply), _p(partial), rmax, B, H, W,
                                out.data_ptr()), "asis_strong_view")
    return out


def nonrigid_map(tables: dict, S: int, return_field: bool = False):
    """The coordinate maps of the non-rigid block (csrc/nonrigid.hip) from the tables of
    ``tools.augment.TrainAugment.nonrigid_tables`` -> int32 [B,S,S,2] = (x, y) source coordinate in 1/32 pixel.
    ``return_field``: also the elastic displacement field fp32 [B,2,S,S] (zero for samples of another kind)."""
    kind = tables["nr_kind"]
    B = kind.shape[0]
    gauss = tables["nr_gauss"]
    want = {"nr_kind": (torch.int32, (B,)), "nr_par": (torch.float32, (B, 8)), "nr_seed": (torch.int64, (B,)),
            "nr_gx": (torch.float32, (B, S)), "nr_gy": (torch.float32, (B, S)), "nr_gauss": (torch.float32, tuple(gauss.shape))}
    for k, (dt, shp) in want.items():
        t = tables[k]
        if t.dtype != dt or tuple(t.shape) != shp or not t.is_contiguous():
            raise ValueError(f"nonrigid_map: table {k} must be contiguous {dt} {shp}")
    _dev(*[tables[k] for k in want])
    if gauss.dim() != 1 or gauss.numel() % 2 != 1:
        raise ValueError("nonrigid_map: table nr_gauss must hold 2 r + 1 weights")
    dev = kind.device
    tmp = torch.empty((B, 2, S, S), device=dev, dtype=torch.float32)
    out = torch.empty((B, S, S, 2), device=dev, dtype=torch.int32)
    field = torch.zeros((B, 2, S, S), device=dev, dtype=torch.float32) if return_field else None
    check(lib().asis_nonrigid_map(_stream(), kind.data_ptr(), tables["nr_par"].data_ptr(), tables["nr_seed"].data_ptr(),
                                  tables["nr_gx"].data_ptr(), tables["nr_gy"].data_ptr(), gauss.data_ptr(), gauss.numel() // 2,
                                  tmp.data_ptr(), out.data_ptr(), field.data_ptr() if return_field else None, B, S),
          "asis_nonrigid_map")
    return (out, field) if return_field else out


def nonrigid_remap(img_u8: torch.Tensor, mask: torch.Tensor, map_q5: torch.Tensor):
    """uint8 [B,S,S,3] + int64 [B,S,S] through a Q5 map int32 [B,S,S,2] (``nonrigid_map``): integer bilinear for the image,
    nearest for the mask, reflect-101 border -> (uint8 [B,S,S,3], int64 [B,S,S])."""
    _dev(img_u8, mask, map_q5)
    B, S = img_u8.shape[0], img_u8.shape[1]
    if img_u8.dtype != torch.uint8 or mask.dtype != torch.int64 or map_q5.dtype != torch.int32 or img_u8.shape != (B, S, S, 3) \
            or mask.shape != (B, S, S) or map_q5.shape != (B, S, S, 2) \
            or not (img_u8.is_contiguous() and mask.is_contiguous() and map_q5.is_contiguous()):
        raise ValueError("nonrigid_remap: img uint8 [B,S,S,3], mask int64 [B,S,S] and map int32 [B,S,S,2], contiguous")
    out = torch.empty_like(img_u8)
    mout = torch.empty_like(mask)
    check(lib().asis_nonrigid_remap(_stream(), img_u8.data_ptr(), mask.data_ptr(), map_q5.data_ptr(), out.data_ptr(),
                                    mout.data_ptr(), B, S), "asis_nonrigid_remap")
    return out, mout


def frame_resize(frames_u8: Optional[torch.Tensor], masks_u8: Optional[torch.Tensor], size: int, lut=None):
    """PIL-exact resize to ``size`` x ``size`` (csrc/frame_resize.hip): uint8 [B,H,W,3] frames (BILINEAR) and uint8 [B,H,W] masks
    (NEAREST, then the 256-entry label table ``lut``; None = identity) -> (uint8 [B,S,S,3], uint8 [B,S,S]).  Either input may be
    None (its output is then None).  Tables: ``tools.frame_resize``."""
    import numpy as np
    from .tools import frame_resize as _fr
    ref = frames_u8 if frames_u8 is not None else masks_u8
    if ref is None:
        raise ValueError("frame_resize: no input")
    _dev(frames_u8, masks_u8)
    B, H, W = ref.shape[0], ref.shape[1], ref.shape[2]
    if frames_u8 is not None and (frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3
                                  or not frames_u8.is_contiguous()):
        raise ValueError("frame_resize: frames must be contiguous uint8 [B,H,W,3]")
    if masks_u8 is not None and (masks_u8.dtype != torch.uint8 or tuple(masks_u8.shape) != (B, H, W) or not masks_u8.is_contiguous()):
        raise ValueError("frame_resize: masks must be contiguous uint8 [B,H,W] of the frames' size")
    S = int(size)
    if S < 1:
        raise ValueError("frame_resize: size must be positive")
    dev = ref.device
    t = _fr.device_tables(H, W, S, dev)
    out_img = out_mask = tmp = None
    if frames_u8 is not None:
        out_img = torch.empty((B, S, S, 3), device=dev, dtype=torch.uint8)
        if H != S and W != S:
            tmp = torch.empty((B, H, S, 3), device=dev, dtype=torch.uint8)
    if masks_u8 is not None:
        out_mask = torch.empty((B, S, S), device=dev, dtype=torch.uint8)
    if lut is None:
        lut = _fr.LUT_IDENTITY
    if not torch.is_tensor(lut):
        lut = torch.from_numpy(np.ascontiguousarray(np.asarray(lut, dtype=np.uint8)))
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (256,):
        raise ValueError("frame_resize: lut must be uint8 [256]")
    lut = lut.to(dev).contiguous()
    check(lib().asis_frame_resize(_stream(), _p(frames_u8), _p(masks_u8), t["xspan"].data_ptr(), t["xcoef"].data_ptr(),
                                  int(t["xcoef"].shape[1]), t["yspan"].data_ptr(), t["ycoef"].data_ptr(), int(t["ycoef"].shape[1]),
                                  t["ix"].data_ptr(), t["iy"].data_ptr(), lut.data_ptr(), _p(tmp), _p(out_img), _p(out_mask),
                                  B, H, W, S, S), "asis_frame_resize")
    return out_img, out_mask


def _u8_table(t, shape, name: str, dev, op: str = "predict_mask") -> torch.Tensor:
    import numpy as np
    if not torch.is_tensor(t):
        arr = np.asarray(t)
        if arr.dtype.kind not in "iu" or arr.size and (arr.min() < 0 or arr.max() > 255):
            raise ValueError(f"{op}: {name} must hold integers in 0..255")
        t = torch.from_numpy(np.ascontiguousarray(arr.astype(np.uint8)))
    if t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{op}: {name} must be uint8 {list(shape)}, got {t.dtype} {list(t.shape)}")
    return t.to(dev).contiguous()


def _predict_outputs(op: str, B: int, Cc: int, size, dev, encode, frames, palette, alpha, target, lut):
    """The checks and tables ``predict_mask`` and ``predict_mask_views`` share -> (H, W, enc, mask, pal, alp, overlay, lut, counts)."""
    if not 1 <= Cc <= 16:
        raise ValueError(f"{op}: logits have C={Cc} classes, supported 1..16")
    if isinstance(size, int):
        size = (size, size)
    if len(size) != 2 or int(size[0]) < 1 or int(size[1]) < 1:
        raise ValueError(f"{op}: size must be a positive int or (H, W), got {size!r}")
    H, W = int(size[0]), int(size[1])
    from .tools import frame_resize as _fr
    enc = _u8_table(_fr.ENCODE_INDEX[:Cc] if encode is None else encode, (Cc,), "encode", dev, op)
    if frames is None and (palette is not None or alpha is not None):
        raise ValueError(f"{op}: palette / alpha given without frames")
    if (target is None) != (lut is None):
        raise ValueError(f"{op}: target (raw masks) and lut (their label table) go together")
    mask = torch.empty((B, H, W), device=dev, dtype=torch.uint8)
    overlay = counts = pal = alp = None
    if frames is not None:
        if frames.dtype != torch.uint8 or tuple(frames.shape) != (B, H, W, 3) or not frames.is_contiguous():
            raise ValueError(f"{op}: frames must be contiguous uint8 [B,H,W,3] = {[B, H, W, 3]}, got {list(frames.shape)}")
        pal = _u8_table(_fr.default_palette(Cc) if palette is None else palette, (Cc, 3), "palette", dev, op)
        alp = _u8_table(_fr.default_alpha(Cc) if alpha is None else alpha, (Cc,), "alpha", dev, op)
        overlay = torch.empty((B, H, W, 3), device=dev, dtype=torch.uint8)
    if target is not None:
        if target.dtype != torch.uint8 or tuple(target.shape) != (B, H, W) or not target.is_contiguous():
            raise ValueError(f"{op}: target must be contiguous uint8 [B,H,W] = {[B, H, W]}, got {list(target.shape)}")
        lut = _u8_table(lut, (256,), "lut", dev, op)
        counts = torch.zeros((Cc, 3), device=dev, dtype=torch.int64)
    return H, W, enc, mask, pal, alp, overlay, lut, counts


def _predict_result(mask, conf, overlay, counts):
    """-> mask, or (mask[, confidence][, overlay][, counts]): what was asked for."""
    out = tuple(t for t in (mask, conf, overlay, counts) if t is not None)
    return mask if len(out) == 1 else out


def _predict_maps(op: str, noun: str, max_count: int, logits):
    """The list of logit maps of ``predict_mask_views`` / ``predict_mask_tiles`` (``noun`` = "views" / "tiles", at most ``max_count``
    of them), checked -> (K, B, C, device, ptrs, hs, ws): the last three are the ctypes arrays of the ABI."""
    import ctypes
    if torch.is_tensor(logits) or not isinstance(logits, (list, tuple)):
        raise ValueError(f"{op}: logits must be a list of 1..{max_count} NHWC tensors, got {type(logits).__name__}")
    K = len(logits)
    if not 1 <= K <= max_count:
        raise ValueError(f"{op}: logits holds {K} {noun}, supported 1..{max_count}")
    for k, v in enumerate(logits):
        if not torch.is_tensor(v) or v.dim() != 4 or v.dtype != torch.float32 or not v.is_contiguous():
            raise ValueError(f"{op}: logits[{k}] must be a contiguous float32 NHWC tensor [B,h,w,C]")
        if v.shape[0] != logits[0].shape[0] or v.shape[3] != logits[0].shape[3]:
            raise ValueError(f"{op}: logits[{k}] is {list(v.shape)}, logits[0] {list(logits[0].shape)}: every {noun[:-1]} has the same "
                             "B and C")
        if v.device != logits[0].device:
            raise ValueError(f"{op}: logits[{k}] on {v.device}, logits[0] on {logits[0].device}")
    ptrs = (ctypes.c_void_p * K)(*[v.data_ptr() for v in logits])
    hs = (ctypes.c_int * K)(*[int(v.shape[1]) for v in logits])
    ws = (ctypes.c_int * K)(*[int(v.shape[2]) for v in logits])
    return K, int(logits[0].shape[0]), int(logits[0].shape[3]), logits[0].device, ptrs, hs, ws


def predict_mask(logits: torch.Tensor, size, encode=None, *, frames: Optional[torch.Tensor] = None, palette=None, alpha=None,
                 target: Optional[torch.Tensor] = None, lut=None):
    """Native-size masks from the decoder's logits in one pass (csrc/predict.hip): fp32 NHWC [B,h,w,C] -> uint8 [B,H,W] =
    ``encode[argmax_c F.interpolate(logits, (H, W), bilinear)]``, ties to the lowest class, equal to the argmax over
    ``resize_bilinear_fwd`` bit for bit.  ``size``: (H, W) or an int; ``encode``: uint8 [C] class -> pixel value (None = the class
    index; named tables in ``tools.frame_resize.ENCODINGS``).
      ``frames`` uint8 [B,H,W,3] (+ ``palette`` uint8 [C,3], ``alpha`` uint8 [C]; defaults: green, 128 for every class but 0)
          -> also ``overlay`` uint8 [B,H,W,3] = (frame * (255 - a) + palette * a + 127) // 255 with a = alpha of the pixel's class
      ``target`` uint8 [B,H,W] raw masks + ``lut`` uint8 [256] (the dataset's label table) -> also ``counts`` int64 [C,3] =
          #(pred == c and label == c), #(pred == c), #(label == c) over the batch (labels >= C count in no class)
    -> mask, or (mask[, overlay][, counts])."""
    _dev(logits, frames, target)
    if logits.dim() != 4 or logits.dtype != torch.float32 or not logits.is_contiguous():
        raise ValueError("predict_mask: logits must be a contiguous float32 NHWC tensor [B,h,w,C]")
    B, h, w, Cc = logits.shape
    H, W, enc, mask, pal, alp, overlay, lut, counts = _predict_outputs("predict_mask", B, Cc, size, logits.device, encode, frames,
                                                                       palette, alpha, target, lut)
    check(lib().asis_predict_mask(_stream(), logits.data_ptr(), B, h, w, Cc, H, W, enc.data_ptr(), mask.data_ptr(), _p(frames),
                                  _p(pal), _p(alp), _p(overlay), _p(target), _p(lut), _p(counts)), "asis_predict_mask")
    return _predict_result(mask, None, overlay, counts)


PREDICT_MAX_VIEWS = 8


def predict_mask_views(logits, size, encode=None, *, flips=None, confidence: bool = False, frames: Optional[torch.Tensor] = None,
                       palette=None, alpha=None, target: Optional[torch.Tensor] = None, lut=None):
    """Test-time augmentation in one pass (csrc/predict.hip): ``logits`` = 1..8 views of one batch, each a contiguous fp32 NHWC map
    [B,h_k,w_k,C] of its own size; ``flips[k]`` true = view k was predicted from the mirrored frame (None = no view is).  Per native
    pixel and view, in view order: the bilinear samples of ``predict_mask`` (a mirrored view is read through mirrored columns: bit
    for bit the result of the un-mirrored map ``v.flip(2)``), a softmax over the classes in fp32, and the sum of the
    probabilities; -> uint8 [B,H,W] = ``encode[argmax_c sum]``, ties to the lowest class.  No [B,H,W,C] map is written however
    many views there are.  ``confidence=True`` -> also uint8 [B,H,W] = floor(255 * mean probability of the chosen class + 0.5).
    ``size``, ``encode``, ``frames`` / ``palette`` / ``alpha`` and ``target`` / ``lut`` as in ``predict_mask``.
    -> mask, or (mask[, confidence][, overlay][, counts])."""
    import ctypes
    op = "predict_mask_views"
    K, B, Cc, dev, ptrs, hs, ws = _predict_maps(op, "views", PREDICT_MAX_VIEWS, logits)
    flips = [False] * K if flips is None else [bool(f) for f in flips]
    if len(flips) != K:
        raise ValueError(f"{op}: flips has {len(flips)} entries for {K} views in logits")
    _dev(logits[0], frames, target)
    H, W, enc, mask, pal, alp, overlay, lut, counts = _predict_outputs(op, B, Cc, size, dev, encode, frames, palette, alpha, target,
                                                                       lut)
    conf = torch.empty((B, H, W), device=dev, dtype=torch.uint8) if confidence else None
    fl = (ctypes.c_int * K)(*[int(f) for f in flips])
    check(lib().asis_predict_mask_views(_stream(), ptrs, hs, ws, fl, K, B, Cc, H, W, enc.data_ptr(), mask.data_ptr(), _p(conf),
                                        _p(frames), _p(pal), _p(alp), _p(overlay), _p(target), _p(lut), _p(counts)),
          "asis_predict_mask_views")
    return _predict_result(mask, conf, overlay, counts)


PREDICT_MAX_TILES = 32
PREDICT_BLENDS = ("uniform", "ramp")       # the ABI's blend = the index


def predict_mask_tiles(logits, tiles, work, size, encode=None, *, blend: str = "ramp", ramp=None, confidence: bool = False,
                       frames: Optional[torch.Tensor] = None, palette=None, alpha=None, target: Optional[torch.Tensor] = None,
                       lut=None):
    """Sliding-window prediction in one pass (csrc/predict.hip): ``logits`` = 1..32 tiles of one batch, each a contiguous fp32 NHWC
    map [B,h_k,w_k,C] of its own size; ``tiles[k]`` = (oy, ox, sy, sx, flip): the integer rectangle of the working grid ``work`` =
    (Lh, Lw) (or an int) that map k holds, and whether it was predicted from the mirrored crop.  Per native pixel (y, x) of
    ``size`` = (H, W): u = (y + 0.5) * Lh / H, (x + 0.5) * Lw / W on the working grid; every tile whose rectangle holds u is
    sampled there (``align_corners=False`` sampling of its map, clamped inside the tile; mirrored columns for a mirrored tile: bit
    for bit the un-mirrored map ``v.flip(2)``), a softmax over the classes in fp32, and the probabilities are summed with the
    weight g, tiles in list order; -> uint8 [B,H,W] = ``encode[argmax_c sum]``, ties to the lowest class.  ``blend="uniform"``:
    g = 1.  ``blend="ramp"``: g = gy * gx, gy = min(distance to the tile's two row edges, ramp) / ramp, an edge on the border of
    the working grid not counting; ``ramp`` >= 1 in working pixels (None: a third of the smallest rectangle side, at least 1).
    The rectangles' row intervals must cover [0, Lh) and their column intervals [0, Lw) (enough for a full grid of windows: every
    pixel then lies in a tile).  ``confidence=True`` -> also uint8 [B,H,W] = floor(255 * weighted mean probability of the chosen
    class + 0.5).  ``size``, ``encode``, ``frames`` / ``palette`` / ``alpha`` and ``target`` / ``lut`` as in ``predict_mask``.
    -> mask, or (mask[, confidence][, overlay][, counts])."""
    import ctypes
    op = "predict_mask_tiles"
    K, B, Cc, dev, ptrs, hs, ws = _predict_maps(op, "tiles", PREDICT_MAX_TILES, logits)
    tiles = list(tiles)
    if len(tiles) != K:
        raise ValueError(f"{op}: tiles has {len(tiles)} entries for {K} maps in logits")
    if isinstance(work, int):
        work = (work, work)
    if len(work) != 2 or int(work[0]) < 1 or int(work[1]) < 1:
        raise ValueError(f"{op}: work must be a positive int or (Lh, Lw), got {work!r}")
    Lh, Lw = int(work[0]), int(work[1])
    rects, flips = [], []
    for k, t in enumerate(tiles):
        if len(t) != 5:
            raise ValueError(f"{op}: tiles[{k}] must be (oy, ox, sy, sx, flip), got {t!r}")
        oy, ox, sy, sx = (int(v) for v in t[:4])
        if sy < 1 or sx < 1 or oy < 0 or ox < 0 or oy + sy > Lh or ox + sx > Lw:
            raise ValueError(f"{op}: tiles[{k}] = {tuple(t)!r} is empty or outside the working grid work = {(Lh, Lw)}")
        rects += [oy, ox, sy, sx]
        flips.append(bool(t[4]))
    for axis, L, name in ((0, Lh, "rows"), (1, Lw, "columns")):
        reach = 0
        for o, e in sorted((rects[4 * k + axis], rects[4 * k + axis] + rects[4 * k + axis + 2]) for k in range(K)):
            if o > reach:
                break
            reach = max(reach, e)
        if reach < L:
            raise ValueError(f"{op}: tiles leave the working grid's {name} from {reach} on uncovered (work = {(Lh, Lw)})")
    if blend not in PREDICT_BLENDS:
        raise ValueError(f"{op}: blend must be one of {PREDICT_BLENDS}, got {blend!r}")
    if ramp is None:
        ramp = max(min(min(rects[4 * k + 2], rects[4 * k + 3]) for k in range(K)) // 3, 1)
    ramp = float(ramp)
    if not ramp >= 1.0:
        raise ValueError(f"{op}: ramp must be at least 1 working pixel, got {ramp!r}")
    _dev(logits[0], frames, target)
    H, W, enc, mask, pal, alp, overlay, lut, counts = _predict_outputs(op, B, Cc, size, dev, encode, frames, palette, alpha, target,
                                                                       lut)
    conf = torch.empty((B, H, W), device=dev, dtype=torch.uint8) if confidence else None
    rc = (ctypes.c_int * (4 * K))(*rects)
    fl = (ctypes.c_int * K)(*[int(f) for f in flips])
    check(lib().asis_predict_mask_tiles(_stream(), ptrs, hs, ws, rc, fl, K, Lh, Lw, PREDICT_BLENDS.index(blend), ramp, B, Cc, H, W,
                                        enc.data_ptr(), mask.data_ptr(), _p(conf), _p(frames), _p(pal), _p(alp), _p(overlay),
                                        _p(target), _p(lut), _p(counts)), "asis_predict_mask_tiles")
    return _predict_result(mask, conf, overlay, counts)


SURFACE_MAX_TOLERANCES = 8
SURFACE_WORKSPACE_BYTES = 512 << 20    # bound on the vertical-distance maps of one asis_surface_stats call (csrc/surface.hip)


def surface_thresholds(tolerances) -> list:
    """Tolerances in pixels -> the integer bounds floor(tau^2) that the squared distances are compared with."""
    import math
    tol = [float(t) for t in tolerances]
    if len(tol) > SURFACE_MAX_TOLERANCES:
        raise ValueError(f"surface_stats: {len(tol)} tolerances, at most {SURFACE_MAX_TOLERANCES} are supported")
    for t in tol:
        if not (0.0 <= t <= 32768.0):     # also refuses nan
            raise ValueError(f"surface_stats: tolerance {t!r} must be a non-negative number of pixels (at most 32768)")
    return [int(math.floor(t * t)) for t in tol]


def surface_plan(B: int, H: int, W: int, C: int, budget: Optional[int] = None, percentiles: bool = False):
    """-> (frames per call, classes per call): the largest whose vertical-distance maps (uint16, both sides) fit ``budget``
    (default ``SURFACE_WORKSPACE_BYTES``); one class of one frame is always allowed.  ``percentiles``: the int32 distances at the
    edge pixels of both sides (``dq`` of asis_surface_quantiles, per frame whatever the number of classes) count as well."""
    budget = SURFACE_WORKSPACE_BYTES if budget is None else int(budget)
    per_class = 2 * H * W * 2
    per_frame = 2 * H * W * 4 if percentiles else 0
    nc = max(1, min(C, (budget - per_frame) // per_class))
    nb = max(1, min(B, budget // (per_class * nc + per_frame))) if nc == C else 1
    return nb, nc


def surface_percentiles(percentiles) -> list:
    """Percents in 0..100, each a multiple of 0.01 (to within 1e-9) -> the integers q in 0..10000 (hundredths of a percent)
    that asis_surface_quantiles takes; at most 4."""
    from .segloss.surface import percentile_qs
    try:
        return percentile_qs(percentiles)
    except ValueError as e:
        raise ValueError(f"surface_stats: {e}") from None


def surface_stats(pred: torch.Tensor, target: torch.Tensor, num_classes: int, tolerances, *, pred_lut=None, lut=None,
                  return_d2: Optional[str] = None, percentiles=None):
    """Boundary statistics of label maps against their ground truth (csrc/surface.hip; definitions in include/asis_hip.h).
    ``pred``, ``target``: contiguous uint8 [B,H,W] raw pixel values on the device; ``pred_lut`` / ``lut``: uint8 [256] label tables
    (None = identity; a value >= C is no class); ``tolerances`` in pixels, at most 8.
    -> ints int64 [B, C, 7 + 2 T] = inter, n_pred, n_lab, e_pred, e_lab, max_pred, max_lab, hit_pred[T], hit_lab[T] and
       sums float64 [B, C, 2] = sum over E(P) of sqrt(d2_G), sum over E(G) of sqrt(d2_P) (bit-identical between calls);
       with ``return_d2`` = "pred" / "target" also the exact squared-distance field of that side's edge pixels, int32 [B,C,H,W]
       (-1 where the class has no edge pixel on that side of the frame).
    ``percentiles``: None, or at most 4 percents in 0..100, multiples of 0.01: after ``sums`` (before ``d2``) also
       ord int64 [B, C, P, 3, 2] = the order statistics (v[lo], v[hi]) of the squared distances over E(P), over E(G) and over
       the two pooled (asis_surface_quantiles: a radix select on the device; ranks and interpolation in segloss/surface.py);
       -1 for a class that is not on both sides of the frame.
    Frames and classes are processed in chunks so that the intermediate maps stay under ``SURFACE_WORKSPACE_BYTES``."""
    qs = surface_percentiles(percentiles) if percentiles is not None else None
    _dev(pred, target)
    for name, t in (("pred", pred), ("target", target)):
        if t.dtype != torch.uint8 or t.dim() != 3 or not t.is_contiguous():
            raise ValueError(f"surface_stats: {name} must be contiguous uint8 [B,H,W], got {t.dtype} {list(t.shape)}")
    if tuple(pred.shape) != tuple(target.shape):
        raise ValueError(f"surface_stats: pred {list(pred.shape)} and target {list(target.shape)} differ in shape")
    if pred.device != target.device:
        raise ValueError(f"surface_stats: pred on {pred.device}, target on {target.device}")
    Cc = int(num_classes)
    if not 1 <= Cc <= 16:
        raise ValueError(f"surface_stats: num_classes={num_classes}, supported 1..16")
    B, H, W = (int(v) for v in pred.shape)
    if B < 1 or H < 1 or W < 1 or H > 16384 or W > 16384:
        raise ValueError(f"surface_stats: shape {[B, H, W]}: sizes must be in 1..16384")
    if return_d2 not in (None, "pred", "target"):
        raise ValueError(f"surface_stats: return_d2={return_d2!r} must be None, 'pred' or 'target'")
    thr = surface_thresholds(tolerances)
    T = len(thr)
    dev = pred.device
    from .tools import frame_resize as _fr
    plut = _u8_table(_fr.LUT_IDENTITY if pred_lut is None else pred_lut, (256,), "pred_lut", dev, "surface_stats")
    glut = _u8_table(_fr.LUT_IDENTITY if lut is None else lut, (256,), "lut", dev, "surface_stats")
    ints = torch.zeros((B, Cc, 7 + 2 * T), device=dev, dtype=torch.int64)
    sums = torch.zeros((B, Cc, 2), device=dev, dtype=torch.float64)
    d2 = torch.full((B, Cc, H, W), -1, device=dev, dtype=torch.int32) if return_d2 else None
    nb, nc = surface_plan(B, H, W, Cc, percentiles=qs is not None)
    edges = torch.empty((nb, 2, H, W), device=dev, dtype=torch.uint8)
    g = torch.empty((nb, 2, nc, H, W), device=dev, dtype=torch.int16)     # uint16 on the device
    partial = torch.empty((nb, 2, nc, H), device=dev, dtype=torch.float64)
    thr_c = (C.c_int32 * max(T, 1))(*thr)
    ord_ = None
    if qs is not None:
        P = len(qs)
        q_c = (C.c_int32 * P)(*qs)
        ord_ = torch.full((B, Cc, P, 3, 2), -1, device=dev, dtype=torch.int64)
        dq = torch.empty((nb, 2, H, W), device=dev, dtype=torch.int32)
        scratch = torch.empty((surface_quantile_scratch_bytes(nb, nc, P),), device=dev, dtype=torch.uint8)
    for b0 in range(0, B, nb):
        n = min(nb, B - b0)
        for c0 in range(0, Cc, nc):
            check(lib().asis_surface_stats(_stream(), pred[b0:b0 + n].data_ptr(), target[b0:b0 + n].data_ptr(), plut.data_ptr(),
                                           glut.data_ptr(), n, H, W, Cc, c0, min(nc, Cc - c0), thr_c, T, edges.data_ptr(),
                                           g.data_ptr(), partial.data_ptr(), ints[b0:b0 + n].data_ptr(), sums[b0:b0 + n].data_ptr(),
                                           _p(d2[b0:b0 + n]) if d2 is not None else None, 1 if return_d2 == "target" else 0),
                  "asis_surface_stats")
            if qs is not None:      # edges, g and ints of the chunk are still those of the call above
                check(lib().asis_surface_quantiles(_stream(), edges.data_ptr(), g.data_ptr(), ints[b0:b0 + n].data_ptr(), n, H, W, Cc,
                                                   c0, min(nc, Cc - c0), T, q_c, P, dq.data_ptr(), scratch.data_ptr(),
                                                   ord_[b0:b0 + n].data_ptr()), "asis_surface_quantiles")
    return (ints, sums) + ((ord_,) if ord_ is not None else ()) + ((d2,) if d2 is not None else ())


def surface_quantile_scratch_bytes(B: int, nc: int, P: int) -> int:
    """Bytes of the histogram / state scratch of asis_surface_quantiles for ``B`` frames and ``nc`` classes per call."""
    n = lib().asis_surface_quantile_scratch_bytes(int(B), int(nc), int(P))
    if n < 0:
        check(int(n), "asis_surface_quantile_scratch_bytes")
    return int(n)


# ---- dropout of the MaskTransformer head (csrc/dropout.hip: counter-based masks, include/asis_hip.h) -----------------------------
def dropout_f32(x: torch.Tensor, seed: int, site: int, p: float, res: Optional[torch.Tensor] = None, alpha: float = 1.0,
                bias_n: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 contiguous [..., C]: out = (res) + (alpha * x + bias_n) * keep / (1 - p)."""
    _dev(x, res, bias_n, out)
    if x.dtype != torch.float32 or not x.is_contiguous() or (res is not None and (res.shape != x.shape or not res.is_contiguous())):
        raise ValueError("dropout_f32: contiguous float32 operands of one shape expected")
    if out is None:
        out = torch.empty_like(x)
    check(lib().asis_dropout_f32(_stream(), x.data_ptr(), _p(res), out.data_ptr(), x.numel(), int(seed), int(site), float(p),
                                 float(alpha), _p(_f32c(bias_n)), int(x.shape[-1])), "asis_dropout_f32")
    return out


def dropout_t16(x: torch.Tensor, seed: int, site: int, p: float, x_lo: Optional[torch.Tensor] = None, rescale: bool = True) -> torch.Tensor:
    """16-bit contiguous, IN PLACE: x *= keep (/ (1 - p) with ``rescale``); ``x_lo`` (split-operand residual half) zeroed alike."""
    _dev(x, x_lo)
    if not x.is_contiguous() or (x_lo is not None and (x_lo.shape != x.shape or not x_lo.is_contiguous() or x_lo.dtype != x.dtype)):
        raise ValueError("dropout_t16: contiguous 16-bit operands of one shape expected")
    check(lib().asis_dropout_t16(_stream(), _dt(x.dtype), x.data_ptr(), _p(x_lo), x.numel(), int(seed), int(site), float(p),
                                 int(bool(rescale))), "asis_dropout_t16")
    return x


def dropout_mask(n: int, seed: int, site: int, p: float, device) -> torch.Tensor:
    """uint8 [n] keep flags of dropout layer ``site`` (test infrastructure replays them in the oracle)."""
    out = torch.empty((n,), device=device, dtype=torch.uint8)
    check(lib().asis_dropout_mask(_stream(), out.data_ptr(), n, int(seed), int(site), float(p)), "asis_dropout_mask")
    return out


def softmax_dropout_fwd(S: torch.Tensor, N: int, scale: float, seed: int, site: int, p: float, dtype: torch.dtype):
    """S fp32 [rows, ld] -> (P, P * keep / (1 - p)) 16-bit [rows, ld], P = softmax(scale * S[:, :N]), padding columns 0."""
    _dev(S)
    rows, ld = S.shape
    if S.dtype != torch.float32 or not S.is_contiguous():
        raise ValueError("softmax_dropout_fwd: contiguous float32 [rows, ld] expected")
    p16 = torch.empty((rows, ld), device=S.device, dtype=dtype)
    pd16 = torch.empty_like(p16)
    check(lib().asis_softmax_dropout_fwd(_stream(), _dt(dtype), S.data_ptr(), p16.data_ptr(), pd16.data_ptr(), rows, int(N), ld,
                                         float(scale), int(seed), int(site), float(p)), "asis_softmax_dropout_fwd")
    return p16, pd16


def softmax_dropout_bwd(p16: torch.Tensor, pd16: torch.Tensor, dPd: torch.Tensor, N: int, scale: float, seed: int, site: int,
                        p: float) -> torch.Tensor:
    """-> dS 16-bit [rows, ld] = scale * P * (keep / (1 - p) * dPd - rowsum(Pd * dPd))."""
    _dev(p16, pd16, dPd)
    rows, ld = p16.shape
    if dPd.dtype != torch.float32 or dPd.shape != p16.shape or not (p16.is_contiguous() and pd16.is_contiguous() and dPd.is_contiguous()):
        raise ValueError("softmax_dropout_bwd: contiguous [rows, ld] operands expected")
    ds = torch.empty_like(p16)
    check(lib().asis_softmax_dropout_bwd(_stream(), _dt(p16.dtype), p16.data_ptr(), pd16.data_ptr(), dPd.data_ptr(), ds.data_ptr(),
                                         rows, int(N), ld, float(scale), int(seed), int(site), float(p)), "asis_softmax_dropout_bwd")
    return ds
