"""The BatchNorm-backward family of csrc/bwd.hip and the gradient-transport kernels beside it, each against a plain torch
reference on the CPU, at the widths and map sizes that reach every branch of ``bn_bwd_shape`` and of the kernels' loops.

Stage backward (``upsample_bn_relu_bwd``, ``maxpool_bn_relu_bwd``): float64 autograd through
``F.batch_norm(training=True)`` -> ``F.relu`` -> ``F.interpolate(bilinear, align_corners=True)`` / ``F.max_pool2d(3, 2, 1)``;
compared are g (the gradient at the BatchNorm output, element by element), dbeta = sum g and dgamma = sum g xhat.  The kernel
receives the float64 statistics rounded to fp32 and the very x and dU the reference sees.  Two input rules keep every element
comparable (``_condition``; asserted on the CPU in test_input_rules): every pre-activation |x scale + shift| >= 1e-3, so fp32
and float64 agree on the ReLU mask, and every pooling window's positive maximum is unique by 1e-3, so they agree on the winner.
Exact ties are a case of their own (integer maps: bit-equal to ATen's first-maximum rule).

``bn_bwd_apply``: float64 ``gamma invstd (g - dbeta / n - xhat dgamma / n)`` on arbitrary dgamma / dbeta / count.

Bounds, none of them taken from what the kernels give:
  fp32 outputs   err <= max(4 Y, U ulp32 max|ref|): Y = the error of the SAME operation evaluated by torch in float32 on the
                 CPU against float64 (the kernels sum in another order, a small multiple is expected; a dropped tap, row or
                 tile is orders of magnitude above).  U = 4 for element-wise outputs.  U = 16 for sums over rows: a thread
                 row (ry == 0) adds the RW <= 256 per-row values of its block one after the other in fp32 before the double
                 reduction; with rounding errors uniform in +-ulp/2 that chain alone has an rms error of sqrt(RW) / 4.9 ulps
                 of |sum| = 3.3 ulps at RW = 256 on zero-mean summands, and 16 is its 4 to 5 sigma.  One dropped row of n
                 moves a sum by 1 / sqrt(n) .. 1 / n of its value: >= 150 ulps at the largest n used here.
  16-bit outputs |out - ref| <= h |ref| + (fp32 bound), h = 2^-11 (fp16) / 2^-8 (bf16) = half an ulp of the type;
                 hi + lo: 2^-21 / 2^-15 in the place of h.  fp16 only: + 2^-25, half a SUBNORMAL fp16 ulp, which is what the
                 stored residual (and a dx below 2^-14) is rounded to whatever its size.
  MX planes      rel-L2 0.04 against the 16-bit planes, as tests/test_gpu_mx.py (e4m3: 3 mantissa bits).
  absmax         against max |dx| of the float32 torch evaluation: the kernel's expression is the same fp32 expression with
                 the compiler free to contract a product and a sum into one FMA (three candidates, each moves the result by
                 at most half an ulp of a term that is itself O(result) on these inputs): <= 8 ulps of the maximum.
  bit-exact      dilate2, the bf16 pack / unpack, hi planes across the three output forms, determinism, tie routing, the
                 skipped SGD step, copies, single fp32 adds and multiplies, the 16-bit image of cast_colsum: ``torch.equal``.

Measured on one MI355X, the case with the largest err / bound per output (all cases: run with ``-s``, every check prints a
MEASURE line before it asserts):

    output                      worst case               err        Y (float32)  bound      err / bound
    upsample  g                 2x5x4    C 268  x4       6.78e-06   6.54e-06     2.62e-05   0.26
    upsample  dbeta             3x11x1   C 16   x2       4.22e-06   2.76e-06     5.54e-05   0.08
    upsample  dgamma            1x6x6    C 256  x4       2.53e-05   1.78e-05     1.80e-04   0.14
    maxpool   g                 1x12x10  C 256           4.77e-07   4.77e-07     2.78e-06   0.17
    maxpool   dbeta             1x5x6    C 20            4.77e-07   2.38e-07     1.21e-05   0.04
    maxpool   dgamma            2x1x7    C 16            7.01e-07   3.12e-07     1.27e-05   0.06
    apply     dx16   f16/bf16   17641 x 256 / 2731 x 1536   (element error / element limit)   0.997 / 0.996
    apply     hi+lo  f16/bf16   2731 x 1536                 (element error / element limit)   0.19  / 0.24
    apply     column sums       1000 x 4                 5.77e-05   5.77e-05     1.04e-03   0.06
    chain     hi+lo  f16        2x13x8   C 96   x2          (element error / element limit)   0.12
    cast_colsum sums            33 x 1028                2.52e-06   3.84e-06     5.35e-05   0.05

rel-L2(hi) / rel-L2(hi + lo) >= 3248 (fp16), 664 (bf16); asis_bn_bwd_absmax EQUAL to the float32 torch maximum in all 28 cases
(0 ulps); decoded MX planes at most 2.67e-2 (hi8) and 2.61e-2 (lo8) rel-L2 from the 16-bit planes.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from adaptersis_amd import _lib, ops
from tests.bound_helpers import DT, HALF, PAIR, SUBN, ULP32, U_ELEM, U_SUM, _bound, _err, _gen
from tests.conftest import rel_l2
from tests.mx_helpers import decode, e4m3, mx_bytes

gpu = pytest.mark.gpu
EPS = 1e-5

# C -> (CW, RW, channel tiles) of bn_bwd_shape, and the branch each width is here for
SHAPES = {4: (1, 256, 1),       # one chunk: a block is 256 rows of one float4
          16: (4, 64, 1),       # power of two, full block
          20: (5, 51, 1),       # C/4 odd: 255 threads
          64: (16, 16, 1),
          96: (24, 10, 1),      # 240 threads: a partial last wave
          256: (64, 4, 1),      # widest single tile
          268: (64, 4, 2),      # C/4 = 67 prime: the "awkward width" branch, second tile 3 chunks wide
          1536: (64, 4, 6)}     # six tiles


def _nblk_expected(rows: int, C: int) -> int:
    CW, RW, tiles = SHAPES[C]
    return max(1, min(-(-rows // RW), max(4096 // tiles, 64)))


def _check_grid(rows: int, C: int, partial: torch.Tensor, capped: bool) -> None:
    """the case has the block count its comment claims: a later change of the shape rule cannot silently uncover a branch"""
    want = _nblk_expected(rows, C)
    assert _lib.lib().asis_bn_bwd_nblk(rows, C) == want == partial.shape[0], (rows, C, want, partial.shape)
    CW, RW, tiles = SHAPES[C]
    assert capped == (want * RW < rows), (rows, C, want, "grid-stride path expected" if capped else "one row per thread expected")


def _stats(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor):
    """float64 batch statistics of NHWC x and the folded affine, as the forward hands them to the backward kernels"""
    x64 = x.double()
    mean = x64.mean((0, 1, 2))
    invstd = (x64.var((0, 1, 2), unbiased=False) + EPS).rsqrt()
    scale = gamma.double() * invstd
    shift = beta.double() - mean * scale
    return scale, shift, mean, invstd


def _window_margin(act: torch.Tensor):
    """act NHWC post-ReLU (float64) -> (top1, top1 - top2, index of top1) per 3x3 / stride 2 / pad 1 window, [B, C, L]"""
    B, H, W, C = act.shape
    cols = F.unfold(F.pad(act.permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(B, C, 9, -1)
    top, idx = cols.topk(2, dim=2)
    return top[:, :, 0], top[:, :, 0] - top[:, :, 1], idx[:, :, 0]


def _condition(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, pool: bool) -> torch.Tensor:
    """nudge the raw fp32 input until |pre-activation| >= 2e-3 everywhere and (``pool``) every window with a positive maximum
    has it unique by 2e-3; no element is excluded.  The statistics move with the nudges, hence the loop."""
    B, H, W, C = x.shape
    for _ in range(40):
        scale, shift, _, _ = _stats(x, gamma, beta)
        pre = x.double() * scale + shift
        delta = torch.where(pre.abs() < 2e-3, torch.where(pre < 0, -4e-3, 4e-3), 0.0).double()
        if pool:
            top, margin, idx = _window_margin(F.relu(pre))
            viol = (top > 0) & (margin < 2e-3)
            hot = torch.zeros(B, C, 9, top.shape[-1], dtype=torch.float64)
            hot.scatter_(2, idx.unsqueeze(2), viol.double().unsqueeze(2))
            hit = F.fold(hot.view(B, C * 9, -1), (H + 2, W + 2), 3, stride=2)[:, :, 1:-1, 1:-1].permute(0, 2, 3, 1)
            delta = delta + torch.where(hit > 0, 4e-3, 0.0)
        if not bool((delta != 0).any()):
            return x
        x = (x.double() + delta / scale).float()
    raise AssertionError("input conditioning did not converge")


UP_CASES = [  # (B, H, W, C, factor, capped)
    (2, 9, 9, 16, 2, False), (2, 9, 9, 16, 4, False),        # the shape test_gpu_kernels2 has
    (2, 7, 5, 4, 4, False),          # fewer rows than RW: one block, idle thread rows; runs 9 wide: second batch trip
    (1, 1, 13, 16, 4, False),        # 1 x W: rh = 0
    (3, 11, 1, 16, 2, False),        # H x 1: rw = 0
    (3, 1, 1, 16, 2, False),         # both
    (2, 8, 8, 16, 1, False), (2, 9, 7, 96, 1, False),         # factor 1 (UNet DoubleConv): identity taps
    (2, 6, 10, 20, 4, False),        # 255-thread block, 3 blocks, the last partial
    (2, 13, 8, 96, 2, False),        # 240-thread block
    (1, 6, 6, 256, 4, False),
    (2, 5, 4, 268, 4, False),        # partial second channel tile
    (1, 3, 2, 1536, 2, False),       # six tiles, 2 blocks
    (2, 42, 84, 16, 2, False), (1, 84, 84, 64, 2, False), (1, 168, 168, 16, 2, False),   # decoder stage sizes, non-square
    (2, 84, 56, 268, 2, True),       # 9408 rows > 2048 blocks x 4: grid-stride, partial tile
    (1, 42, 84, 1536, 1, True),      # 3528 rows > 682 x 4
]
POOL_CASES = [  # (B, H, W, C, capped)
    (2, 2, 2, 16, False), (2, 3, 3, 4, False), (2, 1, 7, 16, False), (2, 6, 1, 16, False), (1, 5, 6, 20, False),
    (2, 8, 7, 64, False), (2, 9, 9, 96, False), (1, 12, 10, 256, False), (1, 4, 5, 268, False), (1, 3, 4, 1536, False),
    (2, 112, 112, 64, False),        # the stem's own map
    (1, 96, 90, 268, True),          # 8640 rows > 2048 x 4
]


@functools.lru_cache(maxsize=None)
def _stage_inputs(kind: str, B: int, H: int, W: int, C: int, factor: int):
    gen = _gen(1 if kind == "up" else 2, B, H, W, C, factor)
    x = torch.randn(B, H, W, C, generator=gen) * 1.5 + 0.3
    gamma = (0.5 + torch.rand(C, generator=gen)) * torch.where(torch.rand(C, generator=gen) < 0.25, -1.0, 1.0)
    beta = torch.randn(C, generator=gen) * 0.3
    x = _condition(x, gamma, beta, kind == "pool")
    if kind == "up":
        OH, OW = H * factor, W * factor
    else:
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dU = torch.randn(B, OH, OW, C, generator=gen) + 0.25
    return x, gamma, beta, dU


def _stage_ref(kind, x, gamma, beta, dU, factor, dtype):
    """autograd in ``dtype``: (g at the BatchNorm output NHWC, dbeta, dgamma)"""
    B, H, W, C = x.shape
    xn = x.to(dtype).permute(0, 3, 1, 2)
    ga, be = gamma.to(dtype).requires_grad_(), beta.to(dtype).requires_grad_()
    y = F.batch_norm(xn, None, None, ga, be, True, 0.1, EPS)
    y.retain_grad()
    a = F.relu(y)
    out = F.interpolate(a, size=(H * factor, W * factor), mode="bilinear", align_corners=True) if kind == "up" \
        else F.max_pool2d(a, 3, 2, 1)
    out.backward(dU.to(dtype).permute(0, 3, 1, 2))
    return y.grad.permute(0, 2, 3, 1), be.grad, ga.grad


def _report(name, case, err, bound, yard):
    print(f"MEASURE {name} {case}: err {err:.3e} yard {yard:.3e} bound {bound:.3e} ratio {err / bound:.3f}")


def _check_stage(dev, kind, case, x, gamma, beta, dU, factor, capped):
    B, H, W, C = x.shape
    scale, shift, mean, invstd = _stats(x, gamma, beta)
    # the input rules, in the precision of the kernel and of the reference
    pre32 = x * scale.float() + shift.float()
    assert float(pre32.abs().min()) >= 1e-3 and float((x.double() * scale + shift).abs().min()) >= 1e-3
    assert bool(((pre32 > 0) == (x.double() * scale + shift > 0)).all())
    g64, db64, dg64 = _stage_ref(kind, x, gamma, beta, dU, factor, torch.float64)
    g32, db32, dg32 = _stage_ref(kind, x, gamma, beta, dU, factor, torch.float32)
    dv = [t.float().to(dev) for t in (scale, shift, mean, invstd)]
    xd, dUd = x.to(dev), dU.to(dev)
    run = (lambda: ops.upsample_bn_relu_bwd(dUd, xd, *dv, factor)) if kind == "up" else (lambda: ops.maxpool_bn_relu_bwd(dUd, xd, *dv))
    g, partial = run()
    _check_grid(B * H * W, C, partial, capped)
    g2, partial2 = run()
    assert torch.equal(g, g2) and torch.equal(partial, partial2)
    red = ops.reduce_rows(partial.view(partial.shape[0], -1)).view(2, C)
    for name, got, ref, f32, ulps in (("g", g, g64, g32, U_ELEM), ("dbeta", red[0], db64, db32, U_SUM), ("dgamma", red[1], dg64, dg32, U_SUM)):
        bound, yard = _bound(f32, ref, ulps)
        err = _err(got, ref)
        _report(f"{kind}.{name}", case, err, bound, yard)
        assert err <= bound, (name, case, err, bound, yard)


def test_input_rules():
    """CPU: the conditioned inputs keep every |pre-activation| >= 1e-3 and every positive window maximum unique by 1e-3,
    in float64 and in the kernel's fp32 arithmetic; nothing is masked out"""
    for kind, cases in (("up", [c[:5] for c in UP_CASES if c[0] * c[1] * c[2] * c[3] < 200000]),
                        ("pool", [c[:4] + (0,) for c in POOL_CASES if c[0] * c[1] * c[2] * c[3] < 200000])):
        for B, H, W, C, f in cases:
            x, gamma, beta, dU = _stage_inputs(kind, B, H, W, C, f)
            scale, shift, _, _ = _stats(x, gamma, beta)
            pre = x.double() * scale + shift
            pre32 = x * scale.float() + shift.float()
            assert float(pre.abs().min()) >= 1e-3 and float(pre32.abs().min()) >= 1e-3, (kind, B, H, W, C)
            assert 0.05 < float((pre > 0).double().mean()) < 0.95        # both sides of the ReLU are populated
            if kind == "pool":
                for p in (pre, pre32.double()):
                    top, margin, _ = _window_margin(F.relu(p))
                    assert bool(((top <= 0) | (margin >= 1e-3)).all()), (B, H, W, C)


@gpu
@pytest.mark.parametrize("B,H,W,C,factor,capped", UP_CASES)
def test_upsample_bn_relu_bwd(dev, B, H, W, C, factor, capped):
    x, gamma, beta, dU = _stage_inputs("up", B, H, W, C, factor)
    _check_stage(dev, "up", (B, H, W, C, factor), x, gamma, beta, dU, factor, capped)


@gpu
@pytest.mark.parametrize("B,H,W,C,capped", POOL_CASES)
def test_maxpool_bn_relu_bwd(dev, B, H, W, C, capped):
    x, gamma, beta, dU = _stage_inputs("pool", B, H, W, C, 0)
    scale, shift, _, _ = _stats(x, gamma, beta)
    for p in (x.double() * scale + shift, (x * scale.float() + shift.float()).double()):
        top, margin, _ = _window_margin(F.relu(p))
        assert bool(((top <= 0) | (margin >= 1e-3)).all())     # every positive maximum unique by a margin
    _check_stage(dev, "pool", (B, H, W, C), x, gamma, beta, dU, 0, capped)


@gpu
@pytest.mark.parametrize("H,W", [(5, 5), (2, 2), (3, 3), (6, 7), (9, 4), (1, 6)])
def test_maxpool_bwd_ties_follow_first_maximum(dev, H, W):
    """integer maps, scale 1, shift 0: ties are exact in every precision, so g and both sums must EQUAL ATen's CPU
    max_pool2d backward (gradient to the first maximum in scan order), and a window whose maximum is 0 after ReLU gives none"""
    B, C = 2, 8
    gen = _gen(3, H, W)
    x = torch.randint(-2, 3, (B, H, W, C), generator=gen).float()
    x[..., 0] = 1.0                      # constant map: every window ties on all of its elements
    x[..., 1] = 0.0                      # maximum 0 after ReLU everywhere
    x[..., 2] = -torch.rand(B, H, W, generator=gen).round() - 1.0   # all negative
    x[..., 3] = torch.randint(0, 2, (B, H, W), generator=gen).float()   # zeros and ones
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy = torch.randint(1, 8, (B, OH, OW, C), generator=gen).float()
    xr = x.double().permute(0, 3, 1, 2).requires_grad_()
    F.max_pool2d(F.relu(xr), 3, 2, 1).backward(dy.double().permute(0, 3, 1, 2))
    g_ref = xr.grad.permute(0, 2, 3, 1)
    if (H, W) == (5, 5):                 # the rule itself: the all-ones map routes each window to its top-left in-bounds element
        want = torch.zeros(B, H, W)
        for oh in range(OH):
            for ow in range(OW):
                want[:, max(2 * oh - 1, 0), max(2 * ow - 1, 0)] += dy[:, oh, ow, 0]
        assert torch.equal(g_ref[..., 0].float(), want)
    assert float(g_ref[..., 1].abs().max()) == 0 and float(g_ref[..., 2].abs().max()) == 0
    one, zero = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    g, partial = ops.maxpool_bn_relu_bwd(dy.to(dev), x.to(dev), one, zero, zero, one)
    assert torch.equal(g.cpu().double(), g_ref)
    red = ops.reduce_rows(partial.view(partial.shape[0], -1)).view(2, C).cpu().double()
    assert torch.equal(red[0], g_ref.sum((0, 1, 2))) and torch.equal(red[1], (g_ref * x.double()).sum((0, 1, 2)))


# ---------------------------------------------------------------------------------------------------------------------------
APPLY_CASES = [  # (R, C, count, capped)
    (100, 4, 100, False), (1000, 4, 2000, False), (162, 16, 162, False), (262181, 16, 262181, True), (120, 20, 120, False),
    (333, 64, 999, False), (208, 96, 208, False), (7, 96, 7, False), (36, 256, 36, False), (17641, 256, 35282, True),
    (41, 268, 41, False), (8200, 268, 8200, True), (6, 1536, 6, False), (2731, 1536, 5462, True)]


@functools.lru_cache(maxsize=None)
def _apply_inputs(R: int, C: int, count: int, zero_g: bool = False):
    gen = _gen(4, R, C, count)
    x = torch.randn(R, C, generator=gen) * 1.5 + 0.2
    g = torch.zeros(R, C) if zero_g else torch.randn(R, C, generator=gen) + 0.3
    gamma = (0.5 + torch.rand(C, generator=gen)) * torch.where(torch.rand(C, generator=gen) < 0.25, -1.0, 1.0)
    x64 = x.double()
    mean = x64.mean(0).float()
    invstd = (x64.var(0, unbiased=False) + EPS).rsqrt().float() if R > 1 else torch.ones(C)
    k = 0.0 if zero_g else 0.3 * count
    dgamma, dbeta = torch.randn(C, generator=gen) * k, torch.randn(C, generator=gen) * k
    return g, x, mean, invstd, gamma, dgamma, dbeta


def _apply_ref(g, x, mean, invstd, gamma, dgamma, dbeta, count, dtype):
    g, x, mean, invstd, gamma, dgamma, dbeta = (t.to(dtype) for t in (g, x, mean, invstd, gamma, dgamma, dbeta))
    inv_n = torch.tensor(1.0 / count, dtype=torch.float64).to(dtype)      # the kernel's (float)(1.0 / count)
    return gamma * invstd * (g - dbeta * inv_n - (x - mean) * invstd * dgamma * inv_n)


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("R,C,count,capped", APPLY_CASES)
def test_bn_bwd_apply_forms(dev, dt, R, C, count, capped):
    """plain, split and MX output of one dx: 16-bit image, hi + lo, column sums of the unrounded dx, absmax, MX bytes"""
    inp = _apply_inputs(R, C, count)
    ref = _apply_ref(*inp, count, torch.float64)
    f32 = _apply_ref(*inp, count, torch.float32)
    b32, yard = _bound(f32, ref, U_ELEM)
    d = [t.to(dev) for t in inp]
    tag = f"{'f16' if dt == torch.float16 else 'bf16'}"
    dx, partial = ops.bn_bwd_apply(*d, count, dt)
    _check_grid(R, C, partial, capped)
    hi, lo, partial_s = ops.bn_bwd_apply(*d, count, dt, split=True)
    hi_m, mx, partial_m = ops.bn_bwd_apply(*d, count, dt, split=True, mx=True)
    assert torch.equal(dx, hi) and torch.equal(dx, hi_m)
    assert torch.equal(partial, partial_s) and torch.equal(partial, partial_m)
    # 16-bit image: half an ulp of the type on top of the fp32 bound, element by element
    e16 = (dx.double().cpu() - ref).abs()
    lim = HALF[dt] * ref.abs() + SUBN[dt] + b32
    _report(f"apply.dx16.{tag}", (R, C), float((e16 / lim).max()), 1.0, yard)
    assert bool((e16 <= lim).all()), float((e16 / lim).max())
    pair = hi.double().cpu() + lo.double().cpu()
    ep = (pair - ref).abs()
    limp = PAIR[dt] * ref.abs() + SUBN[dt] + b32
    _report(f"apply.hi+lo.{tag}", (R, C), float((ep / limp).max()), 1.0, yard)
    assert bool((ep <= limp).all()), float((ep / limp).max())
    r_hi, r_pair = rel_l2(dx, ref), rel_l2(pair, ref)
    print(f"MEASURE apply.gain.{tag} {(R, C)}: hi {r_hi:.3e} hi+lo {r_pair:.3e} gain {r_hi / r_pair:.0f}")
    assert r_pair * 64 < r_hi          # 2^-11 / 2^-21 (2^-8 / 2^-15) in the formats: 128 at the least, 64 asked
    # column sums of the UNROUNDED dx
    cs = ops.reduce_rows(partial)
    bsum, ysum = _bound(f32.double().sum(0).float(), ref.sum(0), U_SUM)
    err = _err(cs, ref.sum(0))
    _report(f"apply.colsum.{tag}", (R, C), err, bsum, ysum)
    assert err <= bsum, (err, bsum, ysum)
    # MX: the scale is max |dx| of the fp32 expression (contraction apart), hi unchanged, bytes decode to hi and lo
    amax = float(mx._asis_mx_amax)
    want = float(f32.abs().max())
    print(f"MEASURE apply.amax.{tag} {(R, C)}: kernel {amax!r} f32 {want!r} ulps {abs(amax - want) / (ULP32 * want):.2f}")
    assert abs(amax - want) <= 8 * ULP32 * want
    assert not any(bool(((b & 0x7F) == 0x7F).any()) for b in mx_bytes(mx.cpu(), False))      # e4m3 has no inf: 0x7f / 0xff are NaN
    dh, dl = decode(mx.cpu(), amax, dt, False)
    assert bool(torch.isfinite(dh).all() and torch.isfinite(dl).all())
    e_h, e_l = rel_l2(dh, hi.float()), rel_l2(dl, lo.float())
    print(f"MEASURE apply.mx.{tag} {(R, C)}: hi8 {e_h:.3e} lo8 {e_l:.3e}")
    assert e_h < 0.04 and e_l < 0.04


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("R,C", [(208, 96), (50, 16)])
def test_bn_bwd_apply_mx_zero_gradient(dev, dt, R, C):
    """all-zero g (and sums): dx = 0, the absolute maximum stays 0; the planes must be finite and decode to zero"""
    inp = _apply_inputs(R, C, R, True)
    d = [t.to(dev) for t in inp]
    hi, mx, partial = ops.bn_bwd_apply(*d, R, dt, split=True, mx=True)
    assert float(mx._asis_mx_amax) == 0.0
    assert float(hi.float().abs().max()) == 0.0 and float(partial.abs().max()) == 0.0
    b_hi, b_lo = mx_bytes(mx.cpu(), False)
    for b in (b_hi, b_lo):
        v = e4m3(b)
        assert not bool(((b & 0x7F) == 0x7F).any())                              # the NaN bytes
        assert bool(torch.isfinite(v).all()) and float(v.abs().max()) == 0.0     # zero at any scale


@gpu
def test_bn_bwd_chain_matches_autograd_dx(dev):
    """stage kernel -> reduce_rows -> bn_bwd_apply, with the true sums and count: the gradient at the BatchNorm INPUT of float64
    autograd, at the 240-thread width (the apply formula above is the textbook one only with consistent sums)"""
    B, H, W, C, f = 2, 13, 8, 96, 2
    x, gamma, beta, dU = _stage_inputs("up", B, H, W, C, f)
    xr = x.double().permute(0, 3, 1, 2).requires_grad_()
    y = F.interpolate(F.relu(F.batch_norm(xr, None, None, gamma.double(), beta.double(), True, 0.1, EPS)), size=(H * f, W * f),
                      mode="bilinear", align_corners=True)
    y.backward(dU.double().permute(0, 3, 1, 2))
    ref = xr.grad.permute(0, 2, 3, 1)
    scale, shift, mean, invstd = (t.float().to(dev) for t in _stats(x, gamma, beta))
    g, partial = ops.upsample_bn_relu_bwd(dU.to(dev), x.to(dev), scale, shift, mean, invstd, f)
    red = ops.reduce_rows(partial.view(partial.shape[0], -1)).view(2, C)
    hi, lo, _ = ops.bn_bwd_apply(g, x.to(dev), mean, invstd, gamma.to(dev), red[1].contiguous(), red[0].contiguous(), B * H * W,
                                 torch.float16, split=True)
    # fp32 throughout plus the pair's 2^-21: the float32 autograd error is the yardstick
    x32 = x.permute(0, 3, 1, 2).clone().requires_grad_()
    F.interpolate(F.relu(F.batch_norm(x32, None, None, gamma, beta, True, 0.1, EPS)), size=(H * f, W * f), mode="bilinear",
                  align_corners=True).backward(dU.permute(0, 3, 1, 2))
    b32, yard = _bound(x32.grad.permute(0, 2, 3, 1), ref, U_ELEM)
    ep = (hi.double().cpu() + lo.double().cpu() - ref).abs()
    lim = PAIR[torch.float16] * ref.abs() + SUBN[torch.float16] + b32
    _report("chain.hi+lo.f16", (B, H, W, C, f), float((ep / lim).max()), 1.0, yard)
    assert bool((ep <= lim).all()), float((ep / lim).max())


# ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("with_lo", [False, True])
def test_dilate2(dev, dt, C, extra, with_lo):
    B, OH, OW = 2, 5, 7
    Hd, Wd = 2 * OH - 1 + extra, 2 * OW - 1 + extra
    gen = _gen(5, C, extra)
    x = torch.randn(B, OH, OW, C, generator=gen).to(dt)
    lo = (torch.randn(B, OH, OW, C, generator=gen) * 1e-3).to(dt) if with_lo else None
    out, out_lo = ops.dilate2(x.to(dev), None if lo is None else lo.to(dev), Hd, Wd)
    for got, src in ((out, x), (out_lo, lo)):
        if src is None:
            assert got is None
            continue
        want = torch.zeros(B, Hd, Wd, C, dtype=dt)
        want[:, 0:2 * OH:2, 0:2 * OW:2] = src
        assert torch.equal(got.cpu().view(torch.int16), want.view(torch.int16))


def _bits(v):
    return torch.tensor([x - (1 << 32) if x >= (1 << 31) else x for x in v], dtype=torch.int32).view(torch.float32)


def _pack_values(n: int) -> torch.Tensor:
    special = _bits([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000, 0x3F80FFFF, 0x3F800001,   # ties at the bf16
                     0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00008000, 0x00018000, 0x007F8000, 0x00400000,   # half-ulp, +-0, subnormals
                     0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7F7F8000, 0x7F7F7FFF, 0xFF7FFFFF])  # inf, NaN, the top of the range
    named = torch.tensor([1e-38, -1e-38, 3e38, -3e38, 1.0, -1.0, 65504.0, 1e-7], dtype=torch.float32)
    gen = _gen(6, n)
    rnd = torch.randint(-(1 << 31), (1 << 31) - 1, (n,), generator=gen, dtype=torch.int64).to(torch.int32).view(torch.float32)
    head = torch.cat([special, named])
    k = min(n, head.numel())
    rnd[:k] = head[:k]
    return rnd


def _same_bf16(got: torch.Tensor, want: torch.Tensor) -> bool:
    nan = want.float().isnan()
    return bool((got.float().isnan() == nan).all()) and torch.equal(got.view(torch.int16)[~nan], want.view(torch.int16)[~nan])


@gpu
@pytest.mark.parametrize("n", [4, 1028, (1 << 20) + 8])
def test_grad_pack_unpack_bf16(dev, n):
    """round to nearest even bit for bit (NaN stays NaN), and the way back is exact"""
    v = _pack_values(n)
    want = v.to(torch.bfloat16)
    out = torch.empty(n, device=dev, dtype=torch.bfloat16)
    ops.grad_pack_bf16(v.to(dev), out)
    assert _same_bf16(out.cpu(), want)
    back = torch.full((n,), 7.0, device=dev)
    ops.grad_unpack_bf16(want.to(dev), back)
    wf = want.float()
    nan = wf.isnan()
    assert bool((back.cpu().isnan() == nan).all()) and torch.equal(back.cpu().view(torch.int32)[~nan], wf.view(torch.int32)[~nan])


@gpu
def test_grad_pack_bf16_slice_and_refusals(dev):
    n, off = 1028, 16
    v = _pack_values(n)
    buf = torch.full((n + 64,), 5.0, device=dev)
    buf[off:off + n] = v.to(dev)
    out = torch.full((n + 64,), 3.0, device=dev, dtype=torch.bfloat16)
    ops.grad_pack_bf16(buf[off:off + n], out[8:8 + n])
    assert _same_bf16(out[8:8 + n].cpu(), v.to(torch.bfloat16))
    assert bool((out[:8] == 3.0).all() and (out[8 + n:] == 3.0).all())
    ops.grad_unpack_bf16(out[8:8 + n], buf[off:off + n])
    assert bool((buf[:off] == 5.0).all() and (buf[off + n:] == 5.0).all())
    assert _same_bf16(buf[off:off + n].cpu().to(torch.bfloat16), v.to(torch.bfloat16))
    keep_b, keep_o = buf.clone(), out.clone()
    with pytest.raises(ValueError, match="asis_grad_pack_bf16"):       # n % 4 != 0
        ops.grad_pack_bf16(buf[off:off + 1026], out[8:8 + 1026])
    with pytest.raises(ValueError, match="asis_grad_pack_bf16"):       # a gradient range that does not start on 16 bytes
        ops.grad_pack_bf16(buf[1:1 + n], out[8:8 + n])
    with pytest.raises(ValueError, match="asis_grad_unpack_bf16"):
        ops.grad_unpack_bf16(out[8:8 + 1026], buf[off:off + 1026])
    with pytest.raises(ValueError, match="asis_grad_unpack_bf16"):
        ops.grad_unpack_bf16(out[8:8 + n], buf[1:1 + n])
    with pytest.raises(ValueError, match="asis_grad_unpack_bf16"):     # bf16 side off its 8 bytes
        ops.grad_unpack_bf16(out[1:1 + n], buf[off:off + n])
    torch.cuda.synchronize()
    assert torch.equal(keep_b.view(torch.int32), buf.view(torch.int32)) and torch.equal(keep_o.view(torch.int16), out.view(torch.int16))


@gpu
@pytest.mark.parametrize("n,off", [(1003, 0), (4099, 1), (3, 0), ((1 << 21) + 6, 0)])
def test_sgd_guarded_skips_exactly(dev, n, off):
    """guard clear: the guarded entry IS sgd_momentum; guard set by one non-finite element anywhere: p and buf keep their
    bits and guard[1] counts one skipped step per counting call.  ``off``: the scalar kernels (a view one element in)"""
    gen = _gen(7, n, off)

    def view(t):
        return torch.empty(n + off, device=dev)[off:].copy_(t)

    p0, b0, g0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 64
    guard = torch.zeros(2, device=dev, dtype=torch.int32)
    for first in (True, False):
        pa, ba, pb, bb, gd = view(p0), view(b0), view(p0), view(b0), view(g0)
        ops.sgd_momentum(pa, gd, ba, 0.01, 0.9, 3e-5, 1 / 64, first)
        ops.grad_guard(gd, guard, True)
        ops.sgd_momentum(pb, gd, bb, 0.01, 0.9, 3e-5, 1 / 64, first, guard)
        assert torch.equal(pa, pb) and torch.equal(ba, bb) and guard.tolist() == [0, 0]
        pr = p0.double()
        gr = g0.double() / 64 + 3e-5 * pr
        br = gr if first else 0.9 * b0.double() + gr
        assert rel_l2(pa, pr - 0.01 * br) < 1e-6 and rel_l2(ba, br) < 1e-6
    skipped = 0
    for pos in sorted({0, n // 2, n - 1, n - (n % 4 or 1)}):
        for bad in (float("nan"), float("inf"), float("-inf")):
            p, buf, gd = view(p0), view(b0), view(g0)
            gd[pos] = bad
            ops.grad_guard(gd, guard, True)
            assert int(guard[0]) == 1, (pos, bad)
            ops.sgd_momentum(p, gd, buf, 0.01, 0.9, 3e-5, 1 / 64, False, guard, count_skip=True)
            skipped += 1
            assert guard.tolist() == [1, skipped]
            ops.sgd_momentum(p, gd, buf, 0.01, 0.9, 3e-5, 1 / 64, False, guard, count_skip=False)
            assert guard.tolist() == [1, skipped]
            assert torch.equal(p.cpu(), p0) and torch.equal(buf.cpu(), b0)
    ops.grad_guard(view(g0), guard, True)          # a clean gradient clears the flag and keeps the count
    assert guard.tolist() == [0, skipped]


@gpu
@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("R,D,ld", [(1, 64, 72), (31, 64, 64), (32, 64, 72), (33, 1028, 1032), (65536, 64, 72), (65537, 64, 64),
                                    (65569, 64, 72)])
def test_cast_colsum(dev, dt, R, D, ld):
    """R around the row-block rule (32 rows a block, 2048 blocks at the most); D = 1028 takes the wide instantiation"""
    assert _lib.lib().asis_rowblock_nblk(R) == min(-(-R // 32), 2048)
    gen = _gen(8, R, D)
    x = torch.randn(R, D, generator=gen) + 0.3
    big = torch.full((R, ld), float("nan"), device=dev)
    big[:, :D] = x.to(dev)
    out, partial = ops.cast_colsum(big[:, :D], dt, 0.37)
    assert partial.shape[0] == min(-(-R // 32), 2048)
    assert torch.equal(out.cpu().view(torch.int16), (x * 0.37).to(dt).view(torch.int16))
    ref = x.double().sum(0)
    bound, yard = _bound(x.sum(0), ref, U_SUM)
    err = _err(ops.reduce_rows(partial), ref)
    _report("cast_colsum", (R, D), err, bound, yard)
    assert err <= bound


@gpu
@pytest.mark.parametrize("dt,width", [(torch.float16, 24), (torch.bfloat16, 40), (torch.float32, 12), (torch.float32, 20),
                                      (torch.float16, 8)])
def test_copy_channels(dev, dt, width):
    rows, ls, ld = 37, 56, 48
    gen = _gen(9, width)
    src = torch.randn(rows, ls, generator=gen).to(dt).to(dev)
    dst = torch.full((rows, ld), 2.0, device=dev, dtype=dt)
    s0, d0 = (ls - width) // 8 * 8, 8
    ops.copy_channels(src[:, s0:s0 + width], dst[:, d0:d0 + width])
    want = torch.full((rows, ld), 2.0, dtype=dt)
    want[:, d0:d0 + width] = src.cpu()[:, s0:s0 + width]
    assert torch.equal(dst.cpu(), want)


@gpu
def test_copy_channels_refuses_odd_widths(dev):
    src = torch.zeros(4, 32, device=dev, dtype=torch.float16)
    dst = torch.ones(4, 32, device=dev, dtype=torch.float16)
    with pytest.raises(ValueError, match="asis_copy_channels"):
        ops.copy_channels(src[:, :12], dst[:, :12])          # 24 bytes a row
    with pytest.raises(ValueError, match="asis_copy_channels"):
        ops.copy_channels(src[:, 4:20], dst[:, :16])         # source 8 bytes off
    assert bool((dst == 1).all())


@gpu
def test_add_f32_batch_strides(dev):
    B, n, D = 3, 5, 12
    gen = _gen(10, B, n, D)
    a_all, b_all = torch.randn(B, n + 2, D, generator=gen).to(dev), torch.randn(B, n + 1, D, generator=gen).to(dev)
    a, b = a_all[:, 1:n + 1], b_all[:, 1:]                   # batch strides (n + 2) D and (n + 1) D
    out_all = torch.full((B, n + 3, D), 9.0, device=dev)
    got = ops.add_f32(a, b, out=out_all[:, 2:n + 2])
    assert torch.equal(got, a + b) and bool((out_all[:, :2] == 9).all() and (out_all[:, n + 2:] == 9).all())
    assert torch.equal(ops.add_f32(a, b), a + b)
    one = b_all[:1, 1:].expand(B, n, D)                      # batch stride 0: one tensor added to every sample
    assert torch.equal(ops.add_f32(a, one), a + one)


@gpu
@pytest.mark.parametrize("shape", [(8, 4, 3, 3), (8, 3, 3, 3), (64, 16, 1, 1), (4, 1, 7, 7)])
def test_conv_weight_absmax(dev, shape):
    """row length divisible by 4 ([Cout, rest] view) and not (one flat row)"""
    gen = _gen(11, *shape)
    w = torch.randn(*shape, generator=gen)
    w.view(-1)[w.numel() - 2] = -7.5                         # the maximum is a negative element near the end
    assert float(ops.conv_weight_absmax(w.to(dev))) == 7.5
    w2 = w.clone()
    w2.view(-1)[w.numel() - 2] = 0.0
    assert float(ops.conv_weight_absmax(w2.to(dev))) == float(w2.abs().max())


@gpu
@pytest.mark.parametrize("n", [1, 1003, 256 * 4096 + 5])
def test_scale_f32(dev, n):
    """asis_scale_f32 (the gradient bucket's in-place scale); the last size runs the grid-stride loop"""
    gen = _gen(12, n)
    x = torch.randn(n, generator=gen)
    xd = torch.full((n + 2,), 4.0, device=dev)
    xd[1:n + 1] = x.to(dev)
    _lib.check(_lib.lib().asis_scale_f32(torch.cuda.current_stream().cuda_stream, xd[1:].data_ptr(), n, 0.37), "asis_scale_f32")
    assert torch.equal(xd[1:n + 1].cpu(), x * 0.37) and float(xd[0]) == 4.0 and float(xd[n + 1]) == 4.0
