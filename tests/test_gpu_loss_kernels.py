"""csrc/loss.hip (with bilinear_tap.h) kernel by kernel, pixel by pixel, against plain torch float64 on the CPU: the bilinear
resize and its transpose, every (mode, n_region, n_ce) of the fused segmentation loss forward and backward, the validation
metrics and ``reduce_rows``, at non-square maps, one-pixel-wide maps, every grid cap and the limits of C and B*C.

References (all written here, none taken from oracle/):
  resize fwd   ``F.interpolate(x.double(), size, mode="bilinear", align_corners=False)``; its float64 autograd is the transpose.
  loss         resize -> n softmaxes -> I = sum q t, Sp = sum q, St = sum t per (b, c) -> the five formulas of the header of
               loss.hip / include/asis_hip.h; CE = ``F.cross_entropy(weight=...)`` on level n_ce - 1.  ``coef`` = d region / d I
               and d region / d Sp by autograd (q enters the region term through I and Sp only), the gradient is taken at the
               RESIZED logits; both times grad_scale.  eps and grad_scale enter the kernel as floats: the reference uses the
               float32 value of eps.  The backward kernel gets the ``coef`` its own forward produced (the production path).
  ce_acc       ``F.cross_entropy(reduction="none")`` and argmax of the float64 resized logits.  That comparison is discontinuous:
               the logits are nudged (``_nudge``; nothing is masked) until every pixel's top-two gap is >= 2e-3; asserted >= 1e-3
               in float64 and in float32 on the CPU by test_input_rules.  Exact ties are a case of their own (integer logits).

Bounds.  None is taken from what the kernels give.  ulp = 2^-23; Y = the error of the SAME operation evaluated by torch in float32
on the CPU against float64 (same float32 source index, so it carries the error of the tap weights, ~ulp(source coordinate) times
the difference of neighbouring values); fp32 outputs: err <= max(4 Y, U ulp max|ref|), U derived per output:
  resize fwd     U = 4: with exact weights (identity, 2x) what is left are the 3 products and 3 sums of ``blend_taps``.
  resize bwd     U = 4 + sqrt(nt), nt = (ceil(2 H / h) + 2) (ceil(2 W / w) + 2) >= the taps one source pixel gathers one after the
                 other in fp32: a chain of nt adds has an rms error of sqrt(nt) / 4.9 ulps, sqrt(nt) is its 5 sigma.  One dropped
                 tap is 1 / nt of a value: >= 2^23 / nt ulps.
  column sums    U = 16 as in test_gpu_bn_bwd (per-thread chain of <= 2 pixels, wave tree, double from there on); dz has mean 0.5,
                 so the sums do not cancel.
  softmax_c      ``__expf(x)`` = exp2(x log2 e): the rounded difference x = z - max and the rounded product each move the result
                 by |x| 2^-24 relative, the instruction by 1 ulp: (|x| + 1) ulps per term, the same again through the sum, the
                 chain of C - 1 adds, the division and the product:  E(D, C) = 2 (D + 1) + (C - 1) / 2 + 2 ulps of a probability,
                 D = max over pixels of (max_c z - min_c z) of the float64 resized logits.  The second softmax sees inputs in [0, 1]
                 (D = 1) that are off by E(D, C) ulps of 1; the shift by the maximum cancels, a convex combination remains:
                 U_q(n) = 0, E(D, C), 2 E(D, C) + E(1, C) for n = 0, 1, 2 softmaxes.
  sums I, Sp     element by element, relative.  E(D, C) is a worst case per pixel; over the pixels of a sum the rounding of
                 x log2 e, of the chain, the division and the product are independent, so they enter with 5 sigma of their sum,
                 5 rho U_q(n_region), rho = max over (b, c) of sqrt(sum q^2) / sum |q| from the reference (1 / sqrt(pixels that
                 count)); what may be one-sided stays whole: 4 ulps a softmax level (the exp instruction's 1 ulp on the term and
                 on the sum, the division, the product).  Accumulation: a per-thread chain of <= 16 pixels and 6 + 2 tree levels,
                 24 roundings, rms sqrt(24) / 4.9 = 1 ulp, 5 sigma and the final rounding: 6; the blend: 4.
                 U_s = kappa (4 n_region + 5 rho U_q(n_region) + 4 + 6).  Probabilities are positive (kappa = 1); raw logits
                 (n_region = 0) are not: kappa = max sum|term| / |sum term| from the reference.  St is a count: EQUAL.
  coef           relative, element by element: U_c = 3 U_s + 2 (I / S^2-like: 2 U_s from the denominator, U_s from the numerator);
                 soft IoU: 7 U_s + 2, its U = Sp + St - I >= (Sp + St + I) / 3 costs a factor 3 on the denominator's share.
                 Mode 4 has no region coefficient (EQUAL 0); the CE scale grad_scale / sum w alone is left, a sum of positive
                 weights: worst case (16 + 7) / 2 + 1 = 13.
  loss           ulp (4 U_s mean|term| + U_ce + 6 |CE| + |loss|), U_ce = 2 + 5 rho_w (C + 3 + 2 A (+ 2 E(D, C) if n_ce = 2)): the
                 per-pixel nll = log(sum exp) - (z_t - max) with accurate expf / logf, A = max |input of that softmax|, averaged
                 with rho_w = sqrt(sum w^2) / sum w over the pixels; 2 for what may be one-sided in expf / logf.
  dz             per (b, c) PLANE: err_p <= max(4 Y_p, U_b ulp max|ref_p|).  An element is one pixel, nothing averages:
                 U_b = [U_c unless mode 4] + [13 if n_ce: the CE scale] + 3 U_q(max(n_region, n_ce)) + C + 4: the coefficient
                 where the kernel reads one, the probabilities of up to three factors of a softmax-backward product, the dot
                 product over C.  CE-only gradients carry no term of the sums.
  ce_acc         red[0]: ulp (2 sum w + 5 (C + 3 + 2 A) sqrt(sum w^2) + 6 |ref|): ``__expf`` terms are <= 1 and their (|x| + 1)-ulp
                 error shrinks with e^-|x|, so sum exp is off by <= C ulps, ``__logf`` by 2, the two fp32 adds of m + log - z_t by
                 2 A, independent from pixel to pixel (5 sigma); 2 a pixel for what may be one-sided; 6 = the accumulation as
                 above.  red[1] with weights: <= 9 pixels a thread and 8 tree levels, worst case 9.  red[1] without weights,
                 red[2] and the counts: EQUAL.
  reduce_rows    positive summands, double accumulation, one rounding: err <= half the float32 spacing at the result
                 + n 2^-52 |ref| for the double sums on either side.
  16-bit outputs |out - ref| <= h |ref| + 2^-25 (fp16) + (fp32 bound): h = 2^-11 / 2^-8 (hi), 2^-21 / 2^-15 (hi + lo).
  bit-exact      identity resize fwd / bwd, St, counts, grad_scale 1024 against 1, two calls, pad channels, B = C = 1.

Measured on one MI355X, the case with the largest err / bound per output (all cases: run with ``-s``, every check prints a
MEASURE line before the test asserts):

    output                  worst case                                 err        Y (float32)  bound      err / bound
    ce_acc.den              (2, 24, 20, 56, 70, 11, True)              3.168e-04  1.715e-04    7.734e-03  0.041
    ce_acc.num              (2, 24, 20, 56, 70, 11, False)             7.150e-04  7.150e-04    1.380e-02  0.052
    loss.coef               (down_up, tversky)                         3.489e-07  4.618e-07    6.970e-06  0.050
    loss.dz                 (many, softdice)                           3.602e-08  3.462e-08    1.385e-07  0.260
    loss.loss               (down_up, ce_dc)                           2.952e-07  5.682e-08    3.720e-06  0.079
    loss.sums.I             (down_up, ce)                              4.125e-07  3.599e-07    2.045e-06  0.202
    loss.sums.Sp            (down_up, ce)                              4.499e-07  4.499e-07    2.045e-06  0.220
    reduce_rows             (64, 2048)                                 1.000e+00  -            1.000e+00  1.000
    reduce_rows.scaled      (1, 2048)                                  9.995e-01  -            1.000e+00  1.000
    resize.adjoint          (2, 1, 1, 7, 5, 16)                        2.710e-05  -            5.678e-03  0.005
    resize_bwd.bf16.hi      (1, 725, 730, 1450, 1460, 2)               9.955e-01  1.349e-06    1.000e+00  0.995
    resize_bwd.bf16.hi+lo   (1, 1025, 1024, 513, 512, 2)               2.399e-01  6.938e-05    1.000e+00  0.240
    resize_bwd.colsum       (2, 13, 11, 6, 1, 3)                       7.153e-07  2.384e-07    1.225e-05  0.058
    resize_bwd.f16.hi       (2, 588, 588, 294, 294, 1)                 9.923e-01  0.000e+00    1.000e+00  0.992
    resize_bwd.f16.hi+lo    (2, 588, 588, 882, 882, 1)                 2.497e-01  3.734e-04    1.000e+00  0.250
    resize_bwd.f32          (2, 20, 20, 28, 28, 8)                     4.897e-06  4.897e-06    1.959e-05  0.250
    resize_fwd              (2, 13, 11, 6, 1, 3)                       1.748e-06  1.689e-06    6.755e-06  0.259

(16-bit rows: element error / element limit, the limit being half an ulp of the type on top of the fp32 bound, so values near 1
are the rounding of the type itself; reduce_rows likewise against half the float32 spacing, 1.000 being a sum that lies exactly
between two floats.  Where err equals Y the error is the float32 source coordinate's, which the kernel and torch share.)
All 564 bit-exact checks hold; the whole file takes 5 s of pytest time on the GPU machine, 9 s of wall time.
"""
import functools
import math
import re

import pytest
import torch
import torch.nn.functional as F

from adaptersis_amd import _lib, ops
from tests.bound_helpers import DT, HALF, PAIR, SUBN, ULP32, U_ELEM, U_SUM, _bound, _err, _gen

gpu = pytest.mark.gpu
TAG = {torch.float16: "f16", torch.bfloat16: "bf16"}


def _nblk_loss(H: int, W: int) -> int:
    return max(1, min(-(-H * W // 2048), 512))


class _Checks:
    """prints every MEASURE line first, asserts at the end: one miss does not hide the figures of the outputs after it"""

    def __init__(self, case):
        self.case, self.fails = case, []

    def add(self, name, err, bound, yard=float("nan")):
        ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        print(f"MEASURE {name} {self.case}: err {err:.3e} yard {yard:.3e} bound {bound:.3e} ratio {ratio:.3f}")
        if not err <= bound:
            self.fails.append((name, err, bound, yard))

    def absolute(self, name, got, ref, f32, ulps, extra=0.0):
        """the scheme of test_gpu_bn_bwd: max(4 Y, U ulp max|ref|) over the whole output"""
        bound, yard = _bound(f32, ref, ulps)
        self.add(name, _err(got, ref), max(bound, extra), yard)

    def relative(self, name, got, ref, f32, ulps):
        """the same scheme element by element, relative to each |ref|; where ref == 0 the output must be 0"""
        got, nz = got.detach().double().cpu(), ref != 0
        if bool((~nz).any()):
            self.add(name + ".zeros", float(got[~nz].abs().max()), 0.0)
        if bool(nz.any()):
            yard = float(((f32.double() - ref)[nz] / ref[nz]).abs().max())
            self.add(name, float(((got - ref)[nz] / ref[nz]).abs().max()), max(4 * yard, ulps * ULP32), yard)

    def exact(self, name, ok):
        print(f"MEASURE {name} {self.case}: exact {bool(ok)}")
        if not ok:
            self.fails.append((name, "not bit-equal"))

    def done(self):
        assert not self.fails, (self.case, self.fails)


# ---------------------------------------------------------------------------------------------------------------------------
# 1 / 4: the resize and its transpose
RESIZE_CASES = [  # (B, h, w, H, W, C)
    (2, 20, 20, 28, 28, 8),           # up (the size test_gpu_kernels2 has)
    (2, 48, 40, 42, 30, 3),           # down; C = 3: 5 pad channels in the 16-bit transpose
    (2, 36, 31, 36, 31, 16),          # identity, MAXC: no pad
    (1, 17, 40, 51, 23, 8),           # up in y, down in x
    (1, 40, 17, 23, 51, 11),          # down in y, up in x; CP = 16
    (3, 1, 9, 5, 14, 1),              # h = 1
    (3, 9, 1, 14, 5, 3),              # w = 1
    (2, 1, 1, 7, 5, 16),              # one source pixel: every output pixel is a tap of it
    (2, 13, 11, 1, 6, 8),             # H = 1
    (2, 13, 11, 6, 1, 3),             # W = 1
    (1, 5, 6, 40, 90, 11),            # strong up: 16 x 30 + margins taps per source pixel
    (2, 588, 588, 882, 882, 1),       # or_unet._rescale 1.5: planes of one channel
    (2, 588, 588, 294, 294, 1),       # or_unet._rescale 0.5
    (1, 725, 730, 1450, 1460, 2),     # 2 117 000 output pixels > 8192 x 256: the forward's grid-stride loop runs twice
    (1, 1025, 1024, 513, 512, 2),     # 1 049 600 source pixels > 4096 x 256: the transpose's loop runs twice
]


@functools.lru_cache(maxsize=None)
def _resize_ref(B, h, w, H, W, C):
    gen = _gen(21, B, h, w, H, W, C)
    x = torch.randn(B, h, w, C, generator=gen) * 2.0
    dz = torch.randn(B, H, W, C, generator=gen) + 0.5
    out = {}
    for dt in (torch.float64, torch.float32):
        xs = x.to(dt).permute(0, 3, 1, 2).requires_grad_()
        y = F.interpolate(xs, size=(H, W), mode="bilinear", align_corners=False)
        y.backward(dz.to(dt).permute(0, 3, 1, 2))
        out[dt] = (y.detach().permute(0, 2, 3, 1), xs.grad.permute(0, 2, 3, 1))
    return x, dz, out[torch.float64], out[torch.float32]


def _u_taps(h, w, H, W) -> float:
    return U_ELEM + math.sqrt((-(-2 * H // h) + 2) * (-(-2 * W // w) + 2))


@gpu
@pytest.mark.parametrize("B,h,w,H,W,C", RESIZE_CASES)
def test_resize_bilinear_fwd(dev, B, h, w, H, W, C):
    x, _, (y64, _), (y32, _) = _resize_ref(B, h, w, H, W, C)
    ck = _Checks((B, h, w, H, W, C))
    y = ops.resize_bilinear_fwd(x.to(dev), H, W)
    ck.absolute("resize_fwd", y, y64, y32, U_ELEM)
    ck.exact("resize_fwd.again", torch.equal(y, ops.resize_bilinear_fwd(x.to(dev), H, W)))
    if (h, w) == (H, W):
        ck.exact("resize_fwd.identity", torch.equal(y.cpu(), x))
    ck.done()


@gpu
def test_resize_bilinear_fwd_refuses_17_channels(dev):
    x = torch.zeros(1, 4, 4, 17, device=dev)
    with pytest.raises(ValueError, match="asis_resize_bilinear_fwd"):
        ops.resize_bilinear_fwd(x, 8, 8)
    with pytest.raises(ValueError, match="asis_resize_bilinear_bwd"):
        ops.resize_bilinear_bwd(x, 2, 2, torch.float32)


@gpu
@pytest.mark.parametrize("B,h,w,H,W,C", RESIZE_CASES)
def test_resize_bilinear_bwd(dev, B, h, w, H, W, C):
    """every output form of the transpose, the partial column sums (the weights of one output pixel sum to 1, so they are the
    column sums of dz itself) and the adjoint identity between the two kernels"""
    x, dz, (y64, g64), (y32, g32) = _resize_ref(B, h, w, H, W, C)
    ck = _Checks((B, h, w, H, W, C))
    ut = _u_taps(h, w, H, W)
    b32, yard = _bound(g32, g64, ut)
    dzd = dz.to(dev)
    g, partial = ops.resize_bilinear_bwd(dzd, h, w, torch.float32)
    nblk = min(-(-B * h * w // 256), 4096)
    assert _lib.lib().asis_resize_bwd_nblk(B * h * w) == nblk == partial.shape[0]
    if B * h * w > 4096 * 256:
        assert nblk == 4096
    ck.absolute("resize_bwd.f32", g, g64, g32, ut)
    ck.exact("resize_bwd.shape", tuple(g.shape) == (B, h, w, C))
    g2, partial2 = ops.resize_bilinear_bwd(dzd, h, w, torch.float32)
    ck.exact("resize_bwd.again", torch.equal(g, g2) and torch.equal(partial, partial2))
    cs64 = dz.double().sum((0, 1, 2))
    ck.absolute("resize_bwd.colsum", ops.reduce_rows(partial), cs64, g32.double().sum((0, 1, 2)).float(), U_SUM)
    # <resize_fwd(x), dz> = <x, resize_bwd(dz)> in float64 from the two kernels' fp32 outputs
    y = ops.resize_bilinear_fwd(x.to(dev), H, W)
    lhs = float((y.double().cpu() * dz.double()).sum())
    rhs = float((x.double() * g.double().cpu()).sum())
    bfwd, _ = _bound(y32, y64, U_ELEM)
    ck.add("resize.adjoint", abs(lhs - rhs), bfwd * float(dz.abs().sum()) + b32 * float(x.abs().sum()))
    CP = (C + 7) // 8 * 8
    for dt in DT:
        hi, lo, partial16 = ops.resize_bilinear_bwd(dzd, h, w, dt, split=True)
        plain, _ = ops.resize_bilinear_bwd(dzd, h, w, dt)
        ck.exact(f"resize_bwd.{TAG[dt]}.forms", tuple(hi.shape) == (B, h, w, CP) and torch.equal(hi, plain)
                 and torch.equal(partial16, partial))
        if CP > C:
            ck.exact(f"resize_bwd.{TAG[dt]}.pad", not bool(hi[..., C:].view(torch.int16).any())
                     and not bool(lo[..., C:].view(torch.int16).any()))
        for name, got, rel in (("hi", hi.double().cpu(), HALF[dt]), ("hi+lo", hi.double().cpu() + lo.double().cpu(), PAIR[dt])):
            e = (got[..., :C] - g64).abs()
            lim = rel * g64.abs() + SUBN[dt] + b32
            ck.add(f"resize_bwd.{TAG[dt]}.{name}", float((e / lim).max()), 1.0, yard)
        if (h, w) == (H, W):
            ck.exact(f"resize_bwd.{TAG[dt]}.identity", torch.equal(hi[..., :C].cpu().view(torch.int16), dz.to(dt).view(torch.int16)))
    if (h, w) == (H, W):
        ck.exact("resize_bwd.identity", torch.equal(g.cpu(), dz))
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------
# 2 / 3: the fused losses
LOSSES = {  # name -> (n_region, mode, eps, n_ce, weighted): SegTrainer.LOSSES and the two CE-only forms of segloss
    "dice": (2, ops.LOSS_DICE, 10e-20, 0, False), "iou": (2, ops.LOSS_IOU, 1e-6, 0, False),
    "softdice": (1, ops.LOSS_SOFTDICE, 1.0, 0, False), "dc_and_ce": (1, ops.LOSS_SOFTDICE, 1.0, 2, False),
    "tversky": (1, ops.LOSS_TVERSKY, 1.0, 0, False), "ce_dc": (1, ops.LOSS_DICE, 10e-20, 1, False),
    "ce": (0, ops.LOSS_NONE, 0.0, 1, False), "ce_weighted": (0, ops.LOSS_NONE, 0.0, 1, True),
}
MODE_EPS = {0: 1e-19, 1: 1e-6, 2: 1.0, 3: 1.0, 4: 0.0}
COMBOS = [(m, r, c) for m in range(4) for r in range(3) for c in range(3)] + [(4, 0, 1), (4, 0, 2)]
COMBO_SHAPE = (2, 5, 14, 23, 45, 52, "plain")        # 2340 pixels: 2 blocks an image
LOSS_SHAPES = {  # name -> (B, C, h, w, H, W, target kind); nblk = ceil(H W / 2048), 512 at the most
    "nblk1": (2, 3, 9, 7, 31, 45, "plain"),               # 1395 pixels
    "nblk2": (2, 5, 20, 33, 50, 70, "plain"),             # 3500
    "many": (2, 11, 60, 50, 150, 131, "plain"),           # 19650: 10 blocks
    "down_up": (1, 8, 200, 90, 120, 130, "plain"),        # 15600: 8 blocks, down in y and up in x
    "cap512": (1, 2, 103, 128, 1025, 1024, "plain"),      # 1 049 600 > 512 x 2048: 9 pixels a thread
    "bc256_16x16": (16, 16, 6, 5, 40, 60, "plain"),       # the finalize block is full, MAXC
    "bc256_128x2": (128, 2, 5, 6, 48, 50, "plain"),
    "b1c1": (1, 1, 7, 9, 50, 47, "plain"),
    "missing": (2, 4, 12, 10, 56, 40, "missing"),         # class 2 absent from image 0 only, class 3 from image 1 only
    "allbg": (2, 3, 10, 12, 44, 50, "allbg"),             # image 0 is background alone (eps 1e-19: dice, ce_dc; eps 1: softdice..)
}
LOSS_NBLK = {"nblk1": 1, "nblk2": 2, "many": 10, "down_up": 8, "cap512": 512, "bc256_16x16": 2, "bc256_128x2": 2, "b1c1": 2,
             "missing": 2, "allbg": 2}
GS = 1024.0


@functools.lru_cache(maxsize=4)
def _loss_inputs(B, C, h, w, H, W, kind):
    gen = _gen(22, B, C, h, w, H, W)
    lg = torch.randn(B, h, w, C, generator=gen) * 1.5 + 1.5 + torch.randn(C, generator=gen) * 0.5     # mean > 0: raw-logit sums
    coarse = torch.randint(0, C, (B, -(-H // 4), -(-W // 4)), generator=gen)                           # do not cancel
    tg = coarse.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :H, :W].contiguous()
    flip = torch.rand(B, H, W, generator=gen) < 0.1
    tg = torch.where(flip, torch.randint(0, C, (B, H, W), generator=gen), tg)
    if kind == "missing":
        tg[0] = torch.where(tg[0] == 2, 0, tg[0])
        tg[1] = torch.where(tg[1] == 3, 1, tg[1])
    if kind == "allbg":
        tg[0] = 0
    wts = torch.linspace(0.2, 2.0, C)
    if C > 1:
        wts[1] = 0.0                                       # one class without weight
    return lg, tg.contiguous(), wts


def _loss_ref(lg, tg, n_region, mode, eps, n_ce, wts, dtype):
    """-> dict of loss, sums [B, C, 3], coef [B*C*2 + 1], dz [B, H, W, C] (both times GS), D, A, kappa, mean|term|, |CE|"""
    B, h, w, C = lg.shape
    H, W = tg.shape[1:]
    x0 = F.interpolate(lg.to(dtype).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).requires_grad_()
    x1 = torch.softmax(x0, 1)
    lv = [x0, x1, torch.softmax(x1, 1)]
    t = F.one_hot(tg, C).permute(0, 3, 1, 2).to(dtype)
    q = lv[n_region]
    I, Sp, St = (q * t).sum((2, 3)), q.sum((2, 3)), t.sum((2, 3))
    I.retain_grad(), Sp.retain_grad()
    e = float(torch.tensor(eps, dtype=torch.float32))
    zero = x0.sum() * 0
    if mode == 0:
        term = 2 * I / (Sp + St + e)
        region = 1 - term.mean()
    elif mode == 1:
        term = (I + e) / (Sp + St - I + e)
        region = (1 - term).mean()
    elif mode == 2:
        term = (2 * I + e) / (Sp + St + e)
        region = -term.mean()
    elif mode == 3:
        term = (I + e) / (I + 0.3 * (Sp - I) + 0.7 * (St - I) + e)
        region = -term.mean()
    else:
        term, region = I * 0, zero
    ce = F.cross_entropy(lv[n_ce - 1], tg, weight=None if wts is None else wts.to(dtype)) if n_ce else zero
    loss = region + ce
    (loss * GS).backward()
    c0 = I.grad if I.grad is not None else torch.zeros_like(I)
    c1 = Sp.grad if Sp.grad is not None else torch.zeros_like(Sp)
    wsum = float(B * H * W) if wts is None else float(wts.double()[tg].sum())
    coef = torch.cat([torch.stack([c0, c1], -1).reshape(-1), torch.tensor([GS / wsum if n_ce else 0.0], dtype=dtype)])
    d, qd = x0.detach(), q.detach()
    kap, rho = 1.0, 0.0
    for s, a, a2 in ((I, (qd.abs() * t).sum((2, 3)), (qd * qd * t).sum((2, 3))), (Sp, qd.abs().sum((2, 3)), (qd * qd).sum((2, 3)))):
        nz = s.detach() != 0
        if bool(nz.any()):
            rho = max(rho, float((a2[nz].sqrt() / a[nz]).max()))          # sqrt(sum q^2) / sum |q|: 1 / sqrt(pixels that count)
            if n_region == 0:
                kap = max(kap, float((a[nz] / s.detach()[nz].abs()).max()))
    wpix = torch.ones(B, H, W, dtype=torch.float64) if wts is None else wts.double()[tg]
    return dict(loss=loss.detach(), sums=torch.stack([I, Sp, St], -1).detach(), coef=coef.detach(),
                dz=x0.grad.permute(0, 2, 3, 1), D=float((d.amax(1) - d.amin(1)).max()), A=float(d.abs().max()), kappa=kap, rho=rho,
                rho_ce=float(wpix.pow(2).sum().sqrt() / wpix.sum()),
                term=float(term.detach().abs().mean()), ce=abs(float(ce.detach())))


def _E(D: float, C: int) -> float:
    return 2 * (D + 1) + (C - 1) / 2 + 2


def _u_q(n: int, D: float, C: int) -> float:
    return (0.0, _E(D, C), 2 * _E(D, C) + _E(1.0, C))[n]


def _check_loss(dev, case, shape, n_region, mode, eps, n_ce, weighted, nblk=None):
    B, C, h, w, H, W, kind = shape
    if nblk is not None:       # the case keeps its purpose
        assert _lib.lib().asis_dice_nblk(H, W) == nblk == _nblk_loss(H, W), (H, W, nblk)
    lg, tg, wts = _loss_inputs(*shape)
    wts = wts if weighted else None
    r64 = _loss_ref(lg, tg, n_region, mode, eps, n_ce, wts, torch.float64)
    r32 = _loss_ref(lg, tg, n_region, mode, eps, n_ce, wts, torch.float32)
    D, A = r64["D"], r64["A"]
    u_s = r64["kappa"] * (4 * n_region + 5 * r64["rho"] * _u_q(n_region, D, C) + 4 + 6)
    u_c = 13.0 if mode == 4 else (7 if mode == 1 else 3) * u_s + 2
    u_ce = 0.0 if n_ce == 0 else 2 + 5 * r64["rho_ce"] * (C + 3 + 2 * (A if n_ce == 1 else 1.0) + (2 * _E(D, C) if n_ce == 2 else 0.0))
    u_b = (0.0 if mode == 4 else u_c) + (13 if n_ce else 0) + 3 * _u_q(max(n_region, n_ce), D, C) + C + 4
    ck = _Checks(case)
    lgd, tgd, wd = lg.to(dev), tg.to(dev), None if wts is None else wts.to(dev)
    loss, coef, sums = ops.seg_loss_fwd(lgd, tgd, n_region, mode, eps, n_ce, wd, GS)
    dz = ops.seg_loss_bwd(lgd, tgd, coef, n_region, mode, n_ce, wd)
    # --- forward
    ck.exact("loss.St", torch.equal(sums[..., 2].cpu().long(), torch.stack([torch.bincount(tg[b].reshape(-1), minlength=C)
                                                                             for b in range(B)])))
    for k, name in ((0, "I"), (1, "Sp")):
        ck.relative(f"loss.sums.{name}", sums[..., k], r64["sums"][..., k], r32["sums"][..., k], u_s)
    ck.relative("loss.coef", coef, r64["coef"], r32["coef"], u_c)
    floor = ULP32 * (4 * u_s * r64["term"] + u_ce + 6 * r64["ce"] + abs(float(r64["loss"])))
    ck.absolute("loss.loss", loss.reshape(()), r64["loss"], r32["loss"], 0, floor)
    loss1, coef1, sums1 = ops.seg_loss_fwd(lgd, tgd, n_region, mode, eps, n_ce, wd, 1.0)
    ck.exact("loss.grad_scale", torch.equal(coef, coef1 * GS) and torch.equal(loss, loss1) and torch.equal(sums, sums1))
    loss2, coef2, sums2 = ops.seg_loss_fwd(lgd, tgd, n_region, mode, eps, n_ce, wd, GS)
    ck.exact("loss.again", torch.equal(loss, loss2) and torch.equal(coef, coef2) and torch.equal(sums, sums2)
             and torch.equal(dz, ops.seg_loss_bwd(lgd, tgd, coef, n_region, mode, n_ce, wd)))
    # --- backward, plane by plane
    got, ref, f32 = dz.double().cpu(), r64["dz"], r32["dz"].double()
    err_p, y_p, top_p = (got - ref).abs().amax((1, 2)), (f32 - ref).abs().amax((1, 2)), ref.abs().amax((1, 2))
    lim_p = torch.maximum(4 * y_p, u_b * ULP32 * top_p)
    ratio = torch.where(lim_p > 0, err_p / lim_p.clamp_min(1e-300), torch.where(err_p == 0, 0.0, float("inf")).double())
    b, c = divmod(int(ratio.argmax()), C)
    print(f"MEASURE loss.dz {case}: worst plane b {b} c {c} err {float(err_p[b, c]):.3e} yard {float(y_p[b, c]):.3e} "
          f"bound {float(lim_p[b, c]):.3e} ratio {float(ratio.max()):.3f}  (plane maxima {float(top_p.min()):.2e} .. {float(top_p.max()):.2e})")
    if not float(ratio.max()) <= 1.0:
        ck.fails.append(("loss.dz", b, c, float(err_p[b, c]), float(lim_p[b, c])))
    if B == 1 and C == 1:
        if n_region >= 1 or mode == 4:      # the softmax of one class is exactly 1
            ck.exact("loss.dz.b1c1", not bool(dz.view(torch.int32).any()) or float(dz.abs().max()) == 0.0)
        else:                               # raw logits: coef0 t + coef1, t = 1 everywhere
            ck.exact("loss.dz.b1c1", torch.equal(dz, (coef[0] + coef[1]).expand_as(dz)))
    ck.done()


@gpu
@pytest.mark.parametrize("mode,n_region,n_ce", COMBOS)
def test_seg_loss_all_combinations(dev, mode, n_region, n_ce):
    """the 38 valid (mode, n_region, n_ce), class weights (one zero) wherever there is a CE term, two blocks an image"""
    assert len(COMBOS) == 38
    _check_loss(dev, (mode, n_region, n_ce), COMBO_SHAPE, n_region, mode, MODE_EPS[mode], n_ce, n_ce > 0, 2)


@gpu
@pytest.mark.parametrize("name", list(LOSSES))
@pytest.mark.parametrize("shape", list(LOSS_SHAPES))
def test_seg_loss_named_at_edges(dev, shape, name):
    n_region, mode, eps, n_ce, weighted = LOSSES[name]
    _check_loss(dev, (shape, name), LOSS_SHAPES[shape], n_region, mode, eps, n_ce, weighted, LOSS_NBLK[shape])


@gpu
@pytest.mark.parametrize("mode,n_ce", [(0, 0), (1, 0), (2, 1), (3, 2)])
def test_seg_loss_single_class_raw_logits(dev, mode, n_ce):
    """B = C = 1 on the raw logits: dz = coef0 t + coef1 with t = 1 at every pixel, the CE part is exactly 0"""
    _check_loss(dev, ("b1c1", mode, 0, n_ce), LOSS_SHAPES["b1c1"], 0, mode, MODE_EPS[mode], n_ce, n_ce > 0, 2)


@gpu
def test_seg_loss_refusals(dev):
    lg, tg = torch.zeros(2, 4, 4, 3, device=dev), torch.zeros(2, 8, 8, dtype=torch.int64, device=dev)
    big = lambda B, C: (torch.zeros(B, 2, 2, C, device=dev), torch.zeros(B, 4, 4, dtype=torch.int64, device=dev))   # noqa: E731
    cases = [("mode 4 without CE", "needs a CE term", lambda: ops.seg_loss_fwd(lg, tg, 1, ops.LOSS_NONE, 1.0, 0)),
             ("n_region 3", "n_region", lambda: ops.seg_loss_fwd(lg, tg, 3, ops.LOSS_DICE)),
             ("B*C 257 x 1", "B\\*C", lambda: ops.seg_loss_fwd(*big(257, 1), 1)),
             ("B*C 129 x 2", "B\\*C", lambda: ops.seg_loss_fwd(*big(129, 2), 1)),
             ("C 17", "C=", lambda: ops.seg_loss_fwd(*big(1, 17), 1)),
             ("int32 target", "contiguous int64", lambda: ops.seg_loss_fwd(lg, tg.int(), 1)),
             ("strided target", "contiguous int64",
              lambda: ops.seg_loss_fwd(lg, torch.zeros(2, 8, 16, dtype=torch.int64, device=dev)[:, :, ::2], 1)),
             ("short coef", "coef", lambda: ops.seg_loss_bwd(lg, tg, torch.zeros(12, device=dev), 1))]
    ck = _Checks("refusals")
    for name, pattern, call in cases:
        try:
            call()
            said = None
        except ValueError as e:
            said = str(e)
        ck.exact(f"loss.refuses.{name.replace(' ', '_')}", said is not None and re.search(pattern, said) is not None)
    torch.cuda.synchronize()
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------
# 5: validation metrics
CE_CASES = [  # (B, h, w, H, W, C, weighted)
    (2, 9, 13, 31, 22, 1, False),
    (2, 12, 17, 40, 33, 2, True),
    (2, 24, 20, 56, 70, 11, True),
    (2, 24, 20, 56, 70, 11, False),
    (1, 30, 22, 21, 35, 16, False),            # down in y, up in x
    (2, 730, 725, 1460, 1450, 2, True),        # 4 234 000 pixels > 2048 x 2048: 9 a thread.  Exactly 2x: the float32 taps are exact
]


def _gap(x0: torch.Tensor) -> torch.Tensor:
    """x0 NCHW -> the top-two gap per pixel (inf with one class)"""
    if x0.shape[1] == 1:
        return torch.full_like(x0[:, 0], float("inf"))
    top = x0.topk(2, dim=1).values
    return top[:, 0] - top[:, 1]


def _nudge(lg: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """raise the leading class at the taps of every pixel whose float64 top-two gap is below 2e-3, until none is left;
    no pixel is excluded from anything.  The step grows with the class index: two neighbours that share their taps and lead with
    different classes would otherwise be lifted together for ever."""
    if lg.shape[-1] == 1:
        return lg
    step = 8e-3 * (1 + 0.5 * torch.arange(lg.shape[-1], dtype=torch.float64))
    for _ in range(60):
        src = lg.double().permute(0, 3, 1, 2).clone().requires_grad_()
        x0 = F.interpolate(src, size=(H, W), mode="bilinear", align_corners=False)
        viol = _gap(x0.detach()) < 2e-3
        if not bool(viol.any()):
            return lg
        (x0.gather(1, x0.detach().argmax(1, keepdim=True)).squeeze(1) * viol).sum().backward()
        lg = (lg.double() + (src.grad > 0).permute(0, 2, 3, 1) * step).float()
    raise AssertionError("nudging did not converge")


@functools.lru_cache(maxsize=None)
def _ce_inputs(B, h, w, H, W, C):
    gen = _gen(23, B, h, w, H, W, C)
    lg = _nudge(torch.randn(B, h, w, C, generator=gen) * 2.0, H, W)
    x0 = F.interpolate(lg.double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
    tg = torch.where(torch.rand(B, H, W, generator=gen) < 0.6, x0.argmax(1), torch.randint(0, C, (B, H, W), generator=gen))
    wts = torch.linspace(0.3, 1.7, C)
    if C > 1:
        wts[C // 2] = 0.0
    return lg, tg.contiguous(), wts


def _ce_ref(lg, tg, wts, dtype):
    B, h, w, C = lg.shape
    H, W = tg.shape[1:]
    x0 = F.interpolate(lg.to(dtype).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
    wv = torch.ones(C, dtype=dtype) if wts is None else wts.to(dtype)
    num = F.cross_entropy(x0, tg, weight=wv, reduction="none").sum()
    pred = x0.argmax(1)
    cnt = torch.stack([torch.stack([(tg == c).sum(), (pred == c).sum(), ((tg == c) & (pred == c)).sum()]) for c in range(C)])
    return num, wv[tg].sum(), int((pred == tg).sum()), cnt, float(x0.abs().max())


def test_input_rules():
    """CPU: after nudging every pixel's top-two gap is >= 1e-3 in float64 AND in torch's float32 resize, both precisions pick
    the same class everywhere, and the reference counts cover every pixel (nothing is masked); the loss cases have the block
    counts their names claim and 38 distinct combinations"""
    for B, h, w, H, W, C, _ in CE_CASES:
        lg, tg, wts = _ce_inputs(B, h, w, H, W, C)
        x64 = F.interpolate(lg.double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
        x32 = F.interpolate(lg.permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
        assert float(_gap(x64).min()) >= 1e-3 and float(_gap(x32).min()) >= 1e-3, (B, h, w, H, W, C)
        assert torch.equal(x64.argmax(1), x32.argmax(1))
        _, _, correct, cnt, _ = _ce_ref(lg, tg, None, torch.float64)
        assert int(cnt[:, 0].sum()) == int(cnt[:, 1].sum()) == B * H * W and int(cnt[:, 2].sum()) == correct
        assert int(tg.min()) >= 0 and int(tg.max()) < C
        if C > 1:
            assert 0.3 < correct / (B * H * W) < 0.95                # right and wrong pixels are both populated
    # one case above every grid cap, so that each grid-stride loop runs more than once somewhere
    assert sum(B * H * W > 8192 * 256 for B, h, w, H, W, C in RESIZE_CASES) == 1          # resize_fwd_kernel
    assert sum(B * h * w > 4096 * 256 for B, h, w, H, W, C in RESIZE_CASES) == 1          # resize_bwd_kernel
    assert sum(B * H * W > 2048 * 2048 for B, h, w, H, W, C, _ in CE_CASES) == 1          # ce_acc_kernel: 2048 blocks of 8 pixels a thread
    assert any((h, w) == (H, W) for B, h, w, H, W, C in RESIZE_CASES)
    assert {C for B, h, w, H, W, C in RESIZE_CASES} >= {1, 3, 8, 11, 16} and {c[5] for c in CE_CASES} >= {1, 2, 11, 16}
    assert len(set(COMBOS)) == 38 and all(m != 4 or c > 0 for m, r, c in COMBOS)
    for name, (B, C, h, w, H, W, kind) in LOSS_SHAPES.items():
        assert _nblk_loss(H, W) == LOSS_NBLK[name] and B * C <= 256, name
    assert {LOSS_NBLK[n] for n in LOSS_SHAPES} >= {1, 2, 10, 512} and _nblk_loss(*COMBO_SHAPE[4:6]) == 2
    assert any(s[0] * s[1] == 256 and s[1] == 16 for s in LOSS_SHAPES.values()) and any(s[0] == 128 for s in LOSS_SHAPES.values())
    lg, tg, wts = _loss_inputs(*LOSS_SHAPES["missing"])
    assert not bool((tg[0] == 2).any()) and bool((tg[1] == 2).any()) and not bool((tg[1] == 3).any()) and bool((tg[0] == 3).any())
    assert float(wts[1]) == 0.0
    lg, tg, wts = _loss_inputs(*LOSS_SHAPES["allbg"])
    assert int(tg[0].max()) == 0 and int(tg[1].max()) == 2


@gpu
@pytest.mark.parametrize("B,h,w,H,W,C,weighted", CE_CASES)
def test_ce_acc(dev, B, h, w, H, W, C, weighted):
    lg, tg, wts = _ce_inputs(B, h, w, H, W, C)
    wts = wts if weighted else None
    n = B * H * W
    nblk = min(-(-n // 2048), 2048)
    assert _lib.lib().asis_ce_acc_nblk(n) == nblk and (n <= 2048 * 2048 or nblk == 2048)
    num64, den64, correct, cnt64, A = _ce_ref(lg, tg, wts, torch.float64)
    num32, den32, _, _, _ = _ce_ref(lg, tg, wts, torch.float32)
    ck = _Checks((B, h, w, H, W, C, weighted))
    wd = None if wts is None else wts.to(dev)
    red, cnt = ops.ce_acc(lg.to(dev), tg.to(dev), wd, counts=True)
    wpix = torch.ones(B, H, W, dtype=torch.float64) if wts is None else wts.double()[tg]
    ck.absolute("ce_acc.num", red[0], num64, num32, 0,
                ULP32 * (2 * float(den64) + 5 * (C + 3 + 2 * A) * float(wpix.pow(2).sum().sqrt()) + 6 * float(num64)))
    if weighted:
        ck.absolute("ce_acc.den", red[1], den64, den32, 9)
    else:
        ck.exact("ce_acc.den", float(red[1]) == n)
    ck.exact("ce_acc.correct", float(red[2]) == correct)
    ck.exact("ce_acc.counts", torch.equal(cnt.cpu().long(), cnt64))
    ck.exact("ce_acc.plain", torch.equal(ops.ce_acc(lg.to(dev), tg.to(dev), wd), red))
    # all one class: the target counts collapse, the prediction counts stay
    one = torch.full_like(tg, C - 1)
    red1, cnt1 = ops.ce_acc(lg.to(dev), one.to(dev), wd, counts=True)
    ck.exact("ce_acc.one_class", torch.equal(cnt1[:, 1].cpu().long(), cnt64[:, 1]) and int(cnt1[C - 1, 0]) == n
             and int(cnt1[:, 0].sum()) == n and int(cnt1[C - 1, 2]) == int(cnt64[C - 1, 1]) == int(red1[2])
             and int(cnt1[:, 2].sum()) == int(cnt64[C - 1, 1]))
    ck.done()


@gpu
@pytest.mark.parametrize("C", [2, 5, 16])
def test_ce_acc_ties_go_to_the_lowest_class(dev, C):
    """integer logits at identity size: ties are exact in every precision; the rule is spelt out, not taken from argmax"""
    B, H, W = 2, 37, 29
    gen = _gen(24, C)
    lg = torch.randint(-1, 2, (B, H, W, C), generator=gen).float()
    lg[0, 0] = 1.0                                       # a row where all classes tie
    tg = torch.randint(0, C, (B, H, W), generator=gen)
    best, pred = lg[..., 0].clone(), torch.zeros(B, H, W, dtype=torch.int64)
    for c in range(1, C):
        up = lg[..., c] > best                           # strictly greater: an equal later class does not take over
        pred[up], best[up] = c, lg[..., c][up]
    assert bool((pred[0, 0] == 0).all())
    want = torch.stack([torch.stack([(tg == c).sum(), (pred == c).sum(), ((tg == c) & (pred == c)).sum()]) for c in range(C)])
    red, cnt = ops.ce_acc(lg.to(dev), tg.to(dev), None, counts=True)
    ck = _Checks(("ties", B, H, W, C))
    ck.exact("ce_acc.ties.counts", torch.equal(cnt.cpu().long(), want))
    ck.exact("ce_acc.ties.correct", float(red[2]) == int((pred == tg).sum()) and float(red[1]) == B * H * W)
    ck.done()


# ---------------------------------------------------------------------------------------------------------------------------
# 6: reduce_rows
@gpu
@pytest.mark.parametrize("K", [1, 3, 8, 9, 2048])
@pytest.mark.parametrize("n", [1, 64, 65, 127, 128, 129, 160, 1000, 4096])
def test_reduce_rows(dev, n, K):
    """n <= 64 takes the wide kernel, above it the grouped one: 32 row groups, 4 x 32 rows a trip, then a tail of 32-row steps
    (n = 65: tail only; 129, 160: one trip and a tail; 128, 4096: no tail); K = 9: a second block with one live column"""
    _reduce_case(dev, n, K)


@gpu
def test_reduce_rows_many_columns_take_the_wide_kernel(dev):
    _reduce_case(dev, 65, 65536)


def _reduce_case(dev, n, K):
    gen = _gen(25, n, K)
    x = torch.rand(n, K, generator=gen) + 0.01
    scale = 0.37
    s32 = float(torch.tensor(scale, dtype=torch.float32))          # the kernel takes the scale as a float
    xd = x.to(dev)
    ck = _Checks((n, K))
    for name, sc, ref in (("reduce_rows", 1.0, x.double().sum(0)), ("reduce_rows.scaled", scale, x.double().sum(0) * s32)):
        got = ops.reduce_rows(xd, sc) if sc != 1.0 else ops.reduce_rows(xd)
        r32 = ref.float()                                        # the correctly rounded result; its spacing is the float32 ulp there
        half = 0.5 * (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()
        e = ((got.double().cpu() - ref).abs() / (half + n * 2.0 ** -52 * ref)).max()
        ck.add(name, float(e), 1.0)
    out = torch.full((K + 2,), 7.0, device=dev)
    ret = ops.reduce_rows(xd, scale, out=out[1:K + 1])
    ck.exact("reduce_rows.out", ret.data_ptr() == out[1:].data_ptr() and torch.equal(out[1:K + 1], ops.reduce_rows(xd, scale))
             and float(out[0]) == 7.0 and float(out[K + 1]) == 7.0)
    ck.done()
