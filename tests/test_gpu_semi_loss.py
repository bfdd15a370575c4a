"""csrc/semi.hip (the kernels of csrc/seg_loss_body.h instantiated with IgnoreLabel) through ``ops.seg_loss_ignore``, output by
output against tests/semi_ref.py in float64: ``sums``, ``loss`` and ``dz`` plane by plane, on the shapes and the named losses of
tests/test_gpu_loss_kernels.py and seven ignore patterns.

Bounds.  Those derived in the docstring of tests/test_gpu_loss_kernels.py (``_E``, ``_u_q``, U_s, U_c, U_b), none taken from what
the kernels give.  The order of accumulation is the parent kernels': the same per-thread chain over the same pixels (an ignored
pixel is skipped, so a chain only gets shorter), the same wave tree, the same four-way LDS step, the same double sums in the
finalize kernel; the accumulation term of U_s (6) is therefore the parent's.  What changes is which pixels count: rho (5 sigma of
the independent per-pixel roundings), rho_w of the CE term, D and A are taken over the VALID pixels by the reference.  With one
valid pixel rho = 1 and the bound is the per-pixel worst case.  The means run over the P*C pairs of the present samples in the
reference and in the kernel alike (one double division), so U_c and the loss bound keep their form.  ``coef`` is not an output of
the op: it is checked through dz, whose U_b carries U_c, and through the exact grad_scale check.

Exact: ``valid`` and St equal the counts; dz has all bits zero on every ignored pixel; with every pixel ignored loss == 0 and
dz == 0; two calls give the same bits; grad_scale 1024 against 1 scales dz exactly and leaves loss and sums; with sample 0 wholly
ignored, NaN logits in sample 0 change no bit of any output.

The pattern zero_w (only class-1 pixels valid, class 1 has CE weight 0: sum v w = 0) runs with ``ce_weighted`` on the shapes with
C > 1; b1c1 has no class 1.  Every check prints a MEASURE line before the test asserts (run with ``-s``).

Measured on one MI355X, the case with the largest err / bound per output:

    output          worst case                               err        Y (float32)  bound      err / bound
    semi.dz         (down_up, ce, onepix)                    1.401e-03  1.340e-03    5.360e-03  0.261
    semi.loss       (down_up, ce_dc, onepix)                 7.290e-06  7.528e-06    3.011e-05  0.242
    semi.sums.I     (down_up, ce, onepix)                    4.207e-06  4.268e-06    1.707e-05  0.246
    semi.sums.Sp    (down_up, ce_weighted, zero_w)           7.668e-07  6.393e-07    2.557e-06  0.300

(Where err is about Y the error is the float32 source coordinate's, which the kernel and torch share: with one valid pixel
nothing averages it out.)  All 2364 bit-exact checks hold; the 307 tests of the file take 3.3 s of pytest time on the GPU machine."""
import functools
import re

import pytest
import torch

from adaptersis_amd import _lib, ops
from tests import semi_ref as R
from tests.bound_helpers import ULP32, _gen
from tests.test_gpu_loss_kernels import GS, LOSS_NBLK, LOSS_SHAPES, LOSSES, _Checks, _E, _loss_inputs, _u_q

gpu = pytest.mark.gpu
SHAPES = ("nblk1", "nblk2", "down_up", "bc256_16x16", "b1c1", "missing")
PATTERNS = ("none", "rand30", "sample0", "all", "onepix", "oneclass")
IGNORE = {"rand30": -1, "oneclass": 1 << 20}       # the ignore value of a pattern; 255 elsewhere
CASES = [(s, n, p) for s in SHAPES for n in LOSSES for p in PATTERNS] \
    + [(s, "ce_weighted", "zero_w") for s in SHAPES if LOSS_SHAPES[s][1] > 1] \
    + [("cap512", n, p) for n in ("dice", "ce_dc") for p in PATTERNS]


@functools.lru_cache(maxsize=8)
def _target(shape, pattern):
    lg, tg, _ = _loss_inputs(*LOSS_SHAPES[shape])
    g = IGNORE.get(pattern, 255)
    return R.ignore_pattern(tg, pattern, g, _gen(31, len(shape), PATTERNS.index(pattern) if pattern in PATTERNS else 9, tg.numel())), g


def _same(a, b) -> bool:
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


@gpu
@pytest.mark.parametrize("shape,name,pattern", CASES)
def test_seg_loss_ignore(dev, shape, name, pattern):
    B, C, h, w, H, W, _ = LOSS_SHAPES[shape]
    assert _lib.lib().asis_dice_nblk(H, W) == LOSS_NBLK[shape]
    n_region, mode, eps, n_ce, weighted = LOSSES[name]
    lg, _, wts = _loss_inputs(*LOSS_SHAPES[shape])
    tg, g = _target(shape, pattern)
    wts = wts if weighted else None
    r64 = R.semi_ref(lg, tg, g, n_region, mode, eps, n_ce, wts, torch.float64, GS)
    r32 = R.semi_ref(lg, tg, g, n_region, mode, eps, n_ce, wts, torch.float32, GS)
    D, A = r64["D"], r64["A"]
    u_s = r64["kappa"] * (4 * n_region + 5 * r64["rho"] * _u_q(n_region, D, C) + 4 + 6)
    u_c = 13.0 if mode == 4 else (7 if mode == 1 else 3) * u_s + 2
    u_ce = 0.0 if n_ce == 0 else 2 + 5 * r64["rho_ce"] * (C + 3 + 2 * (A if n_ce == 1 else 1.0) + (2 * _E(D, C) if n_ce == 2 else 0.0))
    u_b = (0.0 if mode == 4 else u_c) + (13 if n_ce else 0) + 3 * _u_q(max(n_region, n_ce), D, C) + C + 4
    ck = _Checks((shape, name, pattern))
    lgd, tgd, wd = lg.to(dev), tg.to(dev), None if wts is None else wts.to(dev)
    out = loss, dz, valid, sums = ops.seg_loss_ignore(lgd, tgd, g, n_region, mode, eps, n_ce, wd, GS)
    v = tg != g
    # --- exact
    ck.exact("semi.shapes", tuple(loss.shape) == (1,) and tuple(dz.shape) == (B, H, W, C) and tuple(sums.shape) == (B, C, 3)
             and valid.dtype == torch.int32 and tuple(valid.shape) == (B,) and dz.dtype == torch.float32)
    ck.exact("semi.valid", torch.equal(valid.cpu().long(), v.sum((1, 2))))
    cnt = torch.stack([torch.bincount(tg[b][v[b]].reshape(-1), minlength=C)[:C] for b in range(B)])
    ck.exact("semi.St", torch.equal(sums[..., 2].cpu().long(), cnt))
    ck.exact("semi.dz.ignored_bits", not bool(dz.cpu().view(torch.int32)[~v].any()))
    ck.exact("semi.finite", bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dz).all()) and bool(torch.isfinite(sums).all()))
    if not bool(v.any()):
        ck.exact("semi.all_ignored", not bool(loss.view(torch.int32).any()) and not bool(dz.view(torch.int32).any())
                 and not bool(sums.view(torch.int32).any()))
    if pattern == "zero_w":
        ck.exact("semi.zero_weight_sum", float(loss) == 0.0 and float(dz.abs().max()) == 0.0)
    ck.exact("semi.again", _same(out, ops.seg_loss_ignore(lgd, tgd, g, n_region, mode, eps, n_ce, wd, GS)))
    one = ops.seg_loss_ignore(lgd, tgd, g, n_region, mode, eps, n_ce, wd, 1.0)
    ck.exact("semi.grad_scale", torch.equal(dz, one[1] * GS) and _same((loss, valid, sums), (one[0], one[2], one[3])))
    if not bool(v[0].any()):      # the logits of a sample without labels are never read
        nan = lgd.clone()
        nan[0] = float("nan")
        ck.exact("semi.nan_logits_unread", _same(out, ops.seg_loss_ignore(nan, tgd, g, n_region, mode, eps, n_ce, wd, GS)))
    # --- against float64
    for k, nm in ((0, "I"), (1, "Sp")):
        ck.relative(f"semi.sums.{nm}", sums[..., k], r64["sums"][..., k], r32["sums"][..., k], u_s)
    floor = ULP32 * (4 * u_s * r64["term"] + u_ce + 6 * r64["ce"] + abs(float(r64["loss"])))
    ck.absolute("semi.loss", loss.reshape(()), r64["loss"], r32["loss"], 0, floor)
    got, ref, f32 = dz.double().cpu(), r64["dz"], r32["dz"].double()
    err_p, y_p, top_p = (got - ref).abs().amax((1, 2)), (f32 - ref).abs().amax((1, 2)), ref.abs().amax((1, 2))
    lim_p = torch.maximum(4 * y_p, u_b * ULP32 * top_p)
    ratio = torch.where(lim_p > 0, err_p / lim_p.clamp_min(1e-300), torch.where(err_p == 0, 0.0, float("inf")).double())
    b, c = divmod(int(ratio.argmax()), C)
    print(f"MEASURE semi.dz {(shape, name, pattern)}: worst plane b {b} c {c} err {float(err_p[b, c]):.3e} yard {float(y_p[b, c]):.3e} "
          f"bound {float(lim_p[b, c]):.3e} ratio {float(ratio.max()):.3f}  (plane maxima {float(top_p.min()):.2e} .. {float(top_p.max()):.2e})")
    if not float(ratio.max()) <= 1.0:
        ck.fails.append(("semi.dz", b, c, float(err_p[b, c]), float(lim_p[b, c])))
    ck.done()


@gpu
def test_nothing_ignored_is_the_parent_loss_bit_for_bit(dev):
    """with no ignored pixel the op gives the bits of ``seg_loss_fwd`` + ``seg_loss_bwd``: same statements, same order of sums"""
    ck = _Checks("parent_bits")
    for shape in ("nblk2", "missing"):
        lg, tg, wts = _loss_inputs(*LOSS_SHAPES[shape])
        for name, (n_region, mode, eps, n_ce, weighted) in LOSSES.items():
            lgd, tgd, wd = lg.to(dev), tg.to(dev), wts.to(dev) if weighted else None
            loss, coef, sums = ops.seg_loss_fwd(lgd, tgd, n_region, mode, eps, n_ce, wd, GS)
            dz = ops.seg_loss_bwd(lgd, tgd, coef, n_region, mode, n_ce, wd)
            l2, dz2, valid, s2 = ops.seg_loss_ignore(lgd, tgd, 255, n_region, mode, eps, n_ce, wd, GS)
            ck.exact(f"semi.parent_bits.{shape}.{name}", _same((loss, dz, sums), (l2, dz2, s2)) and bool((valid == tg[0].numel()).all()))
    ck.done()


@gpu
def test_seg_loss_ignore_refusals(dev):
    lg, tg = torch.zeros(2, 4, 4, 3, device=dev), torch.zeros(2, 8, 8, dtype=torch.int64, device=dev)
    big = lambda B, C: (torch.zeros(B, 2, 2, C, device=dev), torch.zeros(B, 4, 4, dtype=torch.int64, device=dev))   # noqa: E731
    cases = [("ignore 0", "ignore_index", lambda: ops.seg_loss_ignore(lg, tg, 0, 1)),
             ("ignore C-1", "ignore_index", lambda: ops.seg_loss_ignore(lg, tg, 2, 1)),
             ("ignore float", "ignore_index", lambda: ops.seg_loss_ignore(lg, tg, 255.0, 1)),
             ("int32 target", "contiguous int64", lambda: ops.seg_loss_ignore(lg, tg.int(), 255, 1)),
             ("strided target", "contiguous int64",
              lambda: ops.seg_loss_ignore(lg, torch.zeros(2, 8, 16, dtype=torch.int64, device=dev)[:, :, ::2], 255, 1)),
             ("C 17", "C=", lambda: ops.seg_loss_ignore(*big(1, 17), 255, 1)),
             ("B*C 257 x 1", "B\\*C", lambda: ops.seg_loss_ignore(*big(257, 1), 255, 1)),
             ("mode 4 without CE", "needs a CE term", lambda: ops.seg_loss_ignore(lg, tg, 255, 1, ops.LOSS_NONE, 1.0, 0))]
    ck = _Checks("refusals")
    for name, pattern, call in cases:
        try:
            call()
            said = None
        except ValueError as e:
            said = str(e)
        ck.exact(f"semi.refuses.{name.replace(' ', '_')}", said is not None and re.search(pattern, said) is not None)
    torch.cuda.synchronize()
    ck.done()
