"""The commuted stage-4 tail + classifier (csrc/clslowres.hip, ops.cls_lowres_fwd / ops.cls_lowres_bwd, ops.CLS_LOWRES) against
torch on the CPU in float64:

    F.interpolate(relu(raw * scale + shift), scale_factor=2, mode="bilinear", align_corners=True) -> conv2d(padding=1)

and its autograd.  Compared: the logits, g (the gradient at the BatchNorm output of stage 4), the reduced sums of g and of
g * xhat, and dW.  The reference sees the very values the kernels see: raw, scale, shift, mean, invstd and w in fp32, and for the
gradient the 16-bit planes d16 (+ d_lo) decoded to float64.  Every pre-activation has |raw * scale + shift| >= 1e-3 (asserted on the
CPU where the inputs are made), so the float64 and the fp32 ReLU masks cannot differ.

Bound, per compared quantity: the rel-L2 error of the PRESENT path on the same inputs against the same reference
(bn_relu_upsample -> conv3x3_smallcout_fwd, conv3x3_smallcout_dgrad -> upsample_bn_relu_bwd, wgrad), measured in the same test; the
new path may have at most twice that error.  The factor 2 is for reordered fp32 sums of equal length where both paths sit at the
fp32 floor; nothing else differs in the new path's disfavour (it works on fp32 values where the present path rounds the operand
to a 16-bit hi + lo pair, and for dW to the 16-bit hi alone).  Every check prints a MEASURE line before it asserts (run with -s).

Measured on one MI355X (maxima over all kernel-level and border cases, rel-L2 new | present, and the largest new / present):

    quantity   f16 operands          bf16 operands         worst ratio
    logits     3.2e-7 | 6.5e-7       3.2e-7 | 5.8e-6       0.71   (1x9x6, 2 classes, f16)
    g          4.2e-7 | 6.0e-7       4.2e-7 | 4.0e-6       1.23   (edge pixel (0, 0, 5))
    sum g      2.7e-7 | 5.3e-7       2.6e-7 | 5.1e-6       1.26   (edge pixel (0, 0, 5))
    sum g xhat 4.3e-7 | 5.9e-7       3.8e-7 | 4.7e-6       1.29   (edge pixel (0, 0, 5))
    dW         3.1e-7 | 4.0e-4       3.1e-7 | 3.6e-3       < 0.01

Module level: a parameter whose exact gradient is zero (the bias of a conv in front of a train-mode BatchNorm) has no relative
error; there the gradient must be finite, and the ratio is taken on every other parameter (as tests/test_gpu_modules.py does).
"""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

from adaptersis_amd import _lib, config, ops, parallel
from tests.conftest import rel_l2

gpu = pytest.mark.gpu
DTS = {"f16": torch.float16, "bf16": torch.bfloat16}
SHAPES = [(1, 4, 8), (2, 5, 7), (1, 9, 6), (2, 33, 40)]
CIN = 64


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _split16(d: torch.Tensor, dt: torch.dtype, with_lo: bool):
    """fp32 [B, h, w, C] -> (d16, d_lo | None) padded to 8 channels, and the float64 value the pair encodes"""
    B, h, w, C = d.shape
    hi = torch.zeros((B, h, w, 8), dtype=dt)
    hi[..., :C] = d.to(dt)
    lo = None
    val = hi[..., :C].double()
    if with_lo:
        lo = torch.zeros((B, h, w, 8), dtype=dt)
        lo[..., :C] = (d - hi[..., :C].float()).to(dt)
        val = val + lo[..., :C].double()
    return hi, lo, val


@functools.lru_cache(maxsize=None)
def _inputs(B: int, H: int, W: int, C: int):
    """CPU fp32 inputs of one shape (shared by every dtype / d_lo case), conditioned so that no pre-activation is near zero"""
    g = _gen(1000 * B + 100 * H + 10 * W + C)
    raw = torch.randn((B, H, W, CIN), generator=g)
    scale = (0.5 + torch.rand(CIN, generator=g)) * torch.where(torch.rand(CIN, generator=g) < 0.25, -1.0, 1.0)
    shift = 0.3 * torch.randn(CIN, generator=g)
    pre = raw * scale + shift
    raw = torch.where(pre.abs() < 4e-3, (torch.copysign(torch.full_like(pre, 8e-3), pre) - shift) / scale, raw).contiguous()
    assert float((raw.double() * scale.double() + shift.double()).abs().min()) >= 1e-3
    assert float((raw * scale + shift).abs().min()) >= 1e-3
    mean = 0.2 * torch.randn(CIN, generator=g)
    invstd = 0.5 + torch.rand(CIN, generator=g)
    w = torch.randn((C, CIN, 3, 3), generator=g) / 24.0
    bias = 0.1 * torch.randn(C, generator=g)
    d = torch.randn((B, 2 * H, 2 * W, C), generator=g) * 64.0     # a loss-scaled gradient
    return raw, scale, shift, mean, invstd, w, bias, d


def _reference(raw, scale, shift, mean, invstd, w, bias, dval):
    """float64 torch: logits NHWC, g NHWC, sum g, sum g * xhat, dW"""
    x = raw.double().permute(0, 3, 1, 2)
    pre = (x * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]).requires_grad_()
    wq = w.double().requires_grad_()
    y = F.conv2d(F.interpolate(F.relu(pre), scale_factor=2, mode="bilinear", align_corners=True), wq, bias.double(), padding=1)
    y.backward(dval.permute(0, 3, 1, 2))
    g = pre.grad.permute(0, 2, 3, 1).contiguous()
    xhat = (raw.double() - mean.double()) * invstd.double()
    return dict(logits=y.detach().permute(0, 2, 3, 1).contiguous(), g=g, sum_g=g.sum((0, 1, 2)), sum_gx=(g * xhat).sum((0, 1, 2)),
                dW=wq.grad)


def _new_path(dev, raw, scale, shift, mean, invstd, w, bias, d16, d_lo):
    t = lambda v: None if v is None else v.to(dev)
    logits = ops.cls_lowres_fwd(t(raw), t(scale), t(shift), t(w), t(bias))
    g, partial, dW = ops.cls_lowres_bwd(t(d16), t(d_lo), t(raw), t(scale), t(shift), t(mean), t(invstd), t(w))
    red = ops.reduce_rows(partial.view(partial.shape[0], 2 * CIN))
    assert partial.shape[0] == _lib.lib().asis_cls_lowres_nblk(*raw.shape[:3])
    return dict(logits=logits, g=g, sum_g=red[:CIN], sum_gx=red[CIN:], dW=dW), partial


def _present_path(dev, raw, scale, shift, mean, invstd, w, bias, d16, d_lo):
    t = lambda v: None if v is None else v.to(dev)
    C = w.shape[0]
    hi, lo = ops.bn_relu_upsample(t(raw), t(scale), t(shift), 2, d16.dtype, True)
    logits = ops.conv3x3_smallcout_fwd(hi, lo, t(w), t(bias))
    dU = ops.conv3x3_smallcout_dgrad(t(d16), t(d_lo), t(w))
    g, partial = ops.upsample_bn_relu_bwd(dU, t(raw), t(scale), t(shift), t(mean), t(invstd), 2)
    red = ops.reduce_rows(partial.view(partial.shape[0], 2 * CIN))
    dW = ops.wgrad(t(d16), hi, C, 3, 3, 1, 1, 1.0)
    return dict(logits=logits, g=g, sum_g=red[:CIN], sum_gx=red[CIN:], dW=dW)


def _compare(tag: str, new: dict, old: dict, ref: dict):
    bad = []
    for k in ("logits", "g", "sum_g", "sum_gx", "dW"):
        e_new, e_old = rel_l2(new[k], ref[k]), rel_l2(old[k], ref[k])
        print(f"MEASURE cls_lowres {tag} {k}: new {e_new:.3e} present {e_old:.3e} ratio {e_new / max(e_old, 1e-30):.2f}")
        if not e_new <= 2.0 * e_old:
            bad.append((k, e_new, e_old))
    assert not bad, (tag, bad)


@gpu
@pytest.mark.parametrize("with_lo", [True, False], ids=["lo", "nolo"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_against_float64(dev, shape, C, dt, with_lo):
    B, H, W = shape
    raw, scale, shift, mean, invstd, w, bias, d = _inputs(B, H, W, C)
    assert ops.cls_lowres_ok(raw.to(dev), C)
    d16, d_lo, dval = _split16(d, DTS[dt], with_lo)
    ref = _reference(raw, scale, shift, mean, invstd, w, bias, dval)
    new, _ = _new_path(dev, raw, scale, shift, mean, invstd, w, bias, d16, d_lo)
    old = _present_path(dev, raw, scale, shift, mean, invstd, w, bias, d16, d_lo)
    _compare(f"{B}x{H}x{W} C{C} {dt} {'lo' if with_lo else 'nolo'}", new, old, ref)


def _window(y: int, x: int, H: int, W: int):
    """low-resolution rows / columns that a gradient at output pixel (y, x) can reach: the bilinear sources of the <= 3 x 3 conv taps"""
    def span(o, n):
        lo, hi = n, -1
        for p in range(max(o - 1, 0), min(o + 1, 2 * n - 1) + 1):
            s = p * (n - 1) / (2 * n - 1)
            i0 = int(s)
            lo, hi = min(lo, i0), max(hi, min(i0 + 1, n - 1))
        return lo, hi
    return span(y, H), span(x, W)


@gpu
@pytest.mark.parametrize("where", ["corner", "edge"])
def test_borders(dev, where):
    """d non-zero at one corner pixel, then at one edge pixel: g is exactly zero outside the reachable window and matches inside"""
    B, H, W, C = 2, 5, 7, 2
    raw, scale, shift, mean, invstd, w, bias, d = _inputs(B, H, W, C)
    pts = {"corner": [(0, 0, 0), (1, 2 * H - 1, 2 * W - 1)], "edge": [(0, 0, 5), (1, 6, 2 * W - 1)]}[where]
    for b, y, x in pts:
        one = torch.zeros_like(d)
        one[b, y, x] = d[b, y, x]
        d16, d_lo, dval = _split16(one, torch.float16, True)
        ref = _reference(raw, scale, shift, mean, invstd, w, bias, dval)
        new, _ = _new_path(dev, raw, scale, shift, mean, invstd, w, bias, d16, d_lo)
        old = _present_path(dev, raw, scale, shift, mean, invstd, w, bias, d16, d_lo)
        (r0, r1), (c0, c1) = _window(y, x, H, W)
        inside = torch.zeros((B, H, W), dtype=torch.bool)
        inside[b, r0:r1 + 1, c0:c1 + 1] = True
        g = new["g"].cpu()
        assert float(ref["g"][~inside].abs().max()) == 0.0          # the window is the reference's too
        assert float(ref["g"][inside].abs().max()) > 0.0
        assert float(g[~inside].abs().max()) == 0.0, (where, b, y, x)
        _compare(f"border {where} ({b},{y},{x})", new, old, ref)


@gpu
def test_bit_identical_between_calls(dev):
    B, H, W, C = 2, 33, 40, 3
    raw, scale, shift, mean, invstd, w, bias, d = _inputs(B, H, W, C)
    d16, d_lo, _ = _split16(d, torch.bfloat16, True)
    a, pa = _new_path(dev, raw, scale, shift, mean, invstd, w, bias, d16, d_lo)
    b, pb = _new_path(dev, raw, scale, shift, mean, invstd, w, bias, d16, d_lo)
    assert torch.equal(pa, pb)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _module_run(dev, m, x, dl):
    hi, lo = m._to_nhwc16(x)
    logits, saved = m._forward_core(hi, lo, save=True)
    B, h, w, C = logits.shape
    S = config.loss_scale
    d = dl.to(dev).permute(0, 2, 3, 1).contiguous().float().view(B * h * w, C)
    CP = (C + 7) // 8 * 8
    d16 = ops.cast_pad(d, CP, config.operand_dtype, scale=S).view(B, h, w, CP)
    d_lo = ops.cast_pad(d, CP, config.operand_dtype, scale=S, part=1).view(B, h, w, CP) if config.split_conv else None
    grads = {n: torch.empty_like(p) for n, p in m.named_parameters()}
    m._backward_core(saved, d16, None, 1.0 / S, grads, dlogits_f32=d, d_lo=d_lo)
    parallel.join_grad_streams()
    torch.cuda.synchronize()
    return logits.permute(0, 3, 1, 2), grads, saved


@gpu
def test_feature_decoder_switch_on_and_off(dev):
    """a small FeatureDecoder through _forward_core / _backward_core with ops.CLS_LOWRES on and off, against the float64 autograd of
    the same nn.Module on the CPU: logits and every parameter gradient, the new path at most twice the present path's error"""
    from adaptersis_amd.backbones.decoders import FeatureDecoder
    torch.manual_seed(7)
    m = FeatureDecoder(embed_dim=64, num_classes=2, features=[64, 64, 64, 64, 64])
    for i in range(1, 5):       # BatchNorm affines away from the identity
        bn = getattr(m, f"decoder_{i}")[1]
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
    m.train()
    x = torch.randn(1, 192, 3, 4)
    dl = torch.randn(1, 2, 48, 64) / 64.0
    ref = copy.deepcopy(m).double()
    y = x.double()
    for i in range(1, 5):
        y = getattr(ref, f"decoder_{i}")(y)
    y = ref.final_out(y)
    y.backward(dl.double())
    rgrads = {n: p.grad for n, p in ref.named_parameters()}
    res = {}
    old = ops.CLS_LOWRES
    try:
        for on in (False, True):
            ops.CLS_LOWRES = on
            mm = copy.deepcopy(m).to(dev).train()
            logits, grads, saved = _module_run(dev, mm, x.to(dev), dl)
            assert (saved[4] is None) == on and bool(getattr(saved[3], "cls_lowres", False)) == on
            res[on] = (logits, grads)
    finally:
        ops.CLS_LOWRES = old
    bad = []
    e_new, e_old = rel_l2(res[True][0], y), rel_l2(res[False][0], y)
    print(f"MEASURE cls_lowres module logits: new {e_new:.3e} present {e_old:.3e}")
    if not e_new <= 2.0 * e_old:
        bad.append(("logits", e_new, e_old))
    wmax = max(float(v.abs().max()) for v in rgrads.values())
    for n, r in rgrads.items():
        assert bool(torch.isfinite(res[True][1][n]).all()), n
        if float(r.abs().max()) < 1e-9 * wmax:      # exactly zero but for rounding: no relative error to compare
            continue
        e_new, e_old = rel_l2(res[True][1][n], r), rel_l2(res[False][1][n], r)
        print(f"MEASURE cls_lowres module {n}: new {e_new:.3e} present {e_old:.3e}")
        if not e_new <= 2.0 * e_old:
            bad.append((n, e_new, e_old))
    assert not bad, bad
