"""The decoder input gradient commuted with the transposed x2 upsampling (csrc/dgradlowres.hip, ops.dgrad_lowres, ops.DGRAD_LOWRES)
against torch on the CPU in float64:

    pre = raw * scale + shift                      (a leaf)
    y = conv2d(F.interpolate(relu(pre), scale_factor=2, mode="bilinear", align_corners=True), w, padding=1)
    y.backward(dval);  g = pre.grad

Compared: g (the gradient at the BatchNorm output of the lower stage) and the reduced sums of g and of g * xhat.  The reference sees
the very values the kernel sees: raw, scale, shift, mean, invstd and w in fp32, and for the gradient the 16-bit planes d16 (+ d_lo)
decoded to float64.  Every pre-activation has |raw * scale + shift| >= 1e-3 (asserted on the CPU where the inputs are made), so the
float64 and the fp32 ReLU masks cannot differ.

Bound, per compared quantity: the rel-L2 error of the PRESENT path on the same inputs against the same reference, measured in the same
test — the input-gradient convolution in the form the step uses for that dtype (16-bit + one MX pass where ops.mx_conv_ok takes the
shape, else three 16-bit parts; one 16-bit part without d_lo), then ops.upsample_bn_relu_bwd.  The new path may have at most twice
that error.  The factor 2 is for reordered fp32 sums where both paths sit at the fp32 floor; nothing else differs in the new path's
disfavour.  Every check prints a MEASURE line before it asserts (run with -s).

Measured on one MI355X (maxima over the six kernel-level cases and the eight one-hot cases, rel-L2 new | present, and the largest
new / present; "present" with d_lo is the MX form for f16 where ops.mx_conv_ok takes the shape (2x5x7, 2x17x19), three 16-bit parts
otherwise; without d_lo it is one 16-bit part, whose weight rounding the new path does not share):

    quantity     f16, d_lo          bf16, d_lo         f16, no d_lo       bf16, no d_lo      worst new / present
    g            7.4e-7 | 1.1e-5    4.5e-6 | 3.8e-6    7.4e-7 | 2.3e-4    4.5e-6 | 1.7e-3    1.21   (1x2x2, bf16, d_lo)
    sum g        6.0e-7 | 1.1e-5    4.2e-6 | 4.0e-6    6.3e-7 | 2.6e-4    4.1e-6 | 1.7e-3    1.22   (2x17x19, bf16, d_lo)
    sum g xhat   7.1e-7 | 1.1e-5    4.5e-6 | 4.3e-6    7.1e-7 | 2.5e-4    4.5e-6 | 1.8e-3    1.19   (1x2x2, f16, d_lo)
    one-hot (f16, d_lo): g 7.4e-7 | 1.2e-5, sum g 5.8e-7 | 1.2e-5, sum g xhat 7.0e-7 | 1.3e-5; worst ratio 0.08
    several tiles per workgroup (2x17x19, f16, d_lo; 4 workgroups x 3 tiles and 1 x 12): g bit-identical to the 12 x 1 launch;
    sum g 5.8e-7 | 1.0e-5, sum g xhat 7.1e-7 | 1.1e-5
    (bf16 with d_lo: both paths round the weights to hi + lo = 16 bits; the new one rounds e to 16 bits as well, the present one
    takes d as stored: about sqrt(2) in the error is expected, 1.2 measured.)
    module (FeatureDecoder 192 -> 512 -> 256 -> 128 -> 64 -> 2, [2, 192, 4, 4], f16): every parameter gradient within 0.1 % of the
    present path's error (conv weights 2.1-2.3e-3, BatchNorm affines 0.8-3.1e-3: the 16-bit stages in front, common to both)

Module level: a parameter whose exact gradient is zero (the bias of a conv in front of a train-mode BatchNorm) has no relative
error; there the gradient must be finite, and the ratio is taken on every other parameter (as tests/test_gpu_cls_lowres.py does).
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
# (B, H, W, Co, Ck): the minimum size; odd sizes; a tile seam (tiles are 8 x 16) with a 1..3 pixel remainder in both directions; a
# second image; and the chunk / N-slice loops of the wider channel pairs
CASES = [(1, 2, 2, 64, 128), (2, 5, 7, 64, 128), (1, 9, 6, 64, 128), (2, 17, 19, 64, 128), (2, 5, 7, 128, 256), (2, 5, 7, 256, 512)]


def _split16(d: torch.Tensor, dt: torch.dtype, with_lo: bool):
    """fp32 [B, h, w, Co] -> (d16, d_lo | None) and the float64 value the pair encodes"""
    hi = d.to(dt)
    lo = None
    val = hi.double()
    if with_lo:
        lo = (d - hi.float()).to(dt)
        val = val + lo.double()
    return hi, lo, val


@functools.lru_cache(maxsize=None)
def _inputs(B: int, H: int, W: int, Co: int, Ck: int):
    """CPU fp32 inputs of one shape (shared by every dtype / d_lo case), conditioned so that no pre-activation is near zero"""
    g = torch.Generator().manual_seed(100000 * B + 1000 * H + 10 * W + Co + Ck)
    raw = torch.randn((B, H, W, Ck), generator=g)
    scale = (0.5 + torch.rand(Ck, generator=g)) * torch.where(torch.rand(Ck, generator=g) < 0.25, -1.0, 1.0)
    shift = 0.3 * torch.randn(Ck, generator=g)
    pre = raw * scale + shift
    raw = torch.where(pre.abs() < 4e-3, (torch.copysign(torch.full_like(pre, 8e-3), pre) - shift) / scale, raw).contiguous()
    assert float((raw.double() * scale.double() + shift.double()).abs().min()) >= 1e-3
    assert float((raw * scale + shift).abs().min()) >= 1e-3
    mean = 0.2 * torch.randn(Ck, generator=g)
    invstd = 0.5 + torch.rand(Ck, generator=g)
    w = torch.randn((Co, Ck, 3, 3), generator=g) / 24.0
    d = torch.randn((B, 2 * H, 2 * W, Co), generator=g) * 64.0     # a loss-scaled gradient
    return raw, scale, shift, mean, invstd, w, d


def _reference(raw, scale, shift, mean, invstd, w, dval):
    """float64 torch: g NHWC, sum g, sum g * xhat"""
    x = raw.double().permute(0, 3, 1, 2)
    pre = (x * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]).requires_grad_()
    y = F.conv2d(F.interpolate(F.relu(pre), scale_factor=2, mode="bilinear", align_corners=True), w.double(), padding=1)
    y.backward(dval.permute(0, 3, 1, 2))
    g = pre.grad.permute(0, 2, 3, 1).contiguous()
    xhat = (raw.double() - mean.double()) * invstd.double()
    return dict(g=g, sum_g=g.sum((0, 1, 2)), sum_gx=(g * xhat).sum((0, 1, 2)))


@functools.lru_cache(maxsize=None)
def _full_reference(case, dt: str, with_lo: bool):
    """the reference of one case with the full random gradient, computed once"""
    raw, scale, shift, mean, invstd, w, d = _inputs(*case)
    _, _, dval = _split16(d, DTS[dt], with_lo)
    return _reference(raw, scale, shift, mean, invstd, w, dval)


def _pack_out(g, partial):
    Ck = g.shape[3]
    red = ops.reduce_rows(partial.view(partial.shape[0], 2 * Ck))
    return dict(g=g, sum_g=red[:Ck], sum_gx=red[Ck:])


def _new_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo):
    t = lambda v: None if v is None else v.to(dev)
    wp = ops.dgrad_lowres_pack(t(w), d16.dtype)
    g, partial = ops.dgrad_lowres(t(d16), t(d_lo), wp, t(raw), t(scale), t(shift), t(mean), t(invstd))
    assert partial.shape[0] == _lib.lib().asis_dgrad_lowres_nblk(*raw.shape[:3])
    return _pack_out(g, partial), partial


def _present_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo):
    """decoders._dgrad on the same planes, then the transposed upsampling"""
    t = lambda v: None if v is None else v.to(dev)
    dt = d16.dtype
    B, h, wd_, Co = d16.shape
    Ck = w.shape[1]
    if d_lo is None:
        dU = ops.conv_gemm(t(d16), ops.pack_conv_weight(t(w), 1, dt), 3, 3, 1, 1)
    elif config.mx_conv and (config.mx_conv_all or dt == torch.float16) and ops.mx_conv_ok(B * h * wd_, Co, Ck):
        hi, lo = t(d16), t(d_lo)
        mxp, amax = ops.mx_from_pair(hi.view(-1, Co), lo.view(-1, Co))
        wdh, wdm, wamax = ops.pack_conv_weight_pair(t(w), 1, dt, mx=True)
        dU = ops.conv_gemm_split(hi, ops.MxPlane.tag(mxp.view(hi.shape), amax), wdh, wdm, 3, 3, 1, 1, mx=(amax, wamax))
    else:
        wdh, wdl, _ = ops.pack_conv_weight_pair(t(w), 1, dt)
        dU = ops.conv_gemm_split(t(d16), t(d_lo), wdh, wdl, 3, 3, 1, 1)
    g, partial = ops.upsample_bn_relu_bwd(dU, t(raw), t(scale), t(shift), t(mean), t(invstd), 2)
    return _pack_out(g, partial)


def _compare(tag: str, new: dict, old: dict, ref: dict):
    bad = []
    for k in ("g", "sum_g", "sum_gx"):
        e_new, e_old = rel_l2(new[k], ref[k]), rel_l2(old[k], ref[k])
        print(f"MEASURE dgrad_lowres {tag} {k}: new {e_new:.3e} present {e_old:.3e} ratio {e_new / max(e_old, 1e-30):.2f}")
        if not e_new <= 2.0 * e_old:
            bad.append((k, e_new, e_old))
    assert not bad, (tag, bad)


@gpu
@pytest.mark.parametrize("with_lo", [True, False], ids=["lo", "nolo"])
@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_kernel_against_float64(dev, case, dt, with_lo):
    raw, scale, shift, mean, invstd, w, d = _inputs(*case)
    assert ops.dgrad_lowres_ok(case[3], case[4], case[1], case[2])
    d16, d_lo, _ = _split16(d, DTS[dt], with_lo)
    ref = _full_reference(case, dt, with_lo)
    new, _ = _new_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo)
    old = _present_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo)
    _compare(f"{'x'.join(map(str, case))} {dt} {'lo' if with_lo else 'nolo'}", new, old, ref)


# one-hot gradients on the (2, 17, 19) map, hi-res 34 x 38: (image, row, column).  Tile seams of the 8 x 16 low-resolution tiles lie
# between hi-res rows 15 | 16 and columns 31 | 32.
ONE_HOT = {
    "corner_tl": (0, 0, 0), "corner_tr": (0, 0, 37), "corner_bl": (0, 33, 0), "corner_br": (0, 33, 37),   # br = last pixel of image 0
    "border_mid": (0, 0, 19), "seam_before": (0, 15, 31), "seam_after": (0, 16, 32), "image1_first": (1, 0, 0),
}


@gpu
@pytest.mark.parametrize("where", sorted(ONE_HOT))
def test_one_hot(dev, where):
    """d non-zero at one hi-res pixel: g is exactly zero wherever the reference is (outside the reachable window, the other image,
    masked channels) and meets the bound elsewhere"""
    case = (2, 17, 19, 64, 128)
    raw, scale, shift, mean, invstd, w, d = _inputs(*case)
    b, y, x = ONE_HOT[where]
    one = torch.zeros_like(d)
    one[b, y, x] = d[b, y, x]
    d16, d_lo, dval = _split16(one, torch.float16, True)
    ref = _reference(raw, scale, shift, mean, invstd, w, dval)
    new, _ = _new_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo)
    old = _present_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo)
    g = new["g"].cpu()
    zero = ref["g"] == 0
    off = (raw * scale + shift) <= 0
    assert bool(zero[1 - b].all()) and bool((~zero[b]).any())        # the other image gets nothing, this one something
    assert float(g[zero].abs().max()) == 0.0, where
    assert float(g[off].abs().max()) == 0.0, where
    _compare(f"one-hot {where} ({b},{y},{x})", new, old, ref)


@gpu
def test_bit_identical_between_calls(dev):
    case = (2, 17, 19, 64, 128)
    raw, scale, shift, mean, invstd, w, d = _inputs(*case)
    d16, d_lo, _ = _split16(d, torch.bfloat16, True)
    a, pa = _new_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo)
    b, pb = _new_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo)
    assert torch.equal(pa, pb)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@gpu
@pytest.mark.parametrize("cap", [1, 5])
def test_several_tiles_per_workgroup(dev, cap):
    """the grid-stride tile loop of the large maps (more than 2048 tiles) on the 12 tiles of the (2, 17, 19) map: with the workgroup cap
    at 5 four workgroups walk three tiles each (two images, seams and remainders inside one run), at 1 one workgroup walks all twelve.
    g must have the bits of the one-tile-per-workgroup launch; the sums meet the bound against float64"""
    case = (2, 17, 19, 64, 128)
    raw, scale, shift, mean, invstd, w, d = _inputs(*case)
    d16, d_lo, _ = _split16(d, torch.float16, True)
    ref = _full_reference(case, "f16", True)
    lib = _lib.lib()
    base, pbase = _new_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo)
    assert pbase.shape[0] == 12
    old_cap = lib.asis_dgrad_lowres_cap(cap)
    try:
        assert old_cap == 2048 and lib.asis_dgrad_lowres_nblk(2, 17, 19) == {1: 1, 5: 4}[cap]
        new, partial = _new_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo)
        torch.cuda.synchronize()
    finally:
        lib.asis_dgrad_lowres_cap(old_cap)
    assert lib.asis_dgrad_lowres_nblk(2, 17, 19) == 12
    assert partial.shape[0] == {1: 1, 5: 4}[cap]
    assert torch.equal(new["g"], base["g"])
    old = _present_path(dev, raw, scale, shift, mean, invstd, w, d16, d_lo)
    _compare(f"2x17x19 f16 lo, cap {cap}", new, old, ref)


def test_switch_values():
    """ASIS_DGRAD_LOWRES: 0 / 1 / a list of stages; anything else is an error, not a silent 'off'"""
    assert config.parse_dgrad_lowres("1") == {"d2", "d3", "d4"} and config.parse_dgrad_lowres("0") == frozenset()
    assert config.parse_dgrad_lowres("d3, d4") == {"d3", "d4"}
    for bad in ("d5", "on", "true", "d2,d1"):
        with pytest.raises(ValueError):
            config.parse_dgrad_lowres(bad)
    assert _lib.lib().asis_dgrad_lowres_nblk(0, 4, 4) == 0 and _lib.lib().asis_dgrad_lowres_nblk(1, 4, 0) == 0


@gpu
@pytest.mark.parametrize("what", ["H1", "Co", "align", "nblk"])
def test_bad_arguments_are_refused_before_any_launch(dev, what):
    B, H, W, Co, Ck = 1, 2, 2, 64, 128
    raw, scale, shift, mean, invstd, w, d = _inputs(B, H, W, Co, Ck)
    t = lambda v: v.to(dev)
    d16 = torch.zeros((B, 2 * H, 2 * W, Co + 8), device=dev, dtype=torch.float16)   # room for the shifted pointer
    wp = ops.dgrad_lowres_pack(t(w), torch.float16)
    rawg, sc, sh, mu, isd = t(raw), t(scale), t(shift), t(mean), t(invstd)
    g = torch.full_like(rawg, 7.0)
    lib = _lib.lib()
    nblk = lib.asis_dgrad_lowres_nblk(B, H, W)
    partial = torch.full((nblk + 1, 2, Ck), 7.0, device=dev)
    a = dict(d=d16.data_ptr(), nblk=nblk, H=H, Co=Co)
    if what == "H1":
        a["H"] = 1
    elif what == "Co":
        a["Co"] = 24
    elif what == "align":
        a["d"] += 2
    else:
        a["nblk"] = nblk + 1
    rc = lib.asis_dgrad_lowres(ops._stream(), _lib.ASIS_F16, a["d"], None, wp[0].data_ptr(), wp[1].data_ptr(), rawg.data_ptr(),
                               sc.data_ptr(), sh.data_ptr(), mu.data_ptr(), isd.data_ptr(), g.data_ptr(), partial.data_ptr(), a["nblk"],
                               B, a["H"], W, a["Co"], Ck)
    assert rc == -1
    with pytest.raises(ValueError):
        _lib.check(rc, "asis_dgrad_lowres")
    torch.cuda.synchronize()
    assert bool((g == 7.0).all()) and bool((partial == 7.0).all())      # nothing ran


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
    return grads, saved


@gpu
def test_feature_decoder_switch_on_and_off(dev):
    """a small FeatureDecoder whose three stage boundaries are (256, 512), (128, 256) and (64, 128) through _forward_core /
    _backward_core with ops.DGRAD_LOWRES on and off, against the float64 autograd of the same nn.Module on the CPU: every parameter
    gradient, the new path at most twice the present path's error"""
    from adaptersis_amd.backbones.decoders import FeatureDecoder
    torch.manual_seed(11)
    m = FeatureDecoder(embed_dim=64, num_classes=2, features=[64, 512, 256, 128, 64])
    for i in range(1, 5):       # BatchNorm affines away from the identity
        bn = getattr(m, f"decoder_{i}")[1]
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
    m.train()
    x = torch.randn(2, 192, 4, 4)
    dl = torch.randn(2, 2, 64, 64) / 64.0
    ref = copy.deepcopy(m).double()
    y = x.double()
    for i in range(1, 5):
        y = getattr(ref, f"decoder_{i}")(y)
    y = ref.final_out(y)
    y.backward(dl.double())
    rgrads = {n: p.grad for n, p in ref.named_parameters()}
    res = {}
    old = ops.DGRAD_LOWRES
    try:
        for on in (False, True):
            ops.DGRAD_LOWRES = on
            mm = copy.deepcopy(m).to(dev).train()
            grads, saved = _module_run(dev, mm, x.to(dev), dl)
            assert [bool(getattr(saved[i - 1], "dgrad_lowres", False)) for i in (4, 3, 2)] == [on] * 3   # all three boundaries
            assert not getattr(saved[0], "dgrad_lowres", False)
            res[on] = grads
    finally:
        ops.DGRAD_LOWRES = old
    bad = []
    wmax = max(float(v.abs().max()) for v in rgrads.values())
    for n, r in rgrads.items():
        assert bool(torch.isfinite(res[True][n]).all()), n
        if float(r.abs().max()) < 1e-9 * wmax:      # exactly zero but for rounding: no relative error to compare
            continue
        e_new, e_old = rel_l2(res[True][n], r), rel_l2(res[False][n], r)
        print(f"MEASURE dgrad_lowres module {n}: new {e_new:.3e} present {e_old:.3e} ratio {e_new / max(e_old, 1e-30):.2f}")
        if not e_new <= 2.0 * e_old:
            bad.append((n, e_new, e_old))
    assert not bad, bad
