"""GPU: the hard-pixel losses (csrc/hardpixel.hip, ``ops.hardpixel_loss``, ``TopKLoss`` / ``DC_and_topk_loss`` / ``FocalLoss``, the
engine keys "topk" / "dc_and_topk" / "focal") against the reference's recorded results, against float64, and bit for bit.

Scheme (that of test_gpu_lovasz).  The select is checked EXACTLY: ``selected`` must equal the stable top-K
(``torch.sort(descending=True, stable=True)``) of the ``values`` read back from the device, so near-ties of float64 values cannot
make a check flaky and no pixel is ever masked or skipped.  ``values`` and ``dz`` are then checked pixel by pixel against the
float64 closed forms of tests/hardpixel_ref.py, the loss against the double sum of the device's own selected values.

Crafted values.  A focal value passes through log and pow, so it cannot carry a chosen bit pattern.  The cross entropy can: with
the label's logit -key, another logit 0 and the third -1e30, key >= 18, the kernel computes sum exp = 1 + exp(-key) + 0 = 1,
log 1 = 0 and v = w (0 - (-key - 0)) = w key with no rounding; w = -1 gives negative values and, with key 0, -0.  The key sets
below reach the select bit for bit (asserted), each so that one of the four digit passes decides alone, with ties across
workgroup boundaries (N = 3 WG + 17, WG = asis_hardpixel_tile()).  The focal kind runs the same select on random probabilities.

Bounds (u = 2^-24; none is taken from what the kernels give; derivations in the docstring of tests/hardpixel_ref.py):
  resize       dz = max(4 Y, 4 ulp max |z|) as in test_gpu_loss_kernels (Y = torch's float32 resize against float64), 0 for the
               identity.  P = lovasz_ref.prob_bound = 2 dz + E(D, C) 2^-23 for a probability of softmax(resize(logits)).
  values       cross entropy: |w| (2 dz + ce_bound(A, C, nll)); focal: focal_bounds with dq = P (n_softmax 1) or dz (0).
  loss         the double sum of the selected float32 values, scaled and rounded once: 2 u sum |v_sel| / K.
  dz           cross entropy: w (softmax - onehot) / K * grad_scale: the probability (P), the difference, the weight, 1 / K as a
               float and its product: |w| / K grad_scale (P + 4 u).  focal, n_softmax 0: the coefficient's bound times o_c, plus
               4 u of the element; n_softmax 1: the softmax transpose q_c (g_c - <g, q>) of g = c o carries q three times and
               a dot product over C: (3 P + (C + 8) u) sum_j |g_j| as in test_gpu_lovasz, plus the coefficient's bound through the
               same expression: cb (o_c q_c + q_c <o, q>).  Unselected pixels: EXACTLY 0.
  golden       the reference runs in float32; Y = its own distance to the float64 closed form of the same inputs, element by
               element (tests/test_hardpixel_cpu.py bounds it).  |device - reference| <= X + Y, X the device's bound above; the
               gap rule of the fixture makes the selected set the same, which is asserted on the gradient's zero pattern.
               dc_and_topk adds dice_bound / the dice gradient bound (valid for any float32 evaluation) and u |sum|.
  k = 100      TopKLoss(k=100) and CrossentropyND are two float32 evaluations of one mean: the sum of their bounds, ours as
               above (mean of the per-pixel bounds + 2 u |loss|), the fused loss kernel's ulp (U_ce + 6 |CE|) + 2 dz of
               test_gpu_loss_kernels with U_ce = 2 + 5 (C + 3 + 2 A) / sqrt(pixels).
  engine       the mean of the K largest is 1-Lipschitz in the sup norm of the values (no gap needed): the largest per-pixel
               bound + 2 u |ref|; focal (K = N): the mean of the bounds; dc_and_topk: + dice_bound + 4 dz (a probability moves
               by 2 dz of itself with the resize, numerator and denominator of a ratio <= 1 each by that) + u |sum|.
Every check prints a MEASURE line before it asserts (run with ``-s``).  Measured on one MI355X, largest err / bound over the 679
MEASURE lines: values 0.26 (cross entropy, identity resize), loss 0.47, dz 0.22 (focal on probabilities, 16 -> 37 resize),
select.loss 0.43; golden losses 0.07 and gradients 0.22 (focal, where the reference's own float32 error Y is most of the bound),
golden ops loss 0.004 / dz 0.03, k = 100 against CrossentropyND 0.000 (equal to the last bit here), engine loss 0.002 (the
dc_and_topk bound is the worst-case chain of 224^2 float32 adds and far above what either side does).  All 70 exact selections hold
(10 key sets x 7 values of K; high_byte: 122 distinct values over both signs).  46 cases, 2.3 s of pytest time.
test_more_tiles_than_one_scan_pass (4.2 M pixels, 3 values of K, one CPU sort) came later: select.loss 0.21, about 1 s."""
import json
import math

import pytest
import torch

from adaptersis_amd import _lib, ops
from adaptersis_amd import train as T
from adaptersis_amd import train_multi_class as TMC
from adaptersis_amd.backbones import engines as E
from adaptersis_amd.backbones.engines import SegEngine
from adaptersis_amd.segloss.ND_Crossentropy import CrossentropyND, TopKLoss
from adaptersis_amd.segloss.dice_loss import DC_and_topk_loss, SoftDiceLoss, softmax_helper
from adaptersis_amd.segloss.focal_loss import FocalLoss
from adaptersis_amd.utils import weights as W
from tests import hardpixel_ref as R
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
U = R.U
WG = _lib.lib().asis_hardpixel_tile()
CE, FOCAL = ops.HARDPIXEL_CE, ops.HARDPIXEL_FOCAL


def _measure(name, case, err, bound):
    err, bound = float(err), float(bound)
    print(f"MEASURE {name} {case}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound > 0 else (0.0 if err == 0 else math.inf):.3f}")
    return err <= bound


def _elementwise(name, case, got, ref, bound):
    """max over the elements of |got - ref| / bound (bound per element; 0 / 0 counts as 0)"""
    got, ref, bound = (torch.as_tensor(x).detach().double().cpu().reshape(-1) for x in (got, ref, bound))
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf).double())
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"MEASURE {name} {case}: max err {float(err.max()):.3e} max err/bound {worst:.3f}")
    return worst <= 1.0


def _resize_err(logits, H, Wd):
    if tuple(logits.shape[1:3]) == (H, Wd):
        return 0.0
    z64, z32 = R.resized64(logits, H, Wd), R.resized64(logits, H, Wd, torch.float32).double()
    return max(4.0 * float((z32 - z64).abs().max()), 4.0 * 2.0 ** -23 * float(z64.abs().max()))


def _reference(logits, labels, kind, K, *, n_softmax=0, gamma=2.0, smooth=1e-5, weight=None, size_average=True, grad_scale=1.0):
    """float64 values and per-pixel gradients of the inputs, with the device's bounds:
    -> (v64 [N], dv64 [N, C] scaled like dz, value bound [N], dz bound [N, C])"""
    B, h, w, C = logits.shape
    H, Wd = labels.shape[-2:]
    N = B * H * Wd
    z64 = R.resized64(logits, H, Wd).reshape(N, C)
    v64, dv64, aux = R.pixel_values(z64, labels.reshape(-1), kind, n_softmax=n_softmax, gamma=gamma, smooth=smooth, weight=weight)
    dzr = _resize_err(logits, H, Wd)
    f = (1.0 / K if size_average else 1.0) * grad_scale
    if kind == CE:
        vb = aux["w"].abs() * (2.0 * dzr + R.ce_bound(float(z64.abs().max()), C, aux["nll"]))
        vb = torch.where(aux["ok"], vb, torch.zeros_like(vb))
        gb = (aux["w"].abs() * f * (R.prob_bound(logits, H, Wd) + 4 * U)).view(-1, 1).expand(N, C)
    else:
        dq = R.prob_bound(logits, H, Wd) if n_softmax else dzr
        vb, cb = R.focal_bounds(aux, gamma, smooth, C, dq)
        o, q = aux["o"], aux["q"]
        g = (aux["w"] * R.focal_c(aux["pt"], gamma)).view(-1, 1) * o
        if n_softmax:
            gb = f * ((3 * dq + (C + 8) * U) * g.abs().sum(-1, keepdim=True) + cb.view(-1, 1) * (o * q + q * (o * q).sum(-1, keepdim=True)))
        else:
            gb = f * (cb.view(-1, 1) * o) + 4 * U * (dv64 * f).abs()
    return v64, dv64 * f, vb, gb


def _check(case, logits, labels, kind, K, dev, **cfg):
    """one call against float64 and against its own values -> (loss, dz, values, selected) on the CPU"""
    B, h, w, C = logits.shape
    N = labels.numel()
    weight = cfg.get("weight")
    kw = dict(cfg, class_weight=None if weight is None else weight.to(dev))
    kw.pop("weight", None)
    loss, dz, values, selected = ops.hardpixel_loss(logits.to(dev), labels.to(dev), kind, K, return_selection=True, **kw)
    loss, dz, values, selected = float(loss), dz.cpu().reshape(N, C), values.cpu(), selected.cpu().bool()
    v64, dz64, vb, gb = _reference(logits, labels, kind, K, **cfg)
    ok = [_elementwise("values", case, values, v64, vb)]
    want = R.stable_topk(values, K)
    assert torch.equal(selected, want), f"{case}: selection differs at {int((selected != want).sum())} pixels"
    f = 1.0 / K if cfg.get("size_average", True) else 1.0
    vs = values.double()[selected]
    ok.append(_measure("loss", case, abs(loss - float(vs.sum()) * f), 2 * U * float(vs.abs().sum()) * f))
    sel2 = selected.view(-1, 1)
    ok.append(_elementwise("dz", case, dz, dz64 * sel2, gb * sel2))
    valid = (labels.reshape(-1) >= 0) & (labels.reshape(-1) < C)
    if kind == CE and C == 1:   # one class: softmax - onehot = 0
        assert not bool(dz.any())
    else:
        assert torch.equal((dz != 0).any(-1), selected & valid), f"{case}: zero pattern of dz"
    assert all(ok), case
    return loss, dz, values, selected


# ---------------------------------------------------------------------------------------------------------------------------
# the select, exactly
def _bits(x):
    return x.to(torch.int32).view(torch.float32)


def _crafted(keys, labels01):
    """logits [1,1,N,3] and weights whose cross-entropy values are exactly keys (label 0) / -keys (label 1)"""
    N = keys.numel()
    z = torch.full((N, 3), -1e30)
    z[torch.arange(N), labels01] = -keys
    z[torch.arange(N), 1 - labels01] = torch.where(keys == 0, -1e30, 0.0)   # key 0: sum exp = 1 needs the label's term alone
    return z.view(1, 1, N, 3).contiguous(), labels01.view(1, 1, N), torch.tensor([1.0, -1.0, 1.0])


KEYSETS = ["all_equal", "two_values", "low_byte", "high_byte", "sorted", "reversed", "signed_zero", "all_zero", "mixed_labels",
           "focal_random"]


@pytest.mark.parametrize("kind", KEYSETS)
def test_select_exact(dev, kind):
    gen = torch.Generator().manual_seed(KEYSETS.index(kind))
    N, C = 3 * WG + 17, 3
    zero = torch.zeros(N, dtype=torch.int64)
    signs = torch.randint(0, 2, (N,), generator=gen)
    expect, op_kind, cfg = None, CE, {}
    if kind == "all_equal":
        expect = torch.full((N,), 32.0)
        logits, labels, w = _crafted(expect, zero)
    elif kind == "two_values":
        expect = torch.randint(0, 2, (N,), generator=gen) * 16.0 + 32.0
        logits, labels, w = _crafted(expect, zero)
    elif kind == "low_byte":
        expect = _bits(0x42000000 + torch.randint(0, 256, (N,), generator=gen))
        logits, labels, w = _crafted(expect, zero)
    elif kind == "high_byte":
        keys = _bits((torch.randint(0x42, 0x7F, (N,), generator=gen) << 24) + 0x345678)
        logits, labels, w = _crafted(keys, signs)
        expect = torch.where(signs == 1, -keys, keys)
    elif kind in ("sorted", "reversed"):
        ramp = torch.linspace(4000.0, 18.0, N)
        expect = ramp if kind == "sorted" else ramp.flip(0)
        logits, labels, w = _crafted(expect, zero)
    elif kind == "signed_zero":
        logits, labels, w = _crafted(torch.zeros(N), signs)
        expect = torch.where(signs == 1, -0.0, 0.0)
    elif kind == "all_zero":   # labels outside the range: every value is 0
        logits, labels, w = torch.randn((1, 1, N, C), generator=gen), torch.full((1, 1, N), C + 1, dtype=torch.int64), None
        labels[0, 0, ::3] = -100
        expect = torch.zeros(N)
    elif kind == "mixed_labels":
        logits, w = torch.randn((1, 1, N, C), generator=gen) * 2.0, None
        labels = torch.randint(-2, C + 2, (1, 1, N), generator=gen)
        labels[0, 0, ::7] = -100
    else:
        op_kind, w, cfg = FOCAL, None, dict(n_softmax=0, gamma=2.0, smooth=0.0)
        logits = torch.softmax(torch.randn((1, 1, N, C), generator=gen) * 2.0, -1)
        labels = torch.randint(0, C, (1, 1, N), generator=gen)
    lg, tg, wd = logits.to(dev), labels.to(dev), None if w is None else w.to(dev)
    scratch = torch.empty(ops.hardpixel_scratch_bytes(N), device=dev, dtype=torch.uint8)
    first = None
    for K in (1, 2, N - 1, N, WG, WG + 1, int(N * 10 / 100)):
        loss, dz, values, selected = ops.hardpixel_loss(lg, tg, op_kind, K, class_weight=wd, scratch=scratch, return_selection=True, **cfg)
        values, selected = values.cpu(), selected.cpu().bool()
        if expect is not None:   # the crafted bit patterns reach the select unchanged (-0 included)
            assert torch.equal(values.view(torch.int32), expect.view(torch.int32)), (kind, K)
        first = values if first is None else first
        assert torch.equal(values.view(torch.int32), first.view(torch.int32))
        want = R.stable_topk(values, K)
        nbad = int((selected != want).sum())
        print(f"MEASURE select {kind} K={K}: selected {int(selected.sum())} differing {nbad} distinct values {values.unique().numel()}")
        assert int(selected.sum()) == K and nbad == 0, (kind, K)
        if kind in ("all_equal", "signed_zero", "all_zero", "sorted"):
            assert bool(selected[:K].all())                                    # ties go to the lower pixel index
        vs = values.double()[selected]
        assert _measure("select.loss", (kind, K), abs(float(loss) - float(vs.sum()) / K), 2 * U * float(vs.abs().sum()) / K)
        dz = dz.cpu().view(N, C)
        valid = (labels.reshape(-1) >= 0) & (labels.reshape(-1) < C)
        if kind == "signed_zero":   # softmax = onehot exactly: the gradient of a selected pixel is 0 as well
            assert not bool(dz.any())
        else:
            assert torch.equal((dz != 0).any(-1), selected & valid), (kind, K)
    iv = first.view(torch.int32)
    if kind == "low_byte":
        assert int(((iv >> 8) != (0x42000000 >> 8)).sum()) == 0 and iv.unique().numel() == 256
    if kind == "high_byte":
        assert int(((iv & 0xFFFFFF) != 0x345678).sum()) == 0 and iv.unique().numel() > 100
    if kind == "signed_zero":
        assert set(iv.unique().tolist()) == {0, -(1 << 31)}


@pytest.mark.parametrize("N,C", [(1, 1), (63, 2), (WG - 1, 16), (WG, 8), (WG + 1, 3)])
def test_sizes_around_the_tile(dev, N, C):
    gen = torch.Generator().manual_seed(N * 17 + C)
    q = (torch.randint(1, 64, (1, 1, N, C), generator=gen).float() / 64.0)   # many ties: the index order matters
    lab = torch.randint(0, C, (1, 1, N), generator=gen)
    for K in sorted({1, max(1, N // 10), max(1, N - 1), N}):
        _check(("sizes", N, C, K), q, lab, FOCAL, K, dev, n_softmax=0, gamma=2.0, smooth=0.0)
        _check(("sizes.ce", N, C, K), q * 8.0, lab, CE, K, dev)


def test_more_tiles_than_one_scan_pass(dev):
    """WG + 2 tiles: the scan over the tiles' tie counts takes WG entries a pass (RX_TILE of csrc/radix_routines.h), so its carry
    runs, and so does the stride loop of the histogram passes (more tiles than their 1024 workgroups).  1024 distinct crafted
    values, about 4100 ties each, spread over all tiles; K puts the boundary among the ties of the value T at 10 %."""
    H, Wd = WG + 3, WG - 1
    N = H * Wd
    assert -(-N // WG) == WG + 2
    gen = torch.Generator().manual_seed(5)
    keys = (torch.randint(0, 1024, (N,), generator=gen) + 32).float()
    T = float(torch.sort(keys, descending=True).values[int(N * 10 / 100) - 1])
    if int((keys[WG * WG:] == T).sum()) < 2:   # the last two ties must lie behind the scan's first pass
        keys[-2:] = T
    logits, labels, w = _crafted(keys, torch.zeros(N, dtype=torch.int64))
    lg, tg, wd = logits.view(1, H, Wd, 3).to(dev), labels.view(1, H, Wd).to(dev), w.to(dev)
    order = torch.sort(keys, descending=True, stable=True).indices   # R.stable_topk for every K below from one sort
    above, ties = int((keys > T).sum()), int((keys == T).sum())
    tie_at = (keys == T).nonzero().view(-1)
    scratch = torch.empty(ops.hardpixel_scratch_bytes(N), device=dev, dtype=torch.uint8)
    for K in (above + ties - 1, above + 1, above + ties // 2):
        want = torch.zeros(N, dtype=torch.bool)
        want[order[:K]] = True
        if K == above + ties - 1:   # the last selected tie is in a tile of the second pass and one unselected tie follows it
            assert bool(want[tie_at[:-1]].all()) and not bool(want[tie_at[-1]]) and int(tie_at[-2]) // WG >= WG
        loss, dz, values, selected = ops.hardpixel_loss(lg, tg, CE, K, class_weight=wd, scratch=scratch, return_selection=True)
        values, selected = values.cpu(), selected.cpu().bool()
        assert torch.equal(values.view(torch.int32), keys.view(torch.int32)), K
        nbad = int((selected != want).sum())
        print(f"MEASURE select big K={K}: above {above} ties {ties} selected {int(selected.sum())} differing {nbad}")
        assert int(selected.sum()) == K and nbad == 0, K
        vs = values.double()[selected]
        assert _measure("select.loss", ("big", K), abs(float(loss) - float(vs.sum()) / K), 2 * U * float(vs.abs().sum()) / K)


# ---------------------------------------------------------------------------------------------------------------------------
# values, loss and dz against float64
SHAPES = [(B, h, w, H, Wd, C) for C in (2, 8, 16) for (h, w, H, Wd) in ((8, 8, 8, 8), (9, 7, 21, 17), (16, 16, 37, 37)) for B in (1, 2)]


@pytest.mark.parametrize("shape", SHAPES)
def test_against_float64(dev, shape):
    B, h, w, H, Wd, C = shape
    gen = torch.Generator().manual_seed(sum(shape))
    logits = torch.randn((B, h, w, C), generator=gen) * 1.5
    probs = torch.softmax(torch.randn((B, h, w, C), generator=gen) * 1.5, -1)
    labels = torch.randint(0, C, (B, H, Wd), generator=gen)
    labels[0, 0, 0], labels[-1, -1, -1] = -100, C          # two pixels of no class
    N = B * H * Wd
    K10 = int(N * 10 / 100)
    cw = torch.rand((C,), generator=gen) + 0.5
    a_float, a_list = R.alpha_vector(0.25, C, 1), R.alpha_vector([float(i + 1) for i in range(C)], C)
    _check(("ce", shape), logits, labels, CE, K10, dev)
    _check(("ce.weight", shape), logits, labels, CE, K10, dev, weight=cw)
    _check(("ce.all.sum", shape), logits, labels, CE, N, dev, weight=cw, size_average=False)
    _check(("focal.1", shape), logits, labels, FOCAL, N, dev, n_softmax=1, gamma=2.0, smooth=1e-5)
    _check(("focal.1.float", shape), logits, labels, FOCAL, N, dev, n_softmax=1, gamma=1.5, smooth=0.0, weight=a_float, size_average=False)
    _check(("focal.1.list.g0", shape), logits, labels, FOCAL, N, dev, n_softmax=1, gamma=0.0, smooth=1e-5, weight=a_list)
    _check(("focal.1.g0.s0", shape), logits, labels, FOCAL, K10, dev, n_softmax=1, gamma=0.0, smooth=0.0)
    _check(("focal.0", shape), probs, labels, FOCAL, N, dev, n_softmax=0, gamma=2.0, smooth=0.0)
    _check(("focal.0.list.topk", shape), probs, labels, FOCAL, K10, dev, n_softmax=0, gamma=1.5, smooth=1e-5, weight=a_list)


def test_bit_exact(dev):
    gen = torch.Generator().manual_seed(3)
    B, h, w, H, Wd, C = 2, 24, 20, 56, 70, 11
    logits, labels = torch.randn((B, h, w, C), generator=gen) * 2.0, torch.randint(0, C, (B, H, Wd), generator=gen)
    lg, tg = logits.to(dev), labels.to(dev)
    N = labels.numel()
    for kind, K, cfg in ((CE, N // 10, {}), (FOCAL, N, dict(n_softmax=1)), (FOCAL, N // 5, dict(n_softmax=1, gamma=1.5))):
        a = ops.hardpixel_loss(lg, tg, kind, K, return_selection=True, **cfg)
        b = ops.hardpixel_loss(lg, tg, kind, K, return_selection=True, **cfg)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), kind                       # two calls, the same bits
        scratch = torch.empty(ops.hardpixel_scratch_bytes(N) + 64, device=dev, dtype=torch.uint8)
        c = ops.hardpixel_loss(lg, tg, kind, K, scratch=scratch, **cfg)
        assert all(torch.equal(x, y) for x, y in zip(a[:2], c))                         # a reused, larger scratch
        s = ops.hardpixel_loss(lg, tg, kind, K, grad_scale=1024.0, **cfg)
        assert torch.equal(s[0], a[0]) and torch.equal(s[1], a[1] * 1024.0)             # grad_scale 1024 against 1
        base = torch.randn((B, H, Wd, C), generator=gen).to(dev)
        acc = ops.hardpixel_loss(lg, tg, kind, K, dz=base.clone(), **cfg)
        assert torch.equal(acc[1], base + a[1]) and torch.equal(acc[0], a[0])           # accumulate: the float32 sum
        assert torch.equal(acc[1][a[3].view(B, H, Wd) == 0], base[a[3].view(B, H, Wd) == 0])   # unselected: untouched
    with pytest.raises(ValueError, match="scratch"):
        ops.hardpixel_loss(lg, tg, CE, 10, scratch=scratch[:1000])
    with pytest.raises(ValueError, match="K="):
        ops.hardpixel_loss(lg, tg, CE, 0)
    with pytest.raises(ValueError, match="K="):
        ops.hardpixel_loss(lg, tg, CE, N + 1)
    with pytest.raises(ValueError):
        ops.hardpixel_loss(lg, tg.int(), CE, 10)
    with pytest.raises(ValueError):
        ops.hardpixel_loss(lg.double(), tg, CE, 10)
    with pytest.raises(ValueError):
        ops.hardpixel_loss(lg, tg, CE, 10, class_weight=torch.ones(C, device=dev, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's recorded results
@pytest.fixture(scope="module")
def golden():
    return load_golden("hardpixel_ref")["cases"]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_modules_against_the_reference(dev, golden, i):
    c = golden[i]
    B, h, w, C = c["shape"]
    N, K = B * h * w, c["K"]
    logits, target = c["logits"], c["target"]
    labels = target.reshape(-1)
    ok = []

    def nchw(d):
        return d.reshape(B, h, w, C).permute(0, 3, 1, 2)

    def run(module, inp):
        x = inp.to(dev).requires_grad_(True)
        out = module(x, target.to(dev).unsqueeze(1))
        out.backward()
        return float(out), x.grad.cpu()

    dice, ddice, coef = R.soft_dice(logits.double(), target)
    dice_b, ddice_b = R.dice_bounds(logits.double(), coef)
    z_nchw = logits.permute(0, 3, 1, 2).contiguous()
    for name, weight, module in (("topk", None, TopKLoss(k=10)), ("topk_w", c["weight"], TopKLoss(k=10, weight=c["weight"])),
                                 ("dc_and_topk", None, DC_and_topk_loss({}, {"k": 10}))):
        got, grad = run(module, z_nchw)
        v64, dz64, vb, gb = _reference(logits, target, CE, K, weight=weight)
        sel = R.stable_topk(v64, K)
        l64, X = float(v64[sel].sum()) / K, float(vb[sel].mean()) + 2 * U * abs(float(v64[sel].sum())) / K
        dz64, gb = dz64 * sel.view(-1, 1), gb * sel.view(-1, 1)
        if name == "dc_and_topk":
            l64, dz64 = l64 + float(dice), dz64 + ddice.reshape(N, C)
            X, gb = X + dice_b + U * abs(l64), gb + ddice_b.reshape(N, C)
        else:
            assert torch.equal(grad != 0, c["grad_" + name] != 0), f"{name}: the selected set"
        ref, gref = float(c["loss_" + name]), c["grad_" + name].double()
        ok.append(_measure(f"golden.loss.{name}", c["shape"], abs(got - ref), X + abs(ref - l64)))
        ok.append(_elementwise(f"golden.grad.{name}", c["shape"], grad, gref, nchw(gb) + (gref - nchw(dz64)).abs()))

    q_nhwc = c["probs"].permute(0, 2, 3, 1).contiguous()
    runs = (("focal", FocalLoss(), dict(gamma=2.0, smooth=1e-5), True),
            ("focal_float", FocalLoss(alpha=0.25, balance_index=1, gamma=1.5, size_average=False),
             dict(gamma=1.5, smooth=1e-5, weight=R.alpha_vector(0.25, C, 1)), False),
            ("focal_list", FocalLoss(alpha=c["alpha_list"], smooth=0), dict(gamma=2.0, smooth=0.0, weight=R.alpha_vector(c["alpha_list"], C)),
             True))
    for name, module, cfg, size_average in runs:
        got, grad = run(module, c["probs"])
        v64, dz64, vb, gb = _reference(q_nhwc, target, FOCAL, N, n_softmax=0, size_average=size_average, **cfg)
        f = 1.0 / N if size_average else 1.0
        l64 = float(v64.sum()) * f
        X = (float(vb.sum()) + 2 * U * float(v64.abs().sum())) * f
        ref, gref = float(c["loss_" + name]), c["grad_" + name].double()
        ok.append(_measure(f"golden.loss.{name}", c["shape"], abs(got - ref), X + abs(ref - l64)))
        ok.append(_elementwise(f"golden.grad.{name}", c["shape"], grad, gref, nchw(gb) + (gref - nchw(dz64)).abs()))

    # ops on the recorded logits (n_softmax = 1) against the reference's FocalLoss() of their float32 softmax
    loss, dz = ops.hardpixel_loss(logits.to(dev), target.to(dev), FOCAL, N, n_softmax=1)
    v64, dz64, vb, gb = _reference(logits, target, FOCAL, N, n_softmax=1)
    q64 = torch.softmax(logits.double().reshape(N, C), -1)
    g = c["grad_focal"].double().permute(0, 2, 3, 1).reshape(N, C)
    gref = q64 * (g - (g * q64).sum(-1, keepdim=True))
    ref = float(c["loss_focal"])
    ok.append(_measure("golden.ops.loss", c["shape"], abs(float(loss) - ref),
                       float(vb.mean()) + 2 * U * float(v64.abs().mean()) + abs(ref - float(v64.mean()))))
    ok.append(_elementwise("golden.ops.dz", c["shape"], dz.cpu().reshape(N, C), gref, gb + (gref - dz64).abs()))
    assert all(ok)


# ---------------------------------------------------------------------------------------------------------------------------
# modules
def test_autograd_through_the_resize_transpose(dev):
    gen = torch.Generator().manual_seed(11)
    B, C, h, w, H, Wd = 2, 8, 9, 7, 21, 17
    x = torch.randn((B, C, h, w), generator=gen).to(dev)
    tgt = torch.randint(0, C, (B, 1, H, Wd), generator=gen).to(dev)
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    K = int(B * H * Wd * 10 / 100)
    for module, direct in ((TopKLoss(k=10), lambda: ops.hardpixel_loss(nhwc, tgt[:, 0].contiguous(), CE, K)),
                           (FocalLoss(apply_nonlin=softmax_helper, gamma=1.5),
                            lambda: ops.hardpixel_loss(nhwc, tgt[:, 0].contiguous(), FOCAL, B * H * Wd, n_softmax=1, gamma=1.5))):
        p = x.clone().requires_grad_(True)
        out = module(p, tgt)
        (out * 3.0).backward()
        loss, dz = direct()
        low, _ = ops.resize_bilinear_bwd(dz, h, w, torch.float32)
        assert torch.equal(out.detach().view(1), loss)
        assert torch.equal(p.grad, low.permute(0, 3, 1, 2) * 3.0)                      # the bits of the direct composition
        assert p.grad.shape == x.shape and bool(p.grad.abs().sum() > 0)


def test_dc_and_topk_is_the_sum_of_its_halves(dev):
    gen = torch.Generator().manual_seed(12)
    B, C, H, Wd = 2, 8, 21, 17
    x = torch.randn((B, C, H, Wd), generator=gen).to(dev)
    tgt = torch.randint(0, C, (B, 1, H, Wd), generator=gen).to(dev)
    grads, outs = [], []
    for module in (DC_and_topk_loss({}, {"k": 20}), TopKLoss(k=20), SoftDiceLoss(apply_nonlin=softmax_helper)):
        p = x.clone().requires_grad_(True)
        out = module(p, tgt)
        out.backward()
        outs.append(out.detach())
        grads.append(p.grad)
    assert torch.equal(outs[0], outs[1] + outs[2]) and torch.equal(grads[0], grads[1] + grads[2])


@pytest.mark.parametrize("shape", [(2, 8, 9, 7, 21, 17), (1, 3, 16, 16, 16, 16)])
def test_topk_100_is_the_cross_entropy(dev, shape):
    B, C, h, w, H, Wd = shape
    gen = torch.Generator().manual_seed(13)
    x = torch.randn((B, C, h, w), generator=gen) * 2.0
    tgt = torch.randint(0, C, (B, 1, H, Wd), generator=gen)
    a = float(TopKLoss(k=100)(x.to(dev), tgt.to(dev)))
    b = float(CrossentropyND()(x.to(dev), tgt.to(dev)))
    nhwc = x.permute(0, 2, 3, 1).contiguous()
    v64, _, vb, _ = _reference(nhwc, tgt[:, 0], CE, tgt.numel())
    ce, A, dzr = float(v64.mean()), float(R.resized64(nhwc, H, Wd).abs().max()), _resize_err(nhwc, H, Wd)
    ours = float(vb.mean()) + 2 * U * abs(ce)
    fused = 2.0 ** -23 * (2 + 5 * (C + 3 + 2 * A) / math.sqrt(tgt.numel()) + 6 * abs(ce)) + 2 * dzr
    assert _measure("k100.float64", shape, abs(a - ce), ours)
    assert _measure("k100.crossentropy", shape, abs(a - b), ours + fused)


# ---------------------------------------------------------------------------------------------------------------------------
# engine
class _Kind:
    def __init__(self, kind, **kw):
        self.loss_kind = kind
        self.__dict__.update(kw)


def test_engine_loss_stage_dispatch(dev):
    gen = torch.Generator().manual_seed(1)
    B, h, w, H, Wd, C = 2, 24, 20, 56, 70, 11
    lg = (torch.randn((B, h, w, C), generator=gen) * 2.0).to(dev)
    tg = torch.randint(0, C, (B, H, Wd), generator=gen).to(dev)
    N, S = tg.numel(), 256.0
    holder = _Kind("topk", topk_percent=20.0)
    got = E.loss_and_dz(holder, lg, tg, S)
    direct = ops.hardpixel_loss(lg, tg, CE, int(N * 20.0 / 100), grad_scale=S)
    assert torch.equal(got[0], direct[0]) and torch.equal(got[1], direct[1])
    first = holder._hardpixel_scratch
    E.loss_and_dz(holder, lg, tg, S)
    assert holder._hardpixel_scratch is first and first.numel() == ops.hardpixel_scratch_bytes(N)   # kept between steps
    dflt = E.loss_and_dz(_Kind("topk"), lg, tg, S)                                     # an engine without the attribute: 10 %
    d10 = ops.hardpixel_loss(lg, tg, CE, int(N * 10.0 / 100), grad_scale=S)
    assert torch.equal(dflt[0], d10[0]) and torch.equal(dflt[1], d10[1])
    dc, coef, _ = ops.seg_loss_fwd(lg, tg, 1, ops.LOSS_SOFTDICE, 1.0, 0, None, S)
    dz_dc = ops.seg_loss_bwd(lg, tg, coef, 1, ops.LOSS_SOFTDICE, 0, None)
    both = E.loss_and_dz(_Kind("dc_and_topk", topk_percent=20.0), lg, tg, S)
    assert torch.equal(both[0], dc + direct[0]) and torch.equal(both[1], dz_dc + direct[1])
    fo = E.loss_and_dz(_Kind("focal", focal_gamma=1.5), lg, tg, S)
    dfo = ops.hardpixel_loss(lg, tg, FOCAL, N, n_softmax=1, gamma=1.5, smooth=1e-5, grad_scale=S)
    assert torch.equal(fo[0], dfo[0]) and torch.equal(fo[1], dfo[1])
    with pytest.raises(ValueError, match="selects no pixel"):
        E.loss_and_dz(_Kind("topk", topk_percent=1e-6), lg, tg, S)


def _engine(dev, loss, C=8, **kw):
    args = TMC.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4",
                                             "--num_classes", str(C)])
    torch.manual_seed(0)
    model, enc, cv, cn, dec = T.build_modules(args, "mla", C, dev)
    return SegEngine(model, enc, cv, cn, dec, lr=0.02, momentum=0.9, weight_decay=0.0, num_classes=C, loss=loss, **kw)


@pytest.mark.parametrize("kind", ["topk", "dc_and_topk", "focal"])
def test_engine_step_and_descent(dev, kind):
    C = 8
    eng = _engine(dev, kind, C, topk_percent=20.0, focal_gamma=1.5)
    assert eng.topk_percent == 20.0 and eng.focal_gamma == 1.5
    img, tgt = W.synthetic_batch(4, 224, C)
    img, tgt = img.to(dev), tgt.to(dev)
    taps = {}
    first = float(eng.train_step(img, tgt, taps))
    logits, labels = taps["logits"].cpu(), tgt.cpu().long()
    N = labels.numel()
    if kind == "focal":
        v64, _, vb, _ = _reference(logits, labels, FOCAL, N, n_softmax=1, gamma=1.5, smooth=1e-5)
        ref = float(v64.mean())
        bound = float(vb.mean()) + 2 * U * float(v64.abs().mean())
    else:
        K = int(N * 20.0 / 100)
        v64, _, vb, _ = _reference(logits, labels, CE, K)
        ref = float(v64[R.stable_topk(v64, K)].mean())
        bound = float(vb.max()) + 2 * U * abs(ref)
        if kind == "dc_and_topk":
            z64 = R.resized64(logits, *labels.shape[-2:])
            dice, _, coef = R.soft_dice(z64, labels)
            ref += float(dice)
            bound += R.dice_bounds(z64, coef)[0] + 4 * _resize_err(logits, *labels.shape[-2:]) + U * abs(ref)
    assert _measure("engine.loss", kind, abs(first - ref), bound)
    losses = [first] + [float(eng.train_step(img, tgt)) for _ in range(10)]
    print("MEASURE engine.descent", kind, " ".join(f"{x:.4f}" for x in losses))
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]


def test_train_multi_class_with_the_flags(dev, tmp_path):
    args = TMC.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4", "--lr", "0.08",
                                             "--data_path", "synthetic", "--num_workers", "0", "--output_dir", str(tmp_path),
                                             "--epochs", "1", "--num_classes", "8", "--loss", "dc_and_topk", "--topk_percent", "20"])
    T._ENGINES.clear()
    stats = TMC.train_seg(args)
    (eng,) = T._ENGINES.values()
    T._ENGINES.clear()
    assert eng.loss_kind == "dc_and_topk" and eng.topk_percent == 20.0 and eng.num_classes == 8
    assert {"train_loss", "test_ch_iou", "test_isi_iou"} <= set(stats) and math.isfinite(stats["train_loss"])
    assert stats["train_loss"] > -1.0                                                   # SoftDice >= -1, the cross entropy >= 0
    line = json.loads(open(tmp_path / "log.txt").readline())
    assert "test_ch_iou" in line
    ck = torch.load(tmp_path / "checkpoint.pth.tar", map_location="cpu")
    assert ck["epoch"] == 1
