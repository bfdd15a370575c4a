"""GPU: the Lovasz-Softmax loss (csrc/lovasz.hip, ``ops.lovasz_softmax``, ``segloss.lovasz_loss.LovaszSoftmax``, the engine keys
"lovasz" / "ce_lovasz") against the reference's recorded results, against the float64 closed form, and bit for bit.

Scheme.  The sort is checked EXACTLY: ``order`` must equal ``torch.sort(keys, descending=True, stable=True)`` of the keys read back
from the device.  Loss and gradient are then checked against the float64 closed form (tests/lovasz_ref.py) evaluated from that
order and those keys, so near-ties of float64 keys cannot make a check flaky and no pixel is ever masked or skipped.

Bounds (u = 2^-24, one rounding to float32; none is taken from what the kernels give):
  g            class pixel 1/U, other I/(U(U-1)) from integer counts in double: three roundings of 2^-53, nothing next to u.
  per_class    sum of e g >= 0 in double in a fixed order (no cancellation, N 2^-53 relative), one rounding to float32: 2 u |ref|.
               loss: the mean or sum of C such values in double, one rounding: 2 u |ref|.
  d = s g / C  the double g rounded to float32 (u), the float32 factor 1/C (u), their product (u), grad_scale (u; exact for
               a power of two): 4 u |ref| per element, relative.
  keys         n_softmax = 0 with the sizes equal: the taps are 1 and 0, e = |t - q| is ONE float32 rounding of the exact value
               (t = 1) or exact (t = 0): u |ref|.  n_softmax = 1: |q - q64| <= P = 2 dz + E(D, C) 2^-23 (lovasz_ref.prob_bound:
               the resize error dz of test_gpu_loss_kernels, max(4 Y, 4 ulp max|z|), moves a probability by <= 2 dz; E(D, C) =
               2 (D + 1) + (C - 1) / 2 + 2 ulps is the softmax bound derived there), one more rounding for 1 - q: P + u.
  dz           n_softmax = 1: dz_c = q_c (d_c - <d, q>) with the float64 d of the device's own order: the three factors that
               carry q are each off by <= P, |d_c - <d, q>| <= 2 D1, D1 = sum_j |d_j| of the pixel; the dot product over C,
               the difference, the product, d itself (4 u) and grad_scale: (3 P + (C + 8) u) D1 per element.
  golden       the reference runs in float32; Y = its own distance to the float64 closed form of the same inputs, element by
               element.  |device - reference| <= X + Y with X the bound of the device against that float64 evaluation: module
               (same float32 probabilities, gaps >= 1e-5 so the order is the same): loss 3 u |ref| (the rounding of e, the
               sum, the result), gradient 4 u |ref|.  ops on the recorded logits (n_softmax = 1): the loss is 1-Lipschitz in
               the sup norm of the keys (g >= 0 sums to 1), so X = P + u + 2 u |ref|; dz as above.
  engine       float64 loss of ``taps["logits"]``: X = P + u + 2 u |ref| as above (the Lipschitz argument needs no gap);
               "ce_lovasz" adds the cross-entropy bound of test_gpu_loss_kernels, ulp (U_ce + 6 |CE|) + 2 dz,
               U_ce = 2 + 5 (C + 3 + 2 A) / sqrt(pixels), and one rounding of the sum.
Every check prints a MEASURE line before it asserts (run with ``-s``).  Measured on one MI355X, largest err / bound: keys 0.05,
per_class and loss 0.39, d (n_softmax = 0) 0.50, dz (n_softmax = 1) 0.32, engine loss 0.001; golden gradients 1.00 where the
reference's own float32 error Y is the whole bound and the device sits on the float64 value.  34 cases, 3 s of pytest time."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

from adaptersis_amd import _lib, ops
from adaptersis_amd import train as T
from adaptersis_amd import train_multi_class as TMC
from adaptersis_amd.backbones import engines as E
from adaptersis_amd.backbones.engines import SegEngine
from adaptersis_amd.segloss.lovasz_loss import LovaszSoftmax
from adaptersis_amd.utils import weights as W
from tests import lovasz_ref as R
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
U = R.ULP24
TILE = _lib.lib().asis_lovasz_tile()
SCAN_CHUNK = TILE   # entries one pass of the row-scan workgroup handles (RX_TILE of csrc/radix_routines.h: 256 threads x 8)


def _measure(name, case, err, bound):
    err, bound = float(err), float(bound)
    print(f"MEASURE {name} {case}: err {err:.3e} bound {bound:.3e} ratio {err / bound if bound > 0 else (0.0 if err == 0 else math.inf):.3f}")
    return err <= bound


def _elementwise(name, case, got, ref, bound):
    """max over the elements of |got - ref| / bound (bound per element; 0 / 0 counts as 0)"""
    err = (got.double().cpu() - ref).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, 0.0, math.inf).double())
    worst = float(ratio.max()) if ratio.numel() else 0.0
    print(f"MEASURE {name} {case}: max err {float(err.max()):.3e} max err/bound {worst:.3f}")
    return worst <= 1.0


def _exact_checks(case, q, labels, dev, reduction="mean", grad_scale=1.0):
    """n_softmax = 0 on given ``q`` [B,H,W,C]: order EQUAL, per_class / loss / dz against the float64 closed form of the
    device's keys.  -> (keys, order, dz) on the CPU."""
    B, H, Wd, C = q.shape
    loss, pc, dz, keys, order = ops.lovasz_softmax(q.to(dev), labels.to(dev), 0, reduction, grad_scale, return_order=True)
    keys, order, dz = keys.cpu(), order.cpu().long(), dz.cpu()
    lab = labels.reshape(-1)
    k_exact = R.keys_of(q.double(), labels)
    ok = [_elementwise("keys", case, keys, k_exact, U * k_exact)]
    want = R.stable_order(keys)
    assert torch.equal(order, want), f"{case}: order differs at {int((order != want).sum())} positions"
    pc64, d64 = R.closed_form(keys.double(), lab, want)
    l64, fac = R.reduce(pc64, reduction)
    ok.append(_elementwise("per_class", case, pc, pc64, 2 * U * pc64.abs()))
    ok.append(_measure("loss", case, abs(float(loss) - float(l64)), 2 * U * abs(float(l64))))
    dref = d64 * fac * grad_scale
    ok.append(_elementwise("dz", case, dz.reshape(-1, C), dref, 4 * U * dref.abs()))
    assert torch.equal(dz.reshape(-1, C) == 0, dref == 0), f"{case}: zero pattern of dz"
    assert all(ok), case
    return keys, order, dz


def _from_keys(K, labels):
    """q [1,1,N,C] whose keys |t - q| are K [N, C] wherever that is exact (t = 0: q = K; t = 1: q = 1 - K)."""
    N, C = K.shape
    t = labels.reshape(-1, 1) == torch.arange(C).view(1, C)
    return torch.where(t, 1.0 - K, K).float().view(1, 1, N, C).contiguous(), labels.view(1, 1, N)


def _bits(x):
    return x.to(torch.int32).view(torch.float32)


KEYSETS = ["all_equal", "two_values", "low_byte", "high_byte", "sorted", "reversed", "zero_one", "above_one", "no_pixel",
           "every_pixel", "outside_labels"]


@pytest.mark.parametrize("kind", KEYSETS)
def test_key_sets_exact(dev, kind):
    gen = torch.Generator().manual_seed(KEYSETS.index(kind))
    N, C = 3 * TILE + 17, 3
    labels = torch.randint(0, C, (N,), generator=gen)
    none = torch.full((N,), C + 2, dtype=torch.int64)   # a label of no class: every key is q itself, bit for bit
    if kind == "all_equal":
        q, lab = _from_keys(torch.full((N, C), 0.5), labels)
    elif kind == "two_values":
        q, lab = _from_keys(torch.randint(0, 2, (N, C), generator=gen) * 0.5 + 0.25, labels)
    elif kind == "low_byte":
        q, lab = _from_keys(_bits(0x3F000000 + torch.randint(0, 256, (N, C), generator=gen)), none)
    elif kind == "high_byte":
        q, lab = _from_keys(_bits((torch.randint(1, 0x7F, (N, C), generator=gen) << 24) + 0x345678), none)
    elif kind in ("sorted", "reversed"):
        ramp = torch.linspace(0.999, 0.001, N).view(N, 1).repeat(1, C)
        q, lab = _from_keys(ramp if kind == "sorted" else ramp.flip(0), none if kind == "sorted" else labels)
    elif kind == "zero_one":
        q, lab = torch.randint(0, 2, (1, 1, N, C), generator=gen).float(), labels.view(1, 1, N)
    elif kind == "above_one":
        q, lab = torch.randn((1, 1, N, C), generator=gen) * 3.0, labels.view(1, 1, N)
    elif kind == "no_pixel":
        q, lab = torch.rand((1, 1, N, C), generator=gen), torch.randint(1, C, (1, 1, N), generator=gen)   # class 0 absent
    elif kind == "every_pixel":
        q, lab = torch.rand((1, 1, N, C), generator=gen), torch.full((1, 1, N), 1, dtype=torch.int64)
    else:
        q, lab = torch.rand((1, 1, N, C), generator=gen), torch.randint(-2, C + 2, (1, 1, N), generator=gen)
    keys, order, dz = _exact_checks(kind, q, lab, dev)
    if kind == "all_equal":
        assert torch.equal(order, torch.arange(N).repeat(C, 1))
    if kind in ("low_byte", "high_byte", "sorted"):
        assert torch.equal(keys, q.view(N, C).t())   # the crafted bit patterns reach the sort unchanged
    if kind == "low_byte":
        assert int(((keys.view(torch.int32) >> 8) != (0x3F000000 >> 8)).sum()) == 0
    if kind == "high_byte":
        assert int(((keys.view(torch.int32) & 0xFFFFFF) != 0x345678).sum()) == 0 and keys.view(torch.int32).unique().numel() > 100
    if kind == "sorted":
        assert torch.equal(order, torch.arange(N).repeat(C, 1))
    if kind == "zero_one":
        assert int((keys == 0).sum()) > N // 2 and bool((dz.view(N, C)[keys.t() == 0] == 0).all())


@pytest.mark.parametrize("N,C,reduction", [(1, 1, "mean"), (1, 16, "sum"), (TILE - 1, 2, "mean"), (TILE, 8, "none"),
                                           (TILE + 1, 16, "mean"), (3 * TILE + 17, 1, "sum"), (63, 8, "mean")])
def test_sizes_around_the_tile(dev, N, C, reduction):
    gen = torch.Generator().manual_seed(N * 17 + C)
    q = torch.randint(0, 64, (1, 1, N, C), generator=gen).float() / 64.0   # many ties: the stable order matters
    lab = torch.randint(0, C, (1, 1, N), generator=gen)
    _exact_checks((N, C, reduction), q, lab, dev, reduction)


def test_more_tile_totals_than_one_scan_pass(dev):
    """the scans over the tiles (histogram rows, class-pixel totals) take SCAN_CHUNK entries a pass: SCAN_CHUNK + 2 tiles"""
    H, Wd = SCAN_CHUNK + 3, TILE - 1
    N = H * Wd
    assert -(-N // TILE) > SCAN_CHUNK
    gen = torch.Generator().manual_seed(7)
    q = torch.randint(0, 1 << 16, (1, H, Wd, 1), generator=gen).float() / float(1 << 16)
    lab = torch.randint(0, 2, (1, H, Wd), generator=gen)
    _exact_checks(("big", N), q, lab, dev)


def _softmax_path(case, logits, labels, dev, reduction="mean"):
    B, h, w, C = logits.shape
    H, Wd = labels.shape[-2:]
    loss, pc, dz, keys, order = ops.lovasz_softmax(logits.to(dev), labels.to(dev), 1, reduction, 1.0, return_order=True)
    keys, order, dz = keys.cpu(), order.cpu().long(), dz.cpu()
    P = R.prob_bound(logits, H, Wd)
    q64 = torch.softmax(R.resized64(logits, H, Wd), -1)
    k64 = R.keys_of(q64, labels)
    ok = [_measure("keys", case, (keys.double() - k64).abs().max(), P + U)]
    want = R.stable_order(keys)
    assert torch.equal(order, want), f"{case}: order differs at {int((order != want).sum())} positions"
    pc64, d64 = R.closed_form(keys.double(), labels.reshape(-1), want)
    l64, fac = R.reduce(pc64, reduction)
    ok.append(_elementwise("per_class", case, pc, pc64, 2 * U * pc64.abs()))
    ok.append(_measure("loss", case, abs(float(loss) - float(l64)), 2 * U * abs(float(l64))))
    d = d64 * fac
    qf = q64.reshape(-1, C)
    dz64 = qf * (d - (d * qf).sum(-1, keepdim=True))
    bound = ((3 * P + (C + 8) * U) * d.abs().sum(-1, keepdim=True)).expand_as(dz64)
    ok.append(_elementwise("dz", case, dz.reshape(-1, C), dz64, bound))
    assert all(ok), case
    return float(loss), dz, float(l64), dz64, P


@pytest.mark.parametrize("shape", [(2, 24, 20, 56, 70, 11), (2, 30, 26, 13, 17, 3), (1, 9, 40, 31, 23, 16), (2, 16, 12, 16, 12, 2)])
def test_resize_and_softmax_path(dev, shape):
    B, h, w, H, Wd, C = shape
    gen = torch.Generator().manual_seed(sum(shape))
    logits = torch.randn((B, h, w, C), generator=gen) * 2.0
    labels = torch.randint(0, C, (B, H, Wd), generator=gen)
    _softmax_path(shape, logits, labels, dev)


@pytest.fixture(scope="module")
def golden():
    return load_golden("lovasz_ref")["cases"]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_module_against_the_reference(dev, golden, i):
    c = golden[i]
    probs, target = c["probs"], c["target"]
    C = probs.shape[1]
    keys64 = R.keys_of(probs.double().permute(0, 2, 3, 1), target)
    pc64, d64 = R.closed_form(keys64, target.reshape(-1), R.stable_order(keys64))
    ok = []
    for red in ("mean", "sum", "none"):
        p = probs.to(dev).requires_grad_(True)
        tgt = target.to(dev) if red != "sum" else target.to(dev).unsqueeze(1)   # (B,H,W) and (B,1,H,W)
        out = LovaszSoftmax(reduction=red)(p, tgt)
        ref = c["loss_" + red].double()
        l64 = pc64 if red == "none" else R.reduce(pc64, red)[0]
        ok.append(_elementwise(f"golden.loss.{red}", c["shape"], out.detach().reshape(-1), ref.reshape(-1),
                               (3 * U * l64.abs() + (ref - l64).abs()).reshape(-1)))
        out.sum().backward()
        gref = c["grad_" + ("mean" if red == "mean" else "sum")].double()
        g64 = (d64 * (1.0 / C if red == "mean" else 1.0)).view(*target.shape, C).permute(0, 3, 1, 2)
        ok.append(_elementwise(f"golden.grad.{red}", c["shape"], p.grad, gref, 4 * U * g64.abs() + (gref - g64).abs()))
    assert all(ok)


@pytest.mark.parametrize("i", [0, 1, 2])
def test_ops_on_the_recorded_logits(dev, golden, i):
    c = golden[i]
    logits, target = c["logits"], c["target"]
    B, h, w, C = logits.shape
    loss, dz, l64, dz64, P = _softmax_path(("golden", c["shape"]), logits, target, dev)
    ref = float(c["loss_mean"])
    q64 = torch.softmax(logits.double(), -1)
    k64 = R.keys_of(q64, target)
    pc_e, d_e = R.closed_form(k64, target.reshape(-1), R.stable_order(k64))   # float64 evaluation of the same inputs
    le = float(pc_e.mean())
    ok = [_measure("golden.ops.loss", c["shape"], abs(loss - ref), P + U + 2 * U * abs(le) + abs(ref - le))]
    qf = q64.reshape(-1, C)

    def through_softmax(d):
        return qf * (d - (d * qf).sum(-1, keepdim=True))

    dref = through_softmax(c["grad_mean"].double().permute(0, 2, 3, 1).reshape(-1, C))
    de = through_softmax(d_e / C)
    bound = ((3 * P + (C + 8) * U) * (d_e / C).abs().sum(-1, keepdim=True)).expand_as(de) + (dref - de).abs()
    ok.append(_elementwise("golden.ops.dz", c["shape"], dz.reshape(-1, C), dref, bound))
    assert all(ok)


def _case(seed=0, shape=(2, 24, 20, 56, 70, 11)):
    B, h, w, H, Wd, C = shape
    gen = torch.Generator().manual_seed(seed)
    return torch.randn((B, h, w, C), generator=gen) * 2.0, torch.randint(0, C, (B, H, Wd), generator=gen)


def test_bit_exact(dev):
    logits, labels = _case()
    lg, tg = logits.to(dev), labels.to(dev)
    a = ops.lovasz_softmax(lg, tg, 1, "mean", 1.0, return_order=True)
    b = ops.lovasz_softmax(lg, tg, 1, "mean", 1.0, return_order=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))                       # two calls, the same bits
    scratch = torch.empty(ops.lovasz_scratch_bytes(labels.numel(), 11) + 64, device=dev, dtype=torch.uint8)
    c = ops.lovasz_softmax(lg, tg, 1, "mean", 1.0, scratch=scratch)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], c))                   # a reused, larger scratch
    s = ops.lovasz_softmax(lg, tg, 1, "mean", 1024.0)
    assert torch.equal(s[0], a[0]) and torch.equal(s[2], a[2] * 1024.0)       # grad_scale 1024 against 1
    # accumulate: dz_ce + dz_lovasz to one rounding, i.e. the float32 sum of the two separate results
    ce, coef, _ = ops.seg_loss_fwd(lg, tg, 0, ops.LOSS_NONE, 0.0, 1, None, 1.0)
    dz_ce = ops.seg_loss_bwd(lg, tg, coef, 0, ops.LOSS_NONE, 1, None)
    acc = ops.lovasz_softmax(lg, tg, 1, "mean", 1.0, dz=dz_ce.clone())
    assert torch.equal(acc[2], dz_ce + a[2]) and torch.equal(acc[0], a[0])
    with pytest.raises(ValueError):
        ops.lovasz_softmax(lg, tg, 1, "mean", 1.0, scratch=scratch[:1000])
    with pytest.raises(ValueError):
        ops.lovasz_softmax(lg, tg, 1, "median")
    with pytest.raises(ValueError):
        ops.lovasz_softmax(lg, tg.int(), 1)


class _Kind:
    def __init__(self, kind):
        self.loss_kind = kind


def test_engine_loss_stage_dispatch(dev):
    """the six earlier keys: the bits of a direct seg_loss_fwd / seg_loss_bwd call; "ce_lovasz": the sum of its halves"""
    logits, labels = _case(1)
    lg, tg = logits.to(dev), labels.to(dev)
    S = 256.0
    for kind in ("dice", "iou", "softdice", "dc_and_ce", "tversky", "ce_dc"):
        n_region, mode, eps, n_ce = SegEngine.LOSSES[kind]
        loss, coef, _ = ops.seg_loss_fwd(lg, tg, n_region, mode, eps, n_ce, None, S)
        dz = ops.seg_loss_bwd(lg, tg, coef, n_region, mode, n_ce, None)
        got = E.loss_and_dz(_Kind(kind), lg, tg, S)
        assert torch.equal(got[0], loss) and torch.equal(got[1], dz), kind
    holder = _Kind("lovasz")
    lv = E.loss_and_dz(holder, lg, tg, S)
    direct = ops.lovasz_softmax(lg, tg, 1, "mean", S)
    assert torch.equal(lv[0], direct[0]) and torch.equal(lv[1], direct[2])
    first = holder._lovasz_scratch
    E.loss_and_dz(holder, lg, tg, S)
    assert holder._lovasz_scratch is first                                    # the scratch is kept between steps
    ce, coef, _ = ops.seg_loss_fwd(lg, tg, 0, ops.LOSS_NONE, 0.0, 1, None, S)
    dz_ce = ops.seg_loss_bwd(lg, tg, coef, 0, ops.LOSS_NONE, 1, None)
    both = E.loss_and_dz(_Kind("ce_lovasz"), lg, tg, S)
    assert torch.equal(both[0], ce + direct[0]) and torch.equal(both[1], dz_ce + direct[2])


def _engine(dev, loss, C=8):
    args = TMC.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4",
                                             "--num_classes", str(C)])
    torch.manual_seed(0)
    model, enc, cv, cn, dec = T.build_modules(args, "mla", C, dev)
    return SegEngine(model, enc, cv, cn, dec, lr=0.02, momentum=0.9, weight_decay=0.0, num_classes=C, loss=loss)


@pytest.mark.parametrize("kind", ["lovasz", "ce_lovasz"])
def test_engine_step_and_descent(dev, kind):
    C = 8
    eng = _engine(dev, kind, C)
    img, tgt = W.synthetic_batch(4, 224, C)
    img, tgt = img.to(dev), tgt.to(dev)
    taps = {}
    first = float(eng.train_step(img, tgt, taps))
    logits = taps["logits"].cpu()
    labels = tgt.cpu().long()
    H, Wd = labels.shape[-2:]
    P = R.prob_bound(logits, H, Wd)
    z64 = R.resized64(logits, H, Wd)
    k64 = R.keys_of(torch.softmax(z64, -1), labels)
    pc64, _ = R.closed_form(k64, labels.reshape(-1), R.stable_order(k64))
    ref = float(pc64.mean())
    bound = P + U + 2 * U * abs(ref)
    if kind == "ce_lovasz":
        ce = float(F.cross_entropy(z64.reshape(-1, C), labels.reshape(-1)))
        A = float(z64.abs().max())
        bound += 2.0 ** -23 * (2 + 5 * (C + 3 + 2 * A) / math.sqrt(labels.numel()) + 6 * abs(ce)) + P + U * abs(ref + ce)
        ref += ce
    assert _measure("engine.loss", kind, abs(first - ref), bound)
    losses = [first] + [float(eng.train_step(img, tgt)) for _ in range(10)]
    print("MEASURE engine.descent", kind, " ".join(f"{x:.4f}" for x in losses))
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0]


def test_train_multi_class_with_the_flag(dev, tmp_path):
    args = TMC.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4", "--lr", "0.08",
                                             "--data_path", "synthetic", "--num_workers", "0", "--output_dir", str(tmp_path),
                                             "--epochs", "1", "--num_classes", "8", "--loss", "lovasz"])
    T._ENGINES.clear()
    stats = TMC.train_seg(args)
    (eng,) = T._ENGINES.values()
    T._ENGINES.clear()
    assert eng.loss_kind == "lovasz" and eng.num_classes == 8
    assert {"train_loss", "test_ch_iou", "test_isi_iou"} <= set(stats) and math.isfinite(stats["train_loss"])
    assert 0.0 < stats["train_loss"] <= 1.0                                   # a mean of Lovasz extensions of Jaccard losses
    line = json.loads(open(tmp_path / "log.txt").readline())
    assert "test_ch_iou" in line
    ck = torch.load(tmp_path / "checkpoint.pth.tar", map_location="cpu")
    assert ck["epoch"] == 1
