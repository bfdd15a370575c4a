"""CPU: the host side of the hard-pixel losses (top-k cross entropy, focal) — the C-ABI entries that need no GPU, the argument
errors of ``asis_hardpixel_loss``, the engine keys and the flags of the three training scripts, the module surface, the input rule
of the golden fixture tests/golden/hardpixel_ref.pt (made by tests/golden/make_hardpixel_golden.py), and the float64 closed forms
of tests/hardpixel_ref.py against every loss and gradient the reference recorded there.

Tolerance of the last check.  The reference runs in float32; Y = |recorded - float64 closed form| is printed element by element
(as its maximum and its largest ratio to the bound) and must stay below bounds built from u = 2^-24 alone, derived in the
docstring of tests/hardpixel_ref.py and assembled here:
  topk          every selected v_i within |w| ce_bound (A = max |logit|); the float32 mean of K values adds (K + 2) u mean |v|:
                loss <= mean of the per-pixel bounds + (K + 2) u |loss|.  Gradient w (softmax - onehot) / K: a probability is
                E(D, C) ulps off, the difference, the weight and 1 / K round once each: |w| / K (E 2^-23 + 4 u) per element;
                exactly 0 outside the selected set (the gap rule makes the set the same in every precision).
  dc_and_topk   that plus dice_bound / the dice gradient bound, plus one rounding of the sum.
  focal         per pixel focal_bounds with dq = 0 (the recorded float32 probabilities ARE the input); the float32 mean / sum of
                N values adds (N + 2) u times the mean / sum of |v|.  Gradient c(pt) o_c / N (or without 1 / N): the bound of
                c times o_c, plus 3 u of the element for the two products and the factor."""
import ctypes
import importlib.util
import math
import os

import numpy as np
import pytest
import torch
from torch import nn

from adaptersis_amd import _lib, ops
from adaptersis_amd import train as T
from adaptersis_amd import train_mla as TMLA
from adaptersis_amd import train_multi_class as TMC
from adaptersis_amd.backbones.engines import SegEngine
from adaptersis_amd.segloss.ND_Crossentropy import CrossentropyND, TopKLoss
from adaptersis_amd.segloss.dice_loss import DC_and_topk_loss, SoftDiceLoss, softmax_helper
from adaptersis_amd.segloss.focal_loss import FocalLoss
from tests import hardpixel_ref as R
from tests.conftest import GOLDEN, load_golden

U = R.U


def test_scratch_and_tile_need_no_gpu():
    lib = _lib.lib()
    tile = lib.asis_hardpixel_tile()
    assert tile > 0 and tile % 64 == 0
    last = 0
    for N in (1, tile - 1, tile, tile + 1, 100 * tile + 5, 12 * 588 * 588):
        b = lib.asis_hardpixel_scratch_bytes(N)
        assert b >= last and b >= 4 * N + 12 * (-(-N // tile))   # the values, a count and a double per tile
        last = b
    assert lib.asis_hardpixel_scratch_bytes(1) < lib.asis_hardpixel_scratch_bytes(tile + 1) < last
    assert ops.hardpixel_scratch_bytes(12 * 588 * 588) == last and 16.5e6 < last < 16.8e6   # the figure of the docs: ~4 B a pixel
    assert last < ops.lovasz_scratch_bytes(12 * 588 * 588, 1) / 4
    for N in (0, -5, 1 << 31, 1 << 40):
        assert lib.asis_hardpixel_scratch_bytes(N) == -1 and b"2^31" in lib.asis_last_error()
        with pytest.raises(ValueError):
            ops.hardpixel_scratch_bytes(N)


def test_argument_errors_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(logits=p, target=p, weight=None, B=1, h=2, w=2, H=2, W=2, C=2, kind=0, n_softmax=0, gamma=2.0, smooth=1e-5, K=1,
             scratch=p, loss=p, dz=p):
        return lib.asis_hardpixel_loss(None, logits, target, weight, B, h, w, H, W, C, kind, n_softmax, gamma, smooth, K, 1, 1.0, 0,
                                       scratch, loss, dz, None, None)

    for kw, word in ((dict(logits=None), b"null"), (dict(target=None), b"null"), (dict(scratch=None), b"null"),
                     (dict(loss=None), b"null"), (dict(dz=None), b"null"), (dict(C=17), b"C=17"), (dict(C=0), b"C=0"),
                     (dict(K=0), b"K=0"), (dict(K=5), b"K=5"), (dict(K=-1), b"K=-1"), (dict(kind=2), b"kind"), (dict(kind=-1), b"kind"),
                     (dict(kind=1, n_softmax=2), b"n_softmax"), (dict(kind=0, n_softmax=1), b"n_softmax"),
                     (dict(kind=1, n_softmax=-1), b"n_softmax"), (dict(B=1 << 11, H=1 << 10, W=1 << 10), b"2^31"),
                     (dict(scratch=p + 4), b"aligned"), (dict(kind=1, C=1, smooth=1e-5), b"smooth"),
                     (dict(kind=1, smooth=1.5), b"smooth"), (dict(kind=1, smooth=-0.1), b"smooth"), (dict(B=0), b"empty")):
        assert call(**kw) == _lib.ASIS_EINVAL, kw
        assert word in lib.asis_last_error(), (kw, lib.asis_last_error())
    with pytest.raises(ValueError):
        _lib.check(call(C=17), "asis_hardpixel_loss")


def test_engine_keys_and_flags():
    assert ops.LOSS_TOPK == 6 and ops.LOSS_FOCAL == 7
    assert SegEngine.LOSSES["topk"] == (0, ops.LOSS_TOPK, 0.0, 0)
    assert SegEngine.LOSSES["dc_and_topk"] == (1, ops.LOSS_TOPK, 1.0, 0)       # SoftDice: n_region 1, smooth 1, no CE of its own
    assert SegEngine.LOSSES["focal"] == (1, ops.LOSS_FOCAL, 0.0, 0)
    for mod, default in ((T, "dice"), (TMLA, "dice"), (TMC, "iou")):
        p = mod.get_args_parser()
        d = p.parse_args([])
        assert d.loss == default and d.topk_percent == 10.0 and d.focal_gamma == 2.0
        for key in ("topk", "dc_and_topk", "focal"):
            assert p.parse_args(["--loss", key]).loss == key
        a = p.parse_args(["--loss", "dc_and_topk", "--topk_percent", "20", "--focal_gamma", "1.5"])
        assert a.topk_percent == 20.0 and a.focal_gamma == 1.5
        assert T._loss_args(a) == {"topk_percent": 20.0, "focal_gamma": 1.5}
        with pytest.raises(SystemExit):
            p.parse_args(["--loss", "hinge"])
    import inspect
    sig = inspect.signature(SegEngine.__init__).parameters
    assert sig["topk_percent"].default == 10.0 and sig["focal_gamma"].default == 2.0


def test_module_surface():
    t = TopKLoss()
    assert isinstance(t, CrossentropyND) and t.k == 10 and t.ignore_index == -100 and t.weight is None
    w = torch.ones(3)
    t = TopKLoss(w, -1, 25)
    assert t.weight is w and t.ignore_index == -1 and t.k == 25
    x, y = torch.zeros(1, 3, 4, 5), torch.zeros(1, 1, 4, 5, dtype=torch.int64)
    with pytest.raises(ValueError, match="selects none"):
        TopKLoss(k=1)(x, y)                                  # int(20 * 1 / 100) == 0: the reference's NaN
    with pytest.raises(NotImplementedError):
        TopKLoss(ignore_index=2)(x, y)
    with pytest.raises(NotImplementedError):
        TopKLoss()(torch.zeros(1, 3, 2, 4, 5), torch.zeros(1, 1, 2, 4, 5, dtype=torch.int64))
    with pytest.raises(_lib.AsisError):                      # no CPU fallback
        TopKLoss()(x, y)

    d = DC_and_topk_loss({}, {"k": 20})
    assert d.aggregate == "sum" and isinstance(d.ce, TopKLoss) and d.ce.k == 20
    assert isinstance(d.dc, SoftDiceLoss) and d.dc.apply_nonlin is softmax_helper and d.dc.smooth == 1.0
    assert DC_and_topk_loss({"smooth": 2.0}, {}).dc.smooth == 2.0
    with pytest.raises(NotImplementedError, match="nah son"):
        DC_and_topk_loss({}, {}, aggregate="mean")
    with pytest.raises(_lib.AsisError):
        d(x, y)

    f = FocalLoss()
    assert (f.apply_nonlin, f.alpha, f.gamma, f.balance_index, f.smooth, f.size_average) == (None, None, 2, 0, 1e-5, True)
    f = FocalLoss(softmax_helper, 0.25, 1.5, 1, 0.1, False)
    assert (f.apply_nonlin, f.alpha, f.gamma, f.balance_index, f.smooth, f.size_average) == (softmax_helper, 0.25, 1.5, 1, 0.1, False)
    assert FocalLoss(apply_nonlin=nn.Softmax(1))._n == 1 and FocalLoss()._n == 0
    with pytest.raises(NotImplementedError):
        FocalLoss(apply_nonlin=torch.sigmoid)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"smooth value should be in \[0,1\]"):
            FocalLoss(smooth=bad)
    assert FocalLoss(smooth=0).smooth == 0 and FocalLoss(smooth=None).smooth is None
    # the three alpha forms, as the [C] vector handed to the kernel
    assert FocalLoss().alpha_vector(3) is None
    assert torch.equal(FocalLoss(alpha=0.25, balance_index=1).alpha_vector(3), torch.tensor([0.75, 0.25, 0.75]))
    a = torch.tensor([1.0, 2.0, 5.0])
    assert torch.equal(FocalLoss(alpha=[1.0, 2.0, 5.0]).alpha_vector(3), a / a.sum())
    assert torch.equal(FocalLoss(alpha=np.array([1.0, 2.0, 5.0])).alpha_vector(3), a / a.sum())
    for C in (2, 3):
        for alpha in (None, 0.25, [float(i + 1) for i in range(C)]):
            got = FocalLoss(alpha=alpha, balance_index=1).alpha_vector(C)
            assert torch.equal(torch.ones(C) if got is None else got, R.alpha_vector(alpha, C, 1))
    q, lab = torch.full((1, 3, 4, 5), 1.0 / 3), torch.zeros(1, 4, 5, dtype=torch.int64)
    for bad in (1, "balanced", (1.0, 2.0, 3.0)):
        with pytest.raises(TypeError, match="Not support alpha type"):
            FocalLoss(alpha=bad)(q, lab)
    with pytest.raises(AssertionError):
        FocalLoss(alpha=[1.0, 2.0])(q, lab)
    with pytest.raises(_lib.AsisError):
        FocalLoss()(q, lab)
    with pytest.raises(_lib.AsisError):
        ops.hardpixel_loss(q.permute(0, 2, 3, 1).contiguous(), lab, ops.HARDPIXEL_FOCAL, 20)


def _generator():
    spec = importlib.util.spec_from_file_location("make_hardpixel_golden", os.path.join(GOLDEN, "make_hardpixel_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


def test_golden_input_rule():
    """the gap between the K-th and the (K+1)-th largest cross entropy is >= 1e-4 in float64 and in float32, the seed is the
    first such one, and the file holds what the generator's draw gives"""
    gen = _generator()
    cases = load_golden("hardpixel_ref")["cases"]
    assert [tuple(c["shape"]) for c in cases] == gen.SHAPES
    assert os.path.getsize(os.path.join(GOLDEN, "hardpixel_ref.pt")) < 200 * 1024
    for c in cases:
        B, h, w, C = c["shape"]
        N = B * h * w
        K = int(N * 10 / 100)
        assert c["K"] == K and K >= 1
        logits, target, weight = gen.draw(tuple(c["shape"]), c["seed"])
        assert torch.equal(logits, c["logits"]) and torch.equal(target, c["target"]) and torch.equal(weight, c["weight"])
        assert c["probs"].shape == (B, C, h, w)
        assert float((torch.softmax(logits.double().permute(0, 3, 1, 2), 1) - c["probs"]).abs().max()) < 1e-6
        for z in (logits, logits.double()):
            gap = gen.kth_gap(z, target, K)
            print(f"MEASURE gap {c['shape']} {z.dtype}: {gap:.3e}")
            assert gap >= gen.MIN_GAP
        assert c["seed"] == gen.find_seed(tuple(c["shape"]), c["seed"] + 1)
        for name in gen.CONFIGS:
            assert c["loss_" + name].shape == () and c["grad_" + name].shape == (B, C, h, w)
    assert [c["K"] for c in cases] == [24, 6, 51] and [c["seed"] for c in cases] == [0, 0, 0]


def _report(name, case, got, ref, bound):
    """prints max Y and max Y / bound over the elements, -> whether every element is within its bound"""
    got, ref, bound = (torch.as_tensor(x, dtype=torch.float64).reshape(-1) for x in (got, ref, bound))
    y = (got - ref).abs()
    ratio = torch.where(bound > 0, y / bound.clamp_min(1e-300), torch.where(y == 0, 0.0, math.inf).double())
    print(f"MEASURE {name} {case}: max Y {float(y.max()):.3e} max Y/bound {float(ratio.max()):.3f} at element {int(ratio.argmax())}")
    return float(ratio.max()) <= 1.0


@pytest.mark.parametrize("i", [0, 1, 2])
def test_closed_forms_reproduce_the_reference(i):
    gen = _generator()
    c = load_golden("hardpixel_ref")["cases"][i]
    B, h, w, C = c["shape"]
    N, K = B * h * w, c["K"]
    labels = c["target"].reshape(-1)
    z = c["logits"].double().reshape(-1, C)
    A = float(z.abs().max())
    D = float((z.max(-1).values - z.min(-1).values).max())
    Eq = R.softmax_ulps(D, C) * 2.0 ** -23
    ok = []

    def nchw(d):
        return d.view(B, h, w, C).permute(0, 3, 1, 2)

    dice, ddice, coef = R.soft_dice(c["logits"].double(), c["target"])
    dice_b, ddice_b = R.dice_bounds(c["logits"].double(), coef)
    for name, weight in (("topk", None), ("topk_w", c["weight"]), ("dc_and_topk", None)):
        v, dv, aux = R.pixel_values(z, labels, R.CE, weight=weight)
        sel = R.stable_topk(v, K)
        s = torch.sort(v, descending=True).values
        print(f"MEASURE gap.{name} {c['shape']}: {float(s[K - 1] - s[K]):.3e}")
        loss, dz = R.loss_and_dz(v, dv, sel, K)
        vb = aux["w"].abs() * R.ce_bound(A, C, aux["nll"])
        lb = float(vb[sel].mean()) + (K + 2) * U * abs(float(loss))
        gb = (aux["w"].abs() / K * (Eq + 4 * U)).view(-1, 1).expand(N, C) * sel.view(-1, 1)
        if name == "dc_and_topk":
            loss, dz = loss + dice, dz + ddice.reshape(-1, C)
            lb, gb = lb + dice_b + U * abs(float(loss)), gb + ddice_b.reshape(-1, C)
        else:
            assert bool((nchw(sel.view(-1, 1).expand(N, C)) == (c["grad_" + name] != 0)).all()), "the selected set"
        ok.append(_report(f"loss.{name}", c["shape"], c["loss_" + name], loss, lb))
        ok.append(_report(f"grad.{name}", c["shape"], c["grad_" + name], nchw(dz), nchw(gb)))

    q = c["probs"].double().permute(0, 2, 3, 1).reshape(-1, C)
    runs = (("focal", dict(gamma=2.0, smooth=1e-5, weight=None), True),
            ("focal_float", dict(gamma=gen.FOCAL_FLOAT["gamma"], smooth=1e-5,
                                 weight=R.alpha_vector(gen.FOCAL_FLOAT["alpha"], C, gen.FOCAL_FLOAT["balance_index"])), False),
            ("focal_list", dict(gamma=2.0, smooth=0.0, weight=R.alpha_vector(c["alpha_list"], C)), True))
    for name, kw, size_average in runs:
        v, dv, aux = R.pixel_values(q, labels, R.FOCAL, n_softmax=0, **kw)
        sel = torch.ones(N, dtype=torch.bool)
        loss, dz = R.loss_and_dz(v, dv, sel, N, size_average)
        f = 1.0 / N if size_average else 1.0
        vb, cb = R.focal_bounds(aux, kw["gamma"], kw["smooth"], C)
        lb = f * (float(vb.sum()) + (N + 2) * U * float(v.abs().sum()))
        gb = f * (cb.view(-1, 1) * aux["o"]) + 3 * U * dz.abs()
        ok.append(_report(f"loss.{name}", c["shape"], c["loss_" + name], loss, lb))
        ok.append(_report(f"grad.{name}", c["shape"], c["grad_" + name], nchw(dz), nchw(gb)))
    assert all(ok)
