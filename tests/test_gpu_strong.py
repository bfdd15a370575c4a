"""GPU: ``ops.strong_view`` (csrc/strongaug.hip) element by element against the float64 restatement tests/strong_ref.py, on the
smallest shapes at which the kernel can go wrong: S = 16 (radius 6 reflects at both borders inside one tile; 24 samples, one per
operation order), S = 37 (odd, no multiple of 4, one partial tile), S = 70 (several tiles per axis with partial edge tiles), a
non-square 20 x 45 and 20 x 44 (the 16-byte path beside the tail path).

The map is continuous (the clamps, the HSV round trip including its sector joins and grey, the periodic hue wrap), so every output
element is compared and none is excused.  The tolerance is not tuned on the kernel: it is 4 x the largest absolute difference
between the SAME restatement evaluated in float32 on the CPU and in float64, over all cases of this file (neither is the code under
test; the factor 4 is for the kernel's contracted multiply-adds and its own order of the 13-tap sums).
Measured 2026-10-21: 1.074e-06, hence TOL = 4.3e-06 (``test_the_tolerance_is_the_measured_one`` measures it again)."""
import itertools
import math

import pytest
import torch

from adaptersis_amd import _lib_strong, ops
from adaptersis_amd.tools import augment as A
from tests import strong_ref as R

gpu = pytest.mark.gpu

F32_VS_F64 = 1.074e-06         # measured 2026-10-21 (see the module docstring)
TOL = 4.0 * F32_VS_F64

ORDERS = list(itertools.permutations(range(4)))
SIGMA = {1: 0.3, 2: 0.6, 3: 0.9, 4: 1.2, 5: 1.6, 6: 2.0}


def _inputs(B, H, W, seed):
    """a mix of k/255 lattice values, uniform floats, exact 0 and 1, exactly grey pixels and pure-channel pixels"""
    g = torch.Generator().manual_seed(seed)
    kind = torch.randint(0, 6, (B, 1, H, W), generator=g)
    lattice = torch.randint(0, 256, (B, 3, H, W), generator=g).float() / 255.0
    uniform = torch.rand((B, 3, H, W), generator=g)
    binary = torch.randint(0, 2, (B, 3, H, W), generator=g).float()
    greys = (torch.randint(0, 256, (B, 1, H, W), generator=g).float() / 255.0).expand(B, 3, H, W)
    pure = torch.zeros((B, 3, H, W))
    pure.scatter_(1, torch.randint(0, 3, (B, 1, H, W), generator=g), torch.rand((B, 1, H, W), generator=g))
    x = torch.where(kind == 0, lattice, torch.where(kind == 1, uniform, torch.where(kind == 2, binary, torch.where(kind == 3, greys, pure))))
    x = torch.where(kind == 5, lattice.round(), x)      # a second helping of exact 0 and 1 next to lattice neighbours
    return x.contiguous()


def _cfg(order=None, factors=None, grey=False, r=0):
    if order is not None and factors is None:
        factors = tuple({0: 1.5, 1: 0.6, 2: 1.4, 3: -0.2}[o] for o in order)
    return {"strong": {"order": order, "factors": factors, "grey": grey, "sigma": SIGMA[r] if r else None}}


EVERYTHING = _cfg((3, 1, 0, 2), (0.17, 1.45, 0.55, 0.5), True, 6)
CONFIGS = [  # none, each single operation, grey alone, blur alone at r = 1 and r = 6, everything together, and pairs around contrast
    {"strong": None}, _cfg((0,), (1.5,)), _cfg((1,), (0.5,)), _cfg((2,), (1.5,)), _cfg((3,), (0.25,)), _cfg((3,), (-0.25,)),
    _cfg(grey=True), _cfg(r=1), _cfg(r=6), EVERYTHING, _cfg((0, 1), (1.5, 1.5)), _cfg((1, 0), (1.5, 1.5)), _cfg((2, 3, 1, 0), None, False, 3),
]


def _pad(c):
    st = c["strong"]
    if st is None or st["order"] is None:
        return c
    n = 4 - len(st["order"])
    return {"strong": {**st, "order": tuple(st["order"]) + (-1,) * n, "factors": tuple(st["factors"]) + (0.0,) * n}}


def _case(name):
    """-> (x on the CPU, the draws, apply)"""
    if name == "orders16":      # all 24 orders, one per sample; brightness 1.5 engages the clamps; every radius; grey on every fifth
        return _inputs(24, 16, 16, 1), [_cfg(o, None, k % 5 == 0, (0, 6, 1, 3)[k % 4]) for k, o in enumerate(ORDERS)], None
    if name == "configs37":
        return _inputs(len(CONFIGS), 37, 37, 2), CONFIGS, None
    if name == "masked37":      # an apply mask that switches half of them off
        return _inputs(len(CONFIGS), 37, 37, 3), CONFIGS, [b % 2 for b in range(len(CONFIGS))]
    if name == "tiles70":
        return _inputs(6, 70, 70, 4), [EVERYTHING, _cfg(r=6), _cfg((1, 3, 2, 0), None, False, 0), _cfg(r=2), {"strong": None},
                                        _cfg((0, 2, 1, 3), None, True, 5)], None
    if name == "rect20x45":
        return _inputs(5, 20, 45, 5), [EVERYTHING, _cfg((1,), (1.3,)), {"strong": None}, _cfg(r=4), _cfg((3, 0, 2, 1), None, True, 0)], None
    if name == "rect20x44":     # W % 4 == 0: the 16-byte path, edge tiles 12 wide
        return _inputs(5, 20, 44, 6), [EVERYTHING, _cfg((1,), (1.3,)), {"strong": None}, _cfg(r=4), _cfg((3, 0, 2, 1), None, True, 0)], None
    raise KeyError(name)


CASES = ("orders16", "configs37", "masked37", "tiles70", "rect20x45", "rect20x44")
_AUG = A.TrainAugment(size=16, strong={})
_REF = {}


def _reference(name):
    """the case with its float64 and float32 restatements, computed once and left unchanged"""
    if name not in _REF:
        x, cfgs, apply = _case(name)
        params = [_pad(c) for c in cfgs]
        host = _AUG.strong_tables(params, "cpu", apply)
        _REF[name] = dict(x=x, params=params, apply=apply, host=host, ref=R.strong_view(x, host, apply),
                          ref32=R.strong_view(x, host, apply, dtype=torch.float32))
    return _REF[name]


def test_the_tolerance_is_the_measured_one():
    """CPU: float32 against float64 of the restatement over all cases; the constant of this file is that figure (fp32 arithmetic
    is IEEE on every host; a library that orders the mean's sum differently moves it by a few per cent at most)"""
    worst = max(float((_reference(n)["ref32"].double() - _reference(n)["ref"]).abs().max()) for n in CASES)
    print(f"float32 vs float64 restatement: max |diff| = {worst:.3e}; TOL = {TOL:.3e}")
    assert 0.8 * F32_VS_F64 <= worst <= 1.25 * F32_VS_F64
    assert sorted({tuple(p["strong"]["order"]) for p in _reference("orders16")["params"]}) == ORDERS


@gpu
@pytest.mark.parametrize("name", CASES)
def test_every_element_against_float64(dev, name):
    c = _reference(name)
    x = c["x"].to(dev)
    kept = x.clone()
    tables = _AUG.strong_tables(c["params"], dev, c["apply"])
    assert tables["strong_any"] and tables["st_ops"].is_cuda
    out = ops.strong_view(x, tables)
    again = ops.strong_view(x, tables)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.data_ptr() != x.data_ptr()
    assert torch.equal(x, kept)                                                # out of place: the input is the teacher's view
    assert torch.equal(out, again)                                             # contrast samples included: no atomics
    assert float(out.min()) >= 0.0 and float(out.max()) <= 1.0
    err = (out.double().cpu() - c["ref"]).abs().flatten(1).max(1).values
    print(f"{name}: max |kernel - float64| per sample = {[f'{e:.2e}' for e in err.tolist()]}; TOL = {TOL:.2e}")
    assert float(err.max()) <= TOL, (name, err.tolist())
    for b, p in enumerate(c["params"]):                                        # no draw, or apply == 0: a copy of bits
        if p["strong"] is None or (c["apply"] is not None and not c["apply"][b]):
            assert torch.equal(out[b], x[b]), (name, b)
        else:
            assert not torch.equal(out[b], x[b]), (name, b)
    # the apply argument of the op is the tables' st_apply
    if c["apply"] is not None:
        plain = _AUG.strong_tables(c["params"], dev)
        assert torch.equal(ops.strong_view(x, plain, apply=c["apply"]), out)
        assert torch.equal(ops.strong_view(x, plain, apply=torch.tensor(c["apply"], device=dev, dtype=torch.int32)), out)
    buf = torch.full_like(x, -1.0)
    assert ops.strong_view(x, tables, out=buf) is buf and torch.equal(buf, out)


@gpu
def test_nothing_to_do_returns_the_input_and_opens_nothing(dev, monkeypatch):
    monkeypatch.setattr(_lib_strong, "_dlib", None)                            # as in a process that never opened the library
    x = _inputs(3, 16, 16, 9).to(dev)
    for params, apply in (([{"strong": None}] * 3, None), ([EVERYTHING, {"strong": None}, _cfg(r=1)], [0, 1, 0]), ([{}] * 3, None)):
        tables = _AUG.strong_tables([_pad(p) if "strong" in p else p for p in params], dev, apply)
        assert not tables["strong_any"] and ops.strong_view(x, tables) is x
    assert not _lib_strong.loaded()


@gpu
def test_the_contrast_mean(dev):
    """The grey sum of a contrast sample against float64.  With contrast first a summand is 0.2989 r + 0.587 g + 0.114 b in fp32:
    three coefficient roundings (together <= 2^-24 of the summand) and at most five arithmetic roundings of values <= 1; brightness
    in front adds one rounding per channel (weighted by the coefficients: <= 2^-24 together); the double sum adds nothing visible.
    So |sum - sum64| <= H W (1 + 5 + 1) 2^-24: H W fp32 roundings of the summands, a few times over — derived, not measured."""
    c = _reference("configs37")
    x = c["x"].to(dev)
    tables = _AUG.strong_tables(c["params"], dev)
    part = ops.strong_contrast_partials(x, tables)
    HW = 37 * 37
    assert part.dtype == torch.float64 and tuple(part.shape) == (len(CONFIGS), _lib_strong.lib().asis_strong_nblk(HW))
    assert torch.equal(part, ops.strong_contrast_partials(x, tables))
    checked = 0
    for b, p in enumerate(c["params"]):
        want = R.contrast_mean(c["x"], c["host"], b)
        total = 0.0
        for v in part[b].tolist():                                             # in index order, as the kernel's consumer adds them
            total += v
        if want is None:
            assert total == 0.0
            continue
        order = [o for o in p["strong"]["order"] if o >= 0]
        if order[0] == R.OP_CONTRAST or order[:2] == [R.OP_BRIGHTNESS, R.OP_CONTRAST]:
            assert abs(total - want * HW) <= HW * 7 * 2.0 ** -24, (b, total / HW, want)
            checked += 1
        assert abs(total / HW - want) <= TOL
    assert checked == 3
    # several workgroups per sample: 70 x 70 = 4900 pixels are two chunks
    c = _reference("tiles70")
    part = ops.strong_contrast_partials(c["x"].to(dev), _AUG.strong_tables(c["params"], dev))
    assert part.shape[1] == 2 and math.isclose(float(part[2].sum()) / 4900, R.contrast_mean(c["x"], c["host"], 2), abs_tol=7 * 2.0 ** -24)
    assert float(part[1].abs().sum()) == 0.0 and float(part[4].abs().sum()) == 0.0


@gpu
def test_the_sampler_calls_the_op(dev):
    """``TrainAugment.__call__`` with a strong configuration: the strong view of its own augmentation, the pre-strong tensor on
    request, and without a configuration exactly what it returned before"""
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (6, 32, 32, 3), generator=g, dtype=torch.uint8).to(dev)
    msk = torch.randint(0, 2, (6, 32, 32), generator=g, dtype=torch.uint8).to(dev)
    plain = A.TrainAugment(size=32, seed=4)(img, msk)
    aug = A.TrainAugment(size=32, seed=4, strong=dict(jitter_p=1.0))
    x, m, params, pre = aug(img, msk, return_params=True, return_strong=True)
    assert torch.equal(pre, plain[0]) and torch.equal(m, plain[1]) and len(A.TrainAugment(size=32, seed=4)(img, msk, return_strong=True)) == 3
    assert torch.equal(x, ops.strong_view(pre, aug.strong_tables(params, dev))) and not torch.equal(x, pre)
    assert torch.equal(aug(img, msk, params)[0], x) and torch.equal(aug(img, msk, A.weak_params(params), return_strong=True)[2],
                                                                    aug(img, msk, A.weak_params(params))[0])
    half = aug(img, msk, params, strong_apply=[1, 0, 1, 0, 1, 0])[0]
    assert torch.equal(half[1::2], pre[1::2]) and torch.equal(half[0::2], x[0::2])
