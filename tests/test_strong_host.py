"""CPU: the strong student view without a device — the draws of ``TrainAugment(strong=)`` and their tables, the float64 restatement
tests/strong_ref.py against itself and against scipy, the flags of the three training scripts, the library's symbols and the
argument checks of ``ops.strong_view``."""
import argparse
import ctypes
import itertools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from adaptersis_amd import _lib, _lib_strong, ops
from adaptersis_amd import train as T
from adaptersis_amd import train_mla, train_multi_class
from adaptersis_amd.tools import augment as A
from tests import strong_ref as R

BASE_KEYS = ("crop", "flip", "rotk", "nonrigid", "clahe", "alpha", "beta", "gamma")


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    return a == b


@pytest.fixture(scope="module")
def draws():
    return [p["strong"] for p in A.TrainAugment(size=64, seed=11, strong={}).draw(4000)]


# ---- draws ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, {"non_rigid_p": 0.7}])
def test_the_base_stream_does_not_depend_on_the_block(kw):
    plain, strong = A.TrainAugment(size=64, seed=5, **kw).draw(64), A.TrainAugment(size=64, seed=5, strong={}, **kw).draw(64)
    for p, q in zip(plain, strong):
        assert "strong" not in p and "strong" in q and set(p) == set(BASE_KEYS) and set(q) == set(BASE_KEYS) | {"strong"}
        assert all(_same(p[k], q[k]) for k in BASE_KEYS)
    assert A.TrainAugment(size=64, seed=5).strong is None and A.TrainAugment(size=64, seed=5).strong_rng is None
    again = A.TrainAugment(size=64, seed=5, strong={}, **kw).draw(64)
    assert all(_same(a["strong"], b["strong"]) for a, b in zip(strong, again))
    other = A.TrainAugment(size=64, seed=6, strong={}, **kw).draw(64)
    assert not all(_same(a["strong"], b["strong"]) for a, b in zip(strong, other))


def test_shares_orders_and_radii(draws):
    n = len(draws)
    for share, p in ((sum(d is not None and d["order"] is not None for d in draws) / n, 0.8),
                     (sum(d is not None and d["grey"] for d in draws) / n, 0.2),
                     (sum(d is not None and d["sigma"] is not None for d in draws) / n, 0.5)):
        assert abs(share - p) <= 4.0 * math.sqrt(p * (1.0 - p) / n), (share, p)
    # a sample without any of the three keeps its pixels: None
    assert abs(sum(d is None for d in draws) / n - 0.2 * 0.8 * 0.5) <= 4.0 * math.sqrt(0.08 * 0.92 / n)
    assert all(d["order"] is not None or d["grey"] or d["sigma"] is not None for d in draws if d is not None)
    orders = {d["order"] for d in draws if d is not None and d["order"] is not None}
    assert orders == set(itertools.permutations(range(4)))
    radii = set()
    for d in draws:
        if d is None:
            continue
        if d["order"] is not None:
            f = dict(zip(d["order"], d["factors"]))
            assert all(0.5 <= f[k] <= 1.5 for k in (A.ST_BRIGHTNESS, A.ST_CONTRAST, A.ST_SATURATION)) and -0.25 <= f[A.ST_HUE] <= 0.25
        if d["sigma"] is not None:
            assert 0.1 <= d["sigma"] <= 2.0
            r = A.strong_radius(d["sigma"])
            assert r == max(1, math.ceil(3.0 * d["sigma"])) <= 6
            radii.add(r)
    assert radii == {1, 2, 3, 4, 5, 6}
    assert A.strong_radius(5.0) == 6 and A.strong_radius(0.01) == 1


def test_constructor_arguments():
    d = A.TrainAugment(size=32, seed=0, strong=dict(jitter=(0.1, 0.0, 0.2, 0.05), jitter_p=1.0, grey_p=1.0, blur_p=1.0, sigma=(0.5, 0.5))).draw(50)
    for p in d:
        s = p["strong"]
        f = dict(zip(s["order"], s["factors"]))
        assert 0.9 <= f[0] <= 1.1 and f[1] == 1.0 and 0.8 <= f[2] <= 1.2 and -0.05 <= f[3] <= 0.05 and s["grey"] and s["sigma"] == 0.5
    assert all(p["strong"] is None for p in A.TrainAugment(size=32, strong=dict(jitter_p=0.0, grey_p=0.0, blur_p=0.0)).draw(20))
    for bad in (dict(jitter=(0.5, 0.5, 0.5)), dict(jitter=(0.5, 0.5, 0.5, 0.6)), dict(grey_p=1.5), dict(sigma=(0.0, 1.0)), dict(nope=1), 3):
        with pytest.raises(ValueError, match="strong"):
            A.TrainAugment(size=32, strong=bad)


def test_weak_params_strips_the_block():
    aug = A.TrainAugment(size=32, seed=2, strong=dict(jitter_p=1.0))
    params = aug.draw(6)
    weak = A.weak_params(params)
    assert all(p["strong"] is not None for p in params) and all(w["strong"] is None for w in weak)
    assert all(w["crop"] == p["crop"] and w["flip"] == p["flip"] and w["rotk"] == p["rotk"] for p, w in zip(params, weak))
    assert not aug.strong_tables(weak, "cpu")["strong_any"]


# ---- tables --------------------------------------------------------------------------------------------------------------------------
def test_tables(draws):
    aug = A.TrainAugment(size=64, seed=1, strong={})
    params = [{"strong": d} for d in draws[:200]] + [{}]
    B = len(params)
    t = aug.strong_tables(params, "cpu")
    want = {"st_ops": (torch.int32, (B, 4)), "st_fac": (torch.float32, (B, 4)), "st_flags": (torch.int32, (B, 2)),
            "st_gauss": (torch.float32, (B, 13)), "st_apply": (torch.int32, (B,))}
    for k, (dt, shape) in want.items():
        assert t[k].dtype == dt and tuple(t[k].shape) == shape and t[k].is_contiguous() and torch.equal(t[k], t["st_host"][k])
    assert t["strong_any"] is True and t["contrast_any"] is True and t["blur_any"] is True and bool((t["st_apply"] == 1).all())
    for b, p in enumerate(params):
        d = p.get("strong")
        ops_, fac, (g, r), w = t["st_ops"][b].tolist(), t["st_fac"][b], t["st_flags"][b].tolist(), t["st_gauss"][b].double().numpy()
        if d is None or d["order"] is None:
            assert ops_ == [-1] * 4
        else:
            assert tuple(ops_) == d["order"] and np.array_equal(fac.numpy(), np.asarray(d["factors"], np.float32))
        assert g == int(d is not None and d["grey"])
        if d is None or d["sigma"] is None:
            assert r == 0 and not w.any()
            continue
        assert r == A.strong_radius(d["sigma"]) and not w[:6 - r].any() and not w[7 + r:].any() and (w[6 - r:7 + r] > 0).all()
        assert np.array_equal(w, w[::-1])
        # normalised in float64, rounded to fp32: the sum is 1 within one fp32 rounding (half an ulp of a weight <= 2^-24) per tap
        assert abs(w.sum() - 1.0) <= (2 * r + 1) * 2.0 ** -24
        i = np.arange(-r, r + 1, dtype=np.float64)
        e = np.exp(-0.5 * i * i / d["sigma"] ** 2)
        assert np.array_equal(w[6 - r:7 + r], (e / e.sum()).astype(np.float32).astype(np.float64))
    # the host flags follow the draws and the apply mask
    only_grey = [{"strong": {"order": None, "factors": None, "grey": True, "sigma": None}}, {"strong": None}]
    t = aug.strong_tables(only_grey, "cpu")
    assert (t["strong_any"], t["contrast_any"], t["blur_any"]) == (True, False, False)
    t = aug.strong_tables(only_grey, "cpu", apply=[False, True])
    assert (t["strong_any"], t["contrast_any"], t["blur_any"]) == (False, False, False) and t["st_apply"].tolist() == [0, 1]
    no_contrast = [{"strong": {"order": (0, 2, 3, 1), "factors": (1.2, 0.7, 0.1, 0.8), "grey": False, "sigma": 1.0}}]
    assert aug.strong_tables(no_contrast, "cpu")["contrast_any"] is True
    assert aug.strong_tables(no_contrast, "cpu", apply=[0])["contrast_any"] is False
    with pytest.raises(ValueError, match="apply has 2 entries"):
        aug.strong_tables(no_contrast, "cpu", apply=[1, 1])


# ---- the restatement against itself and against scipy -----------------------------------------------------------------------------
def _image(seed=0, hw=(9, 11)):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((3, *hw), generator=g, dtype=torch.float64)
    x[:, 0, 0] = 0.4            # an exactly grey pixel
    x[:, 0, 1] = torch.tensor([1.0, 0.0, 0.0])
    x[:, 0, 2] = 0.0
    x[:, 0, 3] = 1.0
    return x


def test_identities():
    x = _image()
    for shift in (0.0, 1.0, -1.0):
        assert float((R.hue(x, shift) - x).abs().max()) <= 1e-12
    assert float((R.hue(R.hue(x, 0.2), -0.2) - x).abs().max()) <= 1e-12
    assert torch.equal(R.brightness(x, 1.0), x) and torch.equal(R.contrast(x, 1.0), x) and torch.equal(R.saturation(x, 1.0), x)
    gx = R.to_grey(x)                                                          # r == g == b exactly: max == min
    assert torch.equal(R.hue(gx, 0.13), gx)
    exact = torch.full((3, 4, 5), 0.37, dtype=torch.float64)
    assert torch.equal(R.hue(exact, 0.21), exact)
    # the published coefficients sum to 0.9999: grey(x) of a grey pixel is 0.9999 of it, and saturation moves it by that much
    assert float((R.saturation(exact, 1.4) - (1.4 * exact - 0.4 * 0.9999 * exact)).abs().max()) <= 1e-15
    # pure channels keep their value under a hue shift (v = max stays), and a shift of 1/3 turns red into green
    red = torch.zeros((3, 1, 1), dtype=torch.float64)
    red[0] = 1.0
    assert float((R.hue(red, 1.0 / 3.0) - torch.tensor([0.0, 1.0, 0.0]).view(3, 1, 1)).abs().max()) <= 1e-12
    assert torch.equal(R.to_grey(x)[0], R.grey(x)) and torch.equal(R.to_grey(x)[1], R.to_grey(x)[2])


def test_grey_pixels_are_fixed_points_of_hue_and_saturation():
    x = _image()
    for f in (-0.25, 0.1, 0.25):
        assert torch.equal(R.hue(x, f)[:, 0, 0], x[:, 0, 0]) and torch.equal(R.hue(x, f)[:, 0, 2], x[:, 0, 2])
        assert torch.equal(R.hue(x, f)[:, 0, 3], x[:, 0, 3])
    for f in (0.5, 1.5):   # grey(x) of a grey pixel is 0.9999 of it: torchvision's coefficients do not sum to 1
        assert float((R.saturation(x, f)[:, 0, 0] - x[:, 0, 0]).abs().max()) <= 0.5 * 1e-4 * 0.4 + 1e-15


def test_blur():
    import scipy.ndimage as ndi
    x = _image(3, (16, 23))
    for sigma in (0.1, 0.4, 1.0, 2.0):
        r = A.strong_radius(sigma)
        w = A.strong_gauss(sigma, r).astype(np.float64)[6 - r:7 + r]
        want = ndi.correlate1d(ndi.correlate1d(x.numpy(), w, axis=2, mode="mirror"), w, axis=1, mode="mirror")
        assert float(np.abs(R.blur(x, w, r).numpy() - want).max()) <= 1e-12
        i = np.arange(-r, r + 1, dtype=np.float64)
        w64 = np.exp(-0.5 * i * i / sigma ** 2)
        w64 /= w64.sum()
        const = torch.full((3, 16, 23), 0.625, dtype=torch.float64)
        assert float((R.blur(const, w64, r) - const).abs().max()) <= 1e-12
    assert r == 6 and float(np.abs(R.blur(x[:, :, :7], w, 6).numpy()
                                   - ndi.correlate1d(ndi.correlate1d(x[:, :, :7].numpy(), w, axis=2, mode="mirror"), w, axis=1,
                                                     mode="mirror")).max()) <= 1e-12
    assert R.reflect_index(5, 3).tolist() == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    with pytest.raises(ValueError, match="radius"):
        R.blur(x[:, :6], w, 6)


def test_contrast_uses_the_mean_after_the_preceding_operations():
    x = _image(5)
    first = R.jitter(x, (R.OP_BRIGHTNESS, R.OP_CONTRAST, -1, -1), (1.4, 0.6, 0.0, 0.0))
    last = R.jitter(x, (R.OP_CONTRAST, R.OP_BRIGHTNESS, -1, -1), (0.6, 1.4, 0.0, 0.0))
    bright = R.brightness(x, 1.4)
    assert torch.equal(first, R.contrast(bright, 0.6, R.grey(bright).mean()))
    assert torch.equal(last, R.brightness(R.contrast(x, 0.6, R.grey(x).mean()), 1.4))
    assert float((first - last).abs().max()) > 1e-2
    assert float(R.grey(bright).mean() - R.grey(x).mean()) > 1e-2
    t = {"st_ops": torch.tensor([[0, 1, -1, -1], [1, 0, -1, -1], [0, 2, 3, -1]], dtype=torch.int32),
         "st_fac": torch.tensor([[1.4, 0.6, 0, 0], [0.6, 1.4, 0, 0], [1.4, 1.0, 0.1, 0]], dtype=torch.float32)}
    xb = torch.stack([x, x, x])
    assert R.contrast_mean(xb, t, 0) == float(R.grey(R.brightness(x, float(np.float32(1.4)))).mean())
    assert R.contrast_mean(xb, t, 1) == float(R.grey(x).mean()) and R.contrast_mean(xb, t, 2) is None


def test_the_whole_view_follows_the_tables():
    x = torch.stack([_image(7, (16, 16)), _image(8, (16, 16))])
    w = A.strong_gauss(0.8, 3)
    t = {"st_ops": torch.tensor([[3, 1, 0, 2], [-1] * 4], dtype=torch.int32), "st_fac": torch.tensor([[0.1, 1.3, 0.8, 0.6], [0.0] * 4]),
         "st_flags": torch.tensor([[1, 3], [0, 0]], dtype=torch.int32), "st_gauss": torch.from_numpy(np.stack([w, np.zeros(13, np.float32)]))}
    out = R.strong_view(x, t)
    f = [float(v) for v in t["st_fac"][0]]
    want = R.saturation(R.brightness(R.contrast(R.hue(x[0], f[0]), f[1]), f[2]), f[3])
    want = R.blur(R.to_grey(want), w[3:10].astype(np.float64), 3).clamp(0, 1)
    assert torch.equal(out[0], want) and torch.equal(out[1], x[1]) and out.dtype == torch.float64
    assert torch.equal(R.strong_view(x, t, apply=[0, 1]), x)
    assert R.strong_view(x, t, dtype=torch.float32).dtype == torch.float32


# ---- flags -----------------------------------------------------------------------------------------------------------------------------
def _ns(**kw):
    return argparse.Namespace(arch="vit_large", **kw)


def test_check_strong_args():
    ok = T.check_strong_args
    assert ok(_ns()) is None and ok(_ns(aug_strong=False, aug_strong_on="all")) is None
    assert ok(_ns(aug_strong=True)) is None and ok(_ns(aug_strong=True, aug_strong_on="unlabelled", unlabelled_path="synthetic")) is None
    assert ok(_ns(aug_strong=True, aug_strong_jitter=[0.4, 0.4, 0.4, 0.1], aug_strong_grey=0.0, aug_strong_blur=1.0)) is None
    assert ok(_ns(aug_strong_jitter=[0.4] * 4)) == "--aug_strong_jitter needs --aug_strong"
    assert ok(_ns(aug_strong_grey=0.1)) == "--aug_strong_grey needs --aug_strong"
    assert ok(_ns(aug_strong_blur=0.1)) == "--aug_strong_blur needs --aug_strong"
    assert ok(_ns(aug_strong_on="unlabelled", unlabelled_path="synthetic")) == "--aug_strong_on needs --aug_strong"
    assert "hue in [0, 0.5]" in ok(_ns(aug_strong=True, aug_strong_jitter=[0.4, 0.4, 0.4, 0.6]))
    assert "hue in [0, 0.5]" in ok(_ns(aug_strong=True, aug_strong_jitter=[1.4, 0.4, 0.4, 0.1]))
    assert ok(_ns(aug_strong=True, aug_strong_grey=1.5)) == "--aug_strong_grey must be a probability in [0, 1]"
    assert ok(_ns(aug_strong=True, aug_strong_blur=-0.5)) == "--aug_strong_blur must be a probability in [0, 1]"
    assert ok(_ns(aug_strong=True, aug_strong_on="some")) == "--aug_strong_on must be all or unlabelled"
    assert ok(_ns(aug_strong=True, aug_strong_on="unlabelled")).startswith("--aug_strong_on unlabelled needs --unlabelled_path")
    assert T._strong_config(_ns()) is None and T._strong_config(_ns(aug_strong=True)) == {}
    assert T._strong_config(_ns(aug_strong=True, aug_strong_jitter=[0.4, 0.3, 0.2, 0.1], aug_strong_grey=0.0, aug_strong_blur=1.0)) == \
        {"jitter": (0.4, 0.3, 0.2, 0.1), "grey_p": 0.0, "blur_p": 1.0}


@pytest.mark.parametrize("mod", [T, train_mla, train_multi_class])
def test_the_parsers(mod):
    p = mod.get_args_parser()
    a = p.parse_args([])
    assert a.aug_strong is False and a.aug_strong_on == "all" and a.aug_strong_jitter is None and T._strong_config(a) is None
    a = p.parse_args(["--aug_strong", "--aug_strong_jitter", "0.4", "0.3", "0.2", "0.1", "--aug_strong_grey", "0.1", "--aug_strong_blur", "0.9"])
    assert T._strong_config(a) == {"jitter": (0.4, 0.3, 0.2, 0.1), "grey_p": 0.1, "blur_p": 0.9}
    A.TrainAugment(size=32, strong=T._strong_config(a))
    semi = ["--ema_decay", "0.9", "--distill_teacher", "ema", "--unlabelled_path", "synthetic"]
    assert p.parse_args(["--aug_strong", "--aug_strong_on", "unlabelled", *semi]).aug_strong_on == "unlabelled"
    for bad in (["--aug_strong", "--aug_strong_on", "unlabelled"], ["--aug_strong_grey", "0.1"], ["--aug_strong_on", "unlabelled", *semi],
                ["--aug_strong", "--aug_strong_jitter", "0.4", "0.3", "0.2"], ["--aug_strong", "--aug_strong_blur", "2"],
                ["--aug_strong", "--aug_strong_on", "labelled"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)


def test_train_seg_refuses_before_any_process_group():
    with pytest.raises(ValueError, match="--aug_strong_on unlabelled needs --unlabelled_path"):
        T.train_seg(_ns(aug_strong=True, aug_strong_on="unlabelled"))


# ---- library -------------------------------------------------------------------------------------------------------------------------
def test_library_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "asis_strong.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(asis_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib_strong.SIGNATURES) == ["asis_strong_chunk", "asis_strong_mean", "asis_strong_nblk", "asis_strong_view"]
    assert os.path.dirname(_lib_strong.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    side, main = ctypes.CDLL(_lib_strong.LIB_PATH), ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(side, n) and not hasattr(main, n) and n not in _lib.SIGNATURES
    nm = shutil.which("nm")
    if nm:   # the dynamic symbol table, where the tool is at hand: nothing else with the project's prefix is exported
        out = subprocess.run([nm, "-D", "--defined-only", _lib_strong.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert sorted(l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith("asis_")) == names
    # callable without a GPU
    assert side.asis_strong_chunk() == 4096
    side.asis_strong_nblk.argtypes = [ctypes.c_int64]
    assert side.asis_strong_nblk(588 * 588) == -(-588 * 588 // 4096) and side.asis_strong_nblk(1) == 1 and side.asis_strong_nblk(0) == -1


def test_build_lists_the_library():
    from adaptersis_amd import build
    assert build.SIDE_LIBS["libasis_strong.so"] == ("strongaug.hip",)
    assert not any(s.endswith("strongaug.hip") for s in build.sources()) and any(s.endswith("augment.hip") for s in build.sources())


# ---- ops.strong_view: argument errors without a GPU -------------------------------------------------------------------------------------
def _tables(B=2):
    return {"st_ops": torch.full((B, 4), -1, dtype=torch.int32), "st_fac": torch.zeros((B, 4)), "st_flags": torch.zeros((B, 2), dtype=torch.int32),
            "st_gauss": torch.zeros((B, 13))}


def test_strong_view_argument_errors():
    x = torch.rand(2, 3, 8, 10)
    t = _tables()
    assert ops.strong_view(x, t) is x                                          # nothing to do: nothing launched, nothing opened
    for bad in (x.double(), x[:, :, ::2], x[0], torch.rand(2, 4, 8, 10), "x"):
        with pytest.raises(ValueError, match=r"x must be a contiguous float32 tensor \[B,3,H,W\]"):
            ops.strong_view(bad, t)
    with pytest.raises(ValueError, match="tables must hold"):
        ops.strong_view(x, {k: v for k, v in t.items() if k != "st_gauss"})
    for name, bad in (("st_ops", t["st_ops"].long()), ("st_ops", t["st_ops"][:1]), ("st_fac", t["st_fac"].double()),
                      ("st_flags", torch.zeros((2, 3), dtype=torch.int32)), ("st_gauss", torch.zeros((2, 11))), ("st_gauss", None)):
        with pytest.raises(ValueError, match=name):
            ops.strong_view(x, {**t, name: bad})
    for code in (4, -2):
        bad = _tables()
        bad["st_ops"][1, 2] = code
        with pytest.raises(ValueError, match="operation codes must lie in -1..3"):
            ops.strong_view(x, bad)
    bad = _tables()
    bad["st_ops"][0, :2] = 1
    with pytest.raises(ValueError, match="contrast operation once"):
        ops.strong_view(x, bad)
    for r in (-1, 7, 8):
        bad = _tables()
        bad["st_flags"][0, 1] = r
        with pytest.raises(ValueError, match="blur radius must lie in 0..6 and below"):
            ops.strong_view(x, bad)
    bad = _tables()
    bad["st_flags"][0, 1] = 6
    with pytest.raises(ValueError, match=r"below min\(H, W\) = 6"):
        ops.strong_view(torch.rand(2, 3, 6, 10), bad)
    todo = _tables()
    todo["st_flags"][1, 0] = 1
    with pytest.raises(ValueError, match="apply must hold B=2"):
        ops.strong_view(x, todo, apply=[1, 0, 1])
    with pytest.raises(ValueError, match="out must not alias x"):
        ops.strong_view(x, todo, out=x)
    with pytest.raises(ValueError, match="out must be a contiguous float32"):
        ops.strong_view(x, todo, out=torch.empty(2, 3, 8, 9))
    assert ops.strong_view(x, todo, apply=[1, 0]) is x                         # the only sample with a draw is switched off
    with pytest.raises(_lib.AsisError, match="no CPU fallback"):              # and a real request needs the device
        ops.strong_view(x, todo)
