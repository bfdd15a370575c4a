"""GPU: the non-rigid augmentation block (csrc/nonrigid.hip) against the numpy / float64 restatement tests/nonrigid_ref.py:
noise and remap bit for bit, the blurred field within the fp32 dot-product bound, the Q5 maps within one unit, the whole
pipeline bit for bit, and the training script with the switch on.  Sizes: 20 (smaller than the Gauss radius 24: the window
reflects more than once), 64, 100 (no multiple of the 64 x 16 map tile; grid table with an empty last segment) and one B = 2
case at the reference's 588 (three row-pass segments, the last one partial)."""
import functools

import numpy as np
import pytest
import torch

from adaptersis_amd import ops
from adaptersis_amd.tools import augment as A
from oracle import augment_ref as O
from tests import nonrigid_ref as R

pytestmark = pytest.mark.gpu

ALPHA, SIGMA = 120.0, 6.0
SIZES = [20, 64, 100, 588]


def _data(B, S, seed=0):
    r = np.random.RandomState(seed)
    img = r.randint(0, 256, (B, S, S, 3)).astype(np.uint8)
    img[:, ::2] = (img[:, ::2].astype(np.int32) // 2 + 60).astype(np.uint8)      # smooth-ish rows: interpolation matters
    mask = r.randint(0, 5, (B, S, S)).astype(np.uint8)
    return img, mask


def _samples(S):
    """One sample of each kind plus none (B = 4); at 588 an elastic and an optical one (B = 2)."""
    r = np.random.RandomState(1000 + S)
    el = {"kind": "elastic", "seed": 0x9E3779B97F4A7C15 ^ (S << 40), "pts": r.uniform(-3.6, 3.6, (3, 2))}
    gr = {"kind": "grid", "xsteps": 1.0 + r.uniform(-0.3, 0.3, 6), "ysteps": 1.0 + r.uniform(-0.3, 0.3, 6)}
    op = {"kind": "optical", "k": 2.0, "dx": 0, "dy": 0}
    nrs = [el, op] if S == 588 else [el, gr, op, None]
    return [{"nonrigid": nr} for nr in nrs]


def _map64(S, nr):
    if nr is None:
        return None
    if nr["kind"] == "elastic":
        return R.elastic_map64(S, R.field64(nr["seed"], S, ALPHA, SIGMA), R.elastic_affine(S, nr["pts"]))
    if nr["kind"] == "grid":
        return R.grid_map64(S, 5, nr["xsteps"], nr["ysteps"])
    return R.optical_map64(S, nr["k"], nr["dx"], nr["dy"])


@functools.lru_cache(maxsize=None)
def _case(S):
    """The float64 references of one size, computed once and shared (read-only) by the tests."""
    params = _samples(S)
    q = [R.identity_map(S) if p["nonrigid"] is None else R.quantise(*_map64(S, p["nonrigid"])) for p in params]
    for a in q:
        a.setflags(write=False)
    return params, q


def _device_maps(S, dev, return_field=False):
    params, _ = _case(S)
    aug = A.TrainAugment(size=S, elastic=(ALPHA, SIGMA, 3.6))
    return ops.nonrigid_map(aug.nonrigid_tables(params, dev), S, return_field=return_field)


@pytest.mark.parametrize("S", SIZES)
def test_noise_bit_exact(dev, S):
    """One-tap Gauss table [1.0] and alpha = 1: the exported field IS the counter-based noise."""
    params, _ = _case(S)
    aug = A.TrainAugment(size=S, elastic=(1.0, SIGMA, 3.6))
    t = aug.nonrigid_tables(params, dev)
    t["nr_gauss"] = torch.ones(1, device=dev)
    _, field = ops.nonrigid_map(t, S, return_field=True)
    field = field.cpu().numpy()
    want = R.noise(params[0]["nonrigid"]["seed"], S)
    assert np.array_equal(field[0].astype(np.float64), want)
    assert not field[1:].any()                                       # samples of another kind: untouched (zero)


@pytest.mark.parametrize("S", SIZES)
def test_field_within_the_fp32_bound(dev, S):
    """|field - alpha gaussian_filter64(noise)| <= alpha 2 (2 r + 3) 2^-24: two fp32 dot products of 2 r + 1 terms, |x| <= 1,
    sum w = 1 (7.3e-4 px at alpha 120, r 24)."""
    params, _ = _case(S)
    _, field = _device_maps(S, dev, return_field=True)
    r = int(4 * SIGMA + 0.5)
    want = R.field64(params[0]["nonrigid"]["seed"], S, ALPHA, SIGMA)
    err = float(np.abs(field[0].cpu().numpy().astype(np.float64) - want).max())
    bound = ALPHA * 2 * (2 * r + 3) * 2.0 ** -24
    print(f"S={S}: max |field - ref| = {err:.3e} px (bound {bound:.3e}), max |field| = {np.abs(want).max():.2f} px")
    assert np.abs(want).max() > 1.0                                  # a field worth the name
    assert err <= bound


@pytest.mark.parametrize("S", SIZES)
def test_maps_within_one_unit(dev, S):
    """|q - rint(32 map64)| <= 1 unit of 1/32 px for every kind at every pixel; kind none is exactly 32 (x, y)."""
    params, want = _case(S)
    got = _device_maps(S, dev).cpu().numpy().astype(np.int64)
    assert got.shape == (len(params), S, S, 2)
    for b, p in enumerate(params):
        d = np.abs(got[b] - want[b])
        kind = "none" if p["nonrigid"] is None else p["nonrigid"]["kind"]
        print(f"S={S} {kind}: max |dq| = {int(d.max())}, pixels off by one: {float((d.max(-1) > 0).mean()):.5f}")
        if p["nonrigid"] is None:
            assert np.array_equal(got[b], R.identity_map(S))
        else:
            assert d.max() <= 1, (kind, int(d.max()))
            assert not np.array_equal(want[b], R.identity_map(S))


@pytest.mark.parametrize("S", [20, 64, 100])
def test_optical_maps(dev, S):
    """k = 2, -2 (coordinates reach about -0.75 S .. 1.75 S: far outside the frame) and 0.37 with a shift."""
    nrs = [{"kind": "optical", "k": 2.0, "dx": 0, "dy": 0}, {"kind": "optical", "k": -2.0, "dx": 0, "dy": 0},
           {"kind": "optical", "k": 0.37, "dx": 1, "dy": -1}]
    aug = A.TrainAugment(size=S)
    got = ops.nonrigid_map(aug.nonrigid_tables([{"nonrigid": nr} for nr in nrs], dev), S).cpu().numpy().astype(np.int64)
    for b, nr in enumerate(nrs):
        want = R.quantise(*R.optical_map64(S, nr["k"], nr["dx"], nr["dy"]))
        d = np.abs(got[b] - want)
        print(f"S={S} k={nr['k']}: max |dq| = {int(d.max())}, range {want.min() / 32 / S:.2f} S .. {want.max() / 32 / S:.2f} S")
        assert d.max() <= 1
    assert got[0].max() > 32 * 1.5 * S and got[0].min() < -32 * 0.5 * S


def _check_remap(dev, img, mask, q):
    """Device remap of every sample through ``q`` (integer [B,S,S,2]) == the integer restatement, bit for bit."""
    out, mo = ops.nonrigid_remap(torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev),
                                 torch.from_numpy(q.astype(np.int32)).to(dev))
    out, mo = out.cpu().numpy(), mo.cpu().numpy()
    assert out.dtype == np.uint8 and mo.dtype == np.int64
    for b in range(img.shape[0]):
        ro, rm = R.remap(img[b], mask[b], q[b])
        assert np.array_equal(out[b], ro), (b, int(np.abs(out[b].astype(int) - ro.astype(int)).max()))
        assert np.array_equal(mo[b], rm), b
    return out, mo


@pytest.mark.parametrize("S", SIZES)
def test_remap_through_the_device_map_bit_exact(dev, S):
    params, _ = _case(S)
    img, mask = _data(len(params), S, seed=S)
    mask = mask.astype(np.int64)
    mask[:, 1, 1] = (1 << 40) + 3                                    # the mask is copied as 64-bit values
    q = _device_maps(S, dev).cpu().numpy().astype(np.int64)
    out, mo = _check_remap(dev, img, mask, q)
    if S != 588:                                                     # sample 3 has kind none: the identity map reproduces both
        assert np.array_equal(out[3], img[3]) and np.array_equal(mo[3], mask[3])


@pytest.mark.parametrize("S", [2, 20, 100])
def test_remap_through_a_hand_made_map_bit_exact(dev, S):
    """Negative, far-out-of-range (the int32 ends included) and fx = 0 / 31 entries; S = 2 is the shortest reflection period."""
    r = np.random.RandomState(S)
    img, mask = _data(2, S, seed=S + 7)
    q = np.empty((2, S, S, 2), np.int64)
    q[0] = r.randint(-40 * 32 * S, 40 * 32 * S, (S, S, 2))          # many periods either side
    q[1] = R.identity_map(S) + r.randint(-70, 70, (S, S, 2))        # sub-pixel shifts around every pixel, borders included
    edge = [-(1 << 31), (1 << 31) - 1, (1 << 31) - 17, -1, -31, -32, -33, -16, -17, 0, 15, 16, 31, 32, 32 * (S - 1), 32 * (S - 1) + 31,
            32 * (S - 1) + 15, 32 * (S - 1) + 16, 32 * S, 32 * (2 * S - 2), 32 * (2 * S - 2) - 1, (1 << 30) + 31, -(1 << 30)]
    flat = q[0].reshape(-1, 2)
    n = min(len(edge), S * S // 2)
    flat[:n, 0], flat[n:2 * n, 1] = edge[:n], edge[:n]
    if S * S >= 2 * len(edge) + 4:
        flat[2 * n:2 * n + 4] = [[31, 0], [0, 31], [31, 31], [-(1 << 31), (1 << 31) - 1]]
    _check_remap(dev, img, mask.astype(np.int64), q)


def _post(p):
    return {"crop": None, "flip": False, "rotk": 0, "clahe": p.get("clahe"), "alpha": p["alpha"], "beta": p["beta"], "gamma": p["gamma"]}


def _geo(p):
    return {"crop": p["crop"], "flip": p["flip"], "rotk": p["rotk"], "alpha": 1.0, "beta": 0.0, "gamma": None}


@pytest.mark.parametrize("S", [20, 64, 100])
def test_pipeline_bit_exact(dev, S):
    """crop + flip + rot90 (oracle) -> non-rigid remap through the device's map (restatement) -> CLAHE / tables / 255 (oracle)
    == TrainAugment.__call__, bit for bit."""
    img, mask = _data(4, S, seed=S + 3)
    nr = [p["nonrigid"] for p in _samples(S)]
    base = dict(alpha=1.0, beta=0.0, gamma=None, clahe=None)
    params = [dict(base, crop=(3, 5, S - 9, S - 9), flip=True, rotk=1, clahe=3.7, nonrigid=nr[0]),
              dict(base, crop=None, flip=False, rotk=3, alpha=1.17, beta=-0.11, gamma=0.83, nonrigid=nr[1]),
              dict(base, crop=(0, 0, S // 2, S // 2), flip=True, rotk=2, clahe=1.0, gamma=1.19, nonrigid=dict(nr[2], k=-1.3)),
              dict(base, crop=(S // 2, S // 2 - 1, S // 2, S // 2), flip=True, rotk=0, clahe=2.0, nonrigid=None)]
    aug = A.TrainAugment(size=S, seed=4)
    t = aug.tables(params, dev)
    assert t["nonrigid_any"]
    out, mout = aug(torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev), params)
    q = ops.nonrigid_map(t, S).cpu().numpy()
    assert out.dtype == torch.float32 and tuple(out.shape) == (4, 3, S, S) and mout.dtype == torch.int64
    for b, p in enumerate(params):
        g, gm = O.apply(img[b], mask[b], _geo(p), S)
        g8 = np.ascontiguousarray(np.rint(g * np.float32(255)).astype(np.uint8).transpose(1, 2, 0))
        assert np.array_equal(g8.transpose(2, 0, 1).astype(np.float32) / np.float32(255), g)
        w8, wm = R.remap(g8, gm, q[b])
        ro, rm = O.apply(w8, wm, _post(p), S)
        assert np.array_equal(out[b].cpu().numpy(), ro), (b, float(np.abs(out[b].cpu().numpy() - ro).max()) * 255)
        assert np.array_equal(mout[b].cpu().numpy(), rm), b
        if p["nonrigid"] is not None:
            assert not np.array_equal(w8, g8)                        # the warp did something


def test_all_none_equals_the_pipeline_without_the_key(dev):
    S = 64
    img, mask = _data(3, S, seed=9)
    aug = A.TrainAugment(size=S, seed=5)
    params = aug.draw(3)
    params[0].update(clahe=2.5)
    params[1].update(clahe=None, crop=(3, 5, S - 9, S - 9))
    without = [{k: v for k, v in p.items() if k != "nonrigid"} for p in params]
    x, m = torch.from_numpy(img).to(dev), torch.from_numpy(mask).to(dev)
    a, am = aug(x, m, without)
    b, bm = aug(x, m, [dict(p, nonrigid=None) for p in without])
    assert not aug.tables(params, dev)["nonrigid_any"]
    assert torch.equal(a, b) and torch.equal(am, bm)
    t = aug.tables(without, dev)                                     # and through the non-rigid launches with every kind none
    t.update(aug.nonrigid_tables(without, dev))
    t["nonrigid_any"] = True
    c, cm = ops.augment(x, m, t)
    assert torch.equal(a, c) and torch.equal(am, cm)


def test_train_seg_with_aug_non_rigid(dev, tmp_path, monkeypatch):
    """`--aug_non_rigid 0.8` through the drop-in script on a PNG folder: the non-rigid launches run on the training batches
    only, the loss is finite."""
    from PIL import Image
    from adaptersis_amd import train as T
    r = np.random.RandomState(0)
    for split, n in (("training", 8), ("validation", 4)):
        (tmp_path / "data" / "images" / split).mkdir(parents=True)
        (tmp_path / "data" / "annotations" / split).mkdir(parents=True)
        for i in range(n):
            img = (r.randint(0, 256, (56, 56, 3)).astype(np.uint8)).repeat(4, 0).repeat(4, 1)
            msk = ((r.random_sample((56, 56)) > 0.7).astype(np.uint8) * 255).repeat(4, 0).repeat(4, 1)
            Image.fromarray(img).save(tmp_path / "data" / "images" / split / f"f{i:03d}.png")
            Image.fromarray(msk).save(tmp_path / "data" / "annotations" / split / f"f{i:03d}.png")
    args = T.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4", "--epochs", "1",
                                           "--lr", "0.05", "--data_path", str(tmp_path / "data"), "--num_workers", "0",
                                           "--output_dir", str(tmp_path / "out"), "--aug_non_rigid", "0.8"])
    assert T.get_args_parser().parse_args([]).aug_non_rigid == 0.0
    calls = []
    real = ops.nonrigid_remap
    monkeypatch.setattr(ops, "nonrigid_remap", lambda *a: (calls.append(a[0].shape[0]), real(*a))[1])
    T._ENGINES.clear()
    T._AUGMENTERS.clear()
    try:
        stats = T.train_seg(args)
        assert T._AUGMENTERS[224].non_rigid_p == 0.8
        assert 1 <= len(calls) <= 2                                  # two training batches (P(no sample drawn) = 0.2^4 each); never validation
        assert np.isfinite(stats["train_loss"]) and np.isfinite(stats["test_loss"]) and 0.0 <= stats["test_acc1"] <= 1.0
    finally:
        T._ENGINES.clear()
        T._AUGMENTERS.clear()
