"""GPU: percentile Hausdorff — the order statistics ``ops.surface_stats(..., percentiles=...)`` selects on the device
(``asis_surface_quantiles``, csrc/surface.hip) against the scipy oracle (tests/surface_ref.py): the squared distances at the other
side's edge pixels, sorted on the host and indexed with exact ranks, integer for integer; crafted rows that put chosen keys into
every digit of the select; then ``predict --masks --surface --hd_percentile`` and ``adaptersis_amd.score`` on a small PNG tree."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from adaptersis_amd import ops
from adaptersis_amd.segloss.surface import SurfaceMeter, metrics_from_stats, percentile_from_order, surface_ranks
from adaptersis_amd.tools import frame_resize as FR

from . import surface_ref as R
from .test_gpu_surface import make_case

pytestmark = pytest.mark.gpu

NONE = 255      # a raw value that the identity table maps to no class
PCTS = ([0, 50, 95, 100], [99.5])


def qs_of(pcts):
    return [int(round(100 * p)) for p in pcts]


def order_stats(values, qs):
    """int64 [P, 2]: (v[lo], v[hi]) of a multiset, from the fully sorted list and exact ranks."""
    v = np.sort(np.asarray(values, dtype=np.int64))
    return np.array([[v[surface_ranks(len(v), q)[0]], v[surface_ranks(len(v), q)[1]]] for q in qs], dtype=np.int64)


def expected_ord(pred, tgt, C, pct_lists, pred_lut=None, lut=None):
    """-> (ints of the oracle, [ord int64 [B, C, P, 3, 2] per list of percentiles]); one pass of the oracle for all lists."""
    ints, _, d2p, d2g = R.stats(pred, tgt, C, [], pred_lut=pred_lut, lut=lut, want_d2=True)
    ident = np.arange(256, dtype=np.uint8)
    p = np.asarray(ident if pred_lut is None else pred_lut, dtype=np.uint8)[pred]
    g = np.asarray(ident if lut is None else lut, dtype=np.uint8)[tgt]
    outs = [np.full((pred.shape[0], C, len(pl), 3, 2), -1, dtype=np.int64) for pl in pct_lists]
    for b in range(pred.shape[0]):
        for c in range(C):
            if (b, c) not in d2p or (b, c) not in d2g:
                continue                                            # absent on a side: no value
            at_p = d2g[b, c][R.edges_of(p[b] == c)]                 # d2_G over E(P)
            at_g = d2p[b, c][R.edges_of(g[b] == c)]                 # d2_P over E(G)
            assert len(at_p) == ints[b, c, 3] and len(at_g) == ints[b, c, 4]
            for out, pl in zip(outs, pct_lists):
                for k, v in enumerate((at_p, at_g, np.concatenate([at_p, at_g]))):
                    out[b, c, :, k] = order_stats(v, qs_of(pl))
    return ints, outs


def device_ord(dev, pred, tgt, C, pcts, **kw):
    out = ops.surface_stats(torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev), C, [], percentiles=pcts, **kw)
    assert len(out) == 3 and out[2].dtype == torch.int64 and tuple(out[2].shape) == (pred.shape[0], C, len(pcts), 3, 2)
    return out[0].cpu().numpy(), out[2].cpu().numpy()


def same_ord(got, want, label):
    assert np.array_equal(got, want), (f"{label}: ord differs at (frame, class, percentile, set, lo/hi) "
                                       f"{np.argwhere(got != want)[:8].tolist()}: got {got[got != want][:8].tolist()}, "
                                       f"expected {want[got != want][:8].tolist()}")


# ---- 1. random maps: exact order statistics, and the invariants at q = 0 and q = 100 ------------------------------------------------
SHAPES = [(1, 1), (1, 7), (5, 300), (33, 257), (64, 513)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 2, 8, 16])
@pytest.mark.parametrize("hw", SHAPES)
def test_order_statistics_against_the_oracle(dev, hw, C, B):
    for k, kind in enumerate(("blobs", "lines", "checker", "oneside")):
        pred, tgt = make_case(kind, B, hw[0], hw[1], C, seed=hw[0] * 17 + hw[1] * 5 + C * 3 + B + k)
        want_i, wants = expected_ord(pred, tgt, C, PCTS)
        for pcts, want in zip(PCTS, wants):
            label = f"{kind} {hw} C={C} B={B} {pcts}"
            gi, go = device_ord(dev, pred, tgt, C, pcts)
            assert np.array_equal(gi, want_i), label
            same_ord(go, want, label)
            if pcts != PCTS[0]:
                continue
            matched = (want_i[:, :, 3] > 0) & (want_i[:, :, 4] > 0)
            assert ((go >= 0).all(axis=(2, 3, 4)) == matched).all() and ((go == -1).all(axis=(2, 3, 4)) == ~matched).all(), label
            mx = np.stack([gi[:, :, 5], gi[:, :, 6], np.maximum(gi[:, :, 5], gi[:, :, 6])], axis=-1)      # [B, C, set]
            for b, c in np.argwhere(matched):
                assert (go[b, c, 3] == mx[b, c][:, None]).all(), f"{label}: q = 100 is the maximum of every set"
                assert (go[b, c, 0, :, 0] == go[b, c, 0, :, 1]).all() and go[b, c, 0, 2, 0] == go[b, c, 0, :2, 0].min()
            for b in range(B):                                          # through the metrics: q = 100 is hd, for both conventions
                for m in metrics_from_stats(gi[b], np.zeros((C, 2)), [], go[b], pcts):
                    if m is not None and not m["unmatched"]:
                        assert m["hd_pct"][3] == m["hd"] == m["hd_pct_sym"][3] and m["hd_pct"][0] <= m["hd_pct"][1] <= m["hd_pct"][2]


def test_far_apart_many_tiles(dev):
    """Half a million pixels (many tiles of the select passes), the two boundaries in opposite corners: keys above 2^16, and the
    background between them with keys from 0 up."""
    H, W = 540, 960
    yy, xx = np.mgrid[0:H, 0:W]
    pred = np.zeros((2, H, W), dtype=np.uint8)
    tgt = np.zeros((2, H, W), dtype=np.uint8)
    for b in range(2):
        pred[b][(yy - 60) ** 2 + (xx - 80 - 9 * b) ** 2 <= 50 ** 2] = 1
        tgt[b][((yy - 470) / 40) ** 2 + ((xx - 850) / 70) ** 2 <= 1.0] = 1
    want_i, wants = expected_ord(pred, tgt, 2, PCTS)
    assert want_i[0, 1, 5] > 1 << 16 and (wants[0][:, 1, 0] > 1 << 16).all() and (wants[0][:, 0, 0] == 0).all()
    for pcts, want in zip(PCTS, wants):
        gi, go = device_ord(dev, pred, tgt, 2, pcts)
        assert np.array_equal(gi, want_i)
        same_ord(go, want, f"far apart {pcts}")


# ---- 2. crafted rows: chosen keys ---------------------------------------------------------------------------------------------------
def row_case(W, S, L=(0,)):
    """H = 1: class 1 predicted at the columns S and labelled at the columns L (every mask pixel is an edge pixel).
    -> pred, tgt [1, 1, W] and the three distance multisets."""
    pred = np.full((1, 1, W), NONE, dtype=np.uint8)
    tgt = np.full((1, 1, W), NONE, dtype=np.uint8)
    pred[0, 0, list(S)] = 1
    tgt[0, 0, list(L)] = 1
    at_p = [min((x - l) ** 2 for l in L) for x in S]
    at_g = [min((x - l) ** 2 for x in S) for l in L]
    return pred, tgt, (at_p, at_g, at_p + at_g)


ROWS = {
    "single pixel": (64, [37], [0, 1, 50, 95, 99.5, 100]),                       # n = 1 for every q
    "two pixels, interpolated": (64, [3, 10], [50]),                             # rem = 5000
    "lowest digit": (64, [16, 17], [50]),                                        # 256 and 289: the same upper three digits
    "highest digit": (4100, [1, 4096], [50]),                                    # 1 and 2^24
    "every digit": (16384, [15, 16, 255, 256, 4095, 4096, 16383], [0, 50, 95, 100, 99.5, 16.67, 33.33, 66.67, 83.33, 16.66,
                                                                   83.34, 0.01]),
    "dense row": (16384, list(range(1, 16384)), [0, 50, 95, 100, 99.5, 99.99, 25]),
}


@pytest.mark.parametrize("name", sorted(ROWS))
def test_crafted_rows(dev, name):
    W, S, pcts = ROWS[name]
    pred, tgt, sets = row_case(W, S)
    assert sets[0] == [x * x for x in S]
    for i in range(0, len(pcts), 4):
        pl = pcts[i:i + 4]
        want = np.full((1, 2, len(pl), 3, 2), -1, dtype=np.int64)
        for k, v in enumerate(sets):
            want[0, 1, :, k] = order_stats(v, qs_of(pl))
        _, got = device_ord(dev, pred, tgt, 2, pl)
        same_ord(got, want, f"{name} {pl}")
    if name == "two pixels, interpolated":
        assert got[0, 1, 0, 0].tolist() == [9, 100] and surface_ranks(2, 5000) == (0, 1, 5000)
        assert percentile_from_order(9, 100, 5000) == 6.5
    if name == "highest digit":
        assert got[0, 1, 0, 0].tolist() == [1, 1 << 24]
    if name == "every digit":
        keys = sorted(x * x for x in S)
        assert keys[0] < 1 << 8 <= keys[1] and keys[2] < 1 << 16 <= keys[3] and keys[4] < 1 << 24 <= keys[5] < keys[6]


def test_all_keys_tie(dev):
    """200 predicted pixels, each at distance 2 from two label pixels: every key of every set is 4."""
    pred = np.full((1, 200, 5), NONE, dtype=np.uint8)
    tgt = np.full((1, 200, 5), NONE, dtype=np.uint8)
    pred[0, :, 2] = 1
    tgt[0, :, 0] = tgt[0, :, 4] = 1
    gi, got = device_ord(dev, pred, tgt, 2, [0, 50, 95, 100])
    assert gi[0, 1, 3:7].tolist() == [200, 400, 4, 4]
    assert (got[0, 1] == 4).all() and (got[0, 0] == -1).all()
    _, (want,) = expected_ord(pred, tgt, 2, ([0, 50, 95, 100],))
    same_ord(got, want, "ties")
    # one key above the ties (a predicted pixel 7 columns from the label): v[hi] is v[lo] while the rank stays inside the
    # ties, the next key above them otherwise.  set 0 = 200 x 4 and 49: (n - 1) q = 200 q, so 99.5 % ends on the last 4 exactly
    pred = np.pad(pred, ((0, 0), (0, 0), (0, 7)), constant_values=NONE)
    tgt = np.pad(tgt, ((0, 0), (0, 0), (0, 7)), constant_values=NONE)
    pred[0, 0, 11] = 1
    lists = ([99.5, 99.51, 100, 0], [50, 99.49, 99.99, 1])
    _, wants = expected_ord(pred, tgt, 2, lists)
    assert wants[0][0, 1, :, 0].tolist() == [[4, 4], [4, 49], [49, 49], [4, 4]]
    for pl, want in zip(lists, wants):
        same_ord(device_ord(dev, pred, tgt, 2, pl)[1], want, f"next key {pl}")


# ---- 3. classes without a value -----------------------------------------------------------------------------------------------------
def test_classes_without_a_value(dev):
    rng = np.random.default_rng(5)
    H, W, C = 40, 70, 5
    pred = np.full((2, H, W), NONE, dtype=np.uint8)
    tgt = np.full((2, H, W), NONE, dtype=np.uint8)
    for b in range(2):
        pred[b, 3:20, 5:30], tgt[b, 5:22 + b, 4:28] = 0, 0              # class 0: on both sides
        pred[b, 25:30, 40:60] = 1                                       # class 1: predicted only
        tgt[b, 30:38, 10:20] = 2                                        # class 2: labelled only
        pred[b, 22:24, 33 + b:50], tgt[b, 21:25, 35:52] = 4, 4          # class 4: on both sides; class 3: nowhere
    want_i, (want,) = expected_ord(pred, tgt, C, ([5, 50, 95, 99.5],))
    gi, got = device_ord(dev, pred, tgt, C, [5, 50, 95, 99.5])
    assert np.array_equal(gi, want_i)
    same_ord(got, want, "one-sided classes")
    assert (got[:, [1, 2, 3]] == -1).all() and (got[:, [0, 4]] >= 0).all()
    for m, c in zip(metrics_from_stats(gi[0], np.zeros((C, 2)), [], got[0], [5, 50, 95, 99.5]), range(C)):
        if c == 3:
            assert m is None
        elif c in (1, 2):
            assert m["unmatched"] and m["hd_pct"] is None and m["hd_pct_sym"] is None and m["hd"] is None
        else:
            assert len(m["hd_pct"]) == 4 and all(v >= 0 for v in m["hd_pct"] + m["hd_pct_sym"])
    # tables that send raw values to >= C: those pixels belong to no class on either side
    lut = np.where(np.arange(256) < 100, np.arange(256) % 3, 3 + np.arange(256) % 5).astype(np.uint8)
    plut = np.where(np.arange(256) < 200, np.arange(256) % 4, 9).astype(np.uint8)
    raw_t = rng.integers(0, 256, (2, 96 // 8 + 1, 131 // 8 + 1)).repeat(8, 1).repeat(8, 2)[:, :96, :131].astype(np.uint8)
    raw_p = rng.integers(0, 256, (2, 96 // 4 + 1, 131 // 4 + 1)).repeat(4, 1).repeat(4, 2)[:, :96, :131].astype(np.uint8)
    want_i, (want,) = expected_ord(raw_p, raw_t, 3, ([50, 95],), pred_lut=plut, lut=lut)
    gi, got = device_ord(dev, raw_p, raw_t, 3, [50, 95], pred_lut=plut, lut=lut)
    assert np.array_equal(gi, want_i) and want_i[:, :, 1].sum() < raw_p.size and want_i[:, :, 2].sum() < raw_t.size
    same_ord(got, want, "tables with values >= C")
    assert (got >= 0).all()


# ---- 4. chunks, repeats, the unchanged call -----------------------------------------------------------------------------------------
def test_chunked_calls_agree(dev, monkeypatch):
    pred, tgt = make_case("blobs", 3, 64, 83, 8, seed=21)
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
    whole = ops.surface_stats(p, t, 8, [1, 3], percentiles=[50, 95], return_d2="target")
    assert len(whole) == 4 and whole[2].dtype == torch.int64 and whole[3].dtype == torch.int32          # ints, sums, ord, d2
    monkeypatch.setattr(ops, "SURFACE_WORKSPACE_BYTES", 3 * 2 * 64 * 83 * 2 + 2 * 64 * 83 * 4)          # three classes of one frame
    assert ops.surface_plan(3, 64, 83, 8, percentiles=True) == (1, 3)
    parts = ops.surface_stats(p, t, 8, [1, 3], percentiles=[50, 95], return_d2="target")
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)
    _, (want,) = expected_ord(pred, tgt, 8, ([50, 95],))
    same_ord(parts[2].cpu().numpy(), want, "chunked")
    assert (want >= 0).any()


def test_repeat_calls_and_the_call_without_percentiles(dev):
    pred, tgt = make_case("blobs", 3, 33, 257, 8, seed=4)
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
    first = ops.surface_stats(p, t, 8, [1, 3], percentiles=[95, 99.5])
    second = ops.surface_stats(p, t, 8, [1, 3], percentiles=[95, 99.5])
    plain = ops.surface_stats(p, t, 8, [1, 3])
    assert len(first) == 3 and len(plain) == 2
    assert torch.equal(first[2], second[2]) and (first[2] >= 0).any()
    for a, b in zip(plain, first):
        assert torch.equal(a, b) and a.dtype == b.dtype
    with pytest.raises(ValueError, match="multiple of 0.01"):
        ops.surface_stats(p, t, 8, [1], percentiles=[95.001])
    with pytest.raises(ValueError, match="5 percentiles"):
        ops.surface_stats(p, t, 8, [1], percentiles=[1, 2, 3, 4, 5])


# ---- 5. entry points (the helpers of tests/test_gpu_surface.py, copied) -------------------------------------------------------------
def _engine(dev, num_classes):
    from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
    from adaptersis_amd.backbones.decoders import DecoderMLA
    from adaptersis_amd.backbones.encoders import FeatureEncoder
    from adaptersis_amd.backbones.engines import SegEngine
    from adaptersis_amd.dinov2.models import vision_transformer as vits
    from adaptersis_amd.utils import weights as W
    arch, D = "vit_tiny_test", 128
    model = vits.vit_tiny_test(patch_size=14, img_size=518, init_values=1e-5, block_chunks=0)
    model.load_state_dict(W.make_vit_state_dict(arch))
    enc = FeatureEncoder(embed_dim=D); enc.load_state_dict(W.make_encoder_state_dict(D))
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4); cv.load_state_dict(W.make_cavit_state_dict(D))
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25); cn.load_state_dict(W.make_cacnn_state_dict(D))
    dec = DecoderMLA(img_size=224, mla_channels=D, mlahead_channels=128, num_classes=num_classes)
    dec.load_state_dict(W.make_decoder_mla_state_dict(D, 128, num_classes))
    kw = dict(lr=0.01, momentum=0.9, weight_decay=0.0, loss="iou")
    return SegEngine(model.to(dev).eval(), enc.to(dev), cv.to(dev), cn.to(dev), dec.to(dev), num_classes=num_classes, **kw)


def _write_tree(root, sizes, n, seed):
    """frames/<k>/f<i>.png and labels/<k>/f<i>.png: blocky labels 0..7 as 32 c, the frame's colour follows the label."""
    rng = np.random.default_rng(seed)
    pal = (np.arange(8)[:, None] * np.array([[29, 71, 113]])) % 256
    for k, hw in enumerate(sizes):
        os.makedirs(os.path.join(root, "frames", str(k)))
        os.makedirs(os.path.join(root, "labels", str(k)))
        for i in range(n):
            lab = rng.integers(0, 8, (hw[0] // 32, hw[1] // 32)).repeat(32, 0).repeat(32, 1)
            img = np.clip(pal[lab] + rng.integers(-12, 13, hw + (3,)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(root, "frames", str(k), f"f{i}.png"))
            Image.fromarray((lab * 32).astype(np.uint8)).save(os.path.join(root, "labels", str(k), f"f{i}.png"))


def _same_surface(got, want):
    """Integers and structure with ==; float metrics within 1e-12 relative (the order of the float64 sums behind assd)."""
    def walk(a, b, path):
        if isinstance(b, dict):
            assert isinstance(a, dict) and sorted(a) == sorted(b), path
            for k in b:
                walk(a[k], b[k], f"{path}.{k}")
        elif isinstance(b, list):
            assert isinstance(a, list) and len(a) == len(b), path
            for i, (x, y) in enumerate(zip(a, b)):
                walk(x, y, f"{path}[{i}]")
        elif isinstance(b, float):
            assert isinstance(a, float) and abs(a - b) <= 1e-12 * abs(b), (path, a, b)
        else:
            assert a == b and type(a) is type(b), (path, a, b)
    walk(got, want, "surface")


def test_predict_and_score_entry_points(dev, tmp_path):
    from adaptersis_amd import predict as P
    from adaptersis_amd import score as S
    root = str(tmp_path / "data")
    _write_tree(root, [(192, 288), (256, 320)], 3, seed=2)                    # two native sizes, a short last batch each
    C, tol, pct = 8, [1.0, 2.0], [95.0]

    def pargs(pred, *extra):
        return P.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "2", "--head", "mla",
                                               "--num_classes", str(C), "--input", os.path.join(root, "frames"), "--masks",
                                               os.path.join(root, "labels"), "--encode", "endovis2017", "--pred_dir",
                                               str(tmp_path / pred), "--surface", "1", "2", *extra])

    torch.manual_seed(0)
    surf = pargs("surf")
    P.predict_seg(surf, engine=_engine(dev, C))
    torch.manual_seed(0)
    both = pargs("both", "--hd_percentile", "95")
    P.predict_seg(both, engine=_engine(dev, C))
    m_surf = json.load(open(os.path.join(surf.pred_dir, "metrics.json")))
    m_both = json.load(open(os.path.join(both.pred_dir, "metrics.json")))
    new_top, new_class = ["mean_hd_pct", "mean_hd_pct_sym", "percentiles"], ["hd_pct", "hd_pct_sym"]
    rels = sorted(f"{k}/f{i}.png" for k in range(2) for i in range(3))
    for r in rels:
        assert open(os.path.join(surf.pred_dir, r), "rb").read() == open(os.path.join(both.pred_dir, r), "rb").read()
    # without the flag: none of the new keys; with it: the new keys beside unchanged old ones
    assert sorted(m_both) == sorted(m_surf) and all(m_both[k] == m_surf[k] for k in m_surf if k != "surface")
    s0, s1 = m_surf["surface"], m_both["surface"]
    assert not set(new_top) & set(s0) and not any(set(new_class) & set(p) for p in s0["per_class"])
    assert sorted(s1) == sorted(list(s0) + new_top) and all(s1[k] == s0[k] for k in s0 if k != "per_class")
    for p0, p1 in zip(s0["per_class"], s1["per_class"]):
        assert sorted(p1) == sorted(list(p0) + new_class) and all(p1[k] == p0[k] for k in p0)
    assert s1["percentiles"] == pct

    # the host formula on the PNGs predict wrote and the ground-truth PNGs
    meter = SurfaceMeter(C, tol, pct)
    for r in rels:
        pred = np.array(Image.open(os.path.join(both.pred_dir, r)))[None]
        gt = np.array(Image.open(os.path.join(root, "labels", r)))[None]
        ints, sums = R.stats(pred, gt, C, tol, pred_lut=FR.LUT_MULTI, lut=FR.LUT_MULTI)
        _, (ords,) = expected_ord(pred, gt, C, (pct,), pred_lut=FR.LUT_MULTI, lut=FR.LUT_MULTI)
        meter.update(ints, sums, ords)
    want = json.loads(json.dumps(meter.result()))
    _same_surface(s1, want)
    assert any(p["hd_pct"] is not None for p in s1["per_class"][1:]) and s1["mean_hd_pct"][0] is not None
    for p, q in zip(s1["per_class"], want["per_class"]):          # exact integers behind them: the percentiles agree to the bit
        assert p["hd_pct"] == q["hd_pct"] and p["hd_pct_sym"] == q["hd_pct_sym"]
        if p["hd_pct"] is not None:
            assert p["hd_pct"][0] <= p["hd"] and p["hd_pct_sym"][0] <= p["hd"]

    # score on the written masks: the same block, no model
    m_score = S.score(S.get_args_parser().parse_args(["--pred_dir", both.pred_dir, "--masks", os.path.join(root, "labels"), "--encode",
                                                      "endovis2017", "--num_classes", str(C), "--batch_size_per_gpu", "2", "--surface",
                                                      "1", "2", "--hd_percentile", "95"]))
    on_disk = json.load(open(os.path.join(both.pred_dir, "metrics.json")))
    assert json.loads(json.dumps(m_score)) == on_disk and on_disk["surface"] == s1
    m_plain = S.score(S.get_args_parser().parse_args(["--pred_dir", surf.pred_dir, "--masks", os.path.join(root, "labels"), "--encode",
                                                      "endovis2017", "--num_classes", str(C), "--batch_size_per_gpu", "2", "--surface",
                                                      "1", "2"]))
    assert json.loads(json.dumps(m_plain))["surface"] == s0
