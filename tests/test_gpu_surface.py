"""GPU: boundary metrics — ``ops.surface_stats`` (csrc/surface.hip) against the scipy oracle (tests/surface_ref.py): the squared
distance field bit for bit, every integer statistic with ``==``, the float64 sums within the bound that the order of a sum of
correctly rounded terms allows and bit-identical between calls; then ``predict --masks --surface`` and ``adaptersis_amd.score`` on a
two-size PNG tree."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from adaptersis_amd import ops
from adaptersis_amd.tools import frame_resize as FR

from . import surface_ref as R

pytestmark = pytest.mark.gpu

TOL = [0, 1, 2.5, 7]
NONE = 255      # a raw value that the identity table maps to no class (>= C for every C <= 16)


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _classes(C, rng):
    """Up to three classes of 0..C-1, the highest always among them (the full-size cases cost the oracle ~0.5 s per class)."""
    rest = rng.permutation(C - 1)[:2].tolist() if C > 1 else []
    return [C - 1] + rest


def _blobs(rng, H, W, classes, shift):
    m = np.full((H, W), NONE if len(classes) < 2 else classes[-1], dtype=np.uint8)     # background: a class when there are two
    yy, xx = np.mgrid[0:H, 0:W]
    for c in classes[:2] if len(classes) > 1 else classes:
        for _ in range(2):
            cy, cx = rng.integers(0, H) + shift[0], rng.integers(0, W) + shift[1]
            ry, rx = 1 + rng.integers(0, max(2, H // 4)), 1 + rng.integers(0, max(2, W // 4))
            m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = c
    return m


def make_case(kind, B, H, W, C, seed):
    """-> pred, target uint8 [B,H,W] of class indices (NONE = no class)."""
    rng = np.random.default_rng(seed)
    pred = np.full((B, H, W), NONE, dtype=np.uint8)
    tgt = np.full((B, H, W), NONE, dtype=np.uint8)
    for b in range(B):
        cl = _classes(C, rng)
        if kind == "blobs":
            shift = (int(rng.integers(-3, 4)), int(rng.integers(-3, 4)))
            state = rng.bit_generator.state
            pred[b] = _blobs(rng, H, W, cl, (0, 0))
            rng.bit_generator.state = state                       # the same blobs, a few pixels away
            tgt[b] = _blobs(rng, H, W, cl, shift)
        elif kind == "lines":
            for k, c in enumerate(cl):
                y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
                pred[b, y, :] = c
                tgt[b, :, x] = c
                d = np.arange(min(H, W))
                tgt[b, d, (d + k) % W] = c
        elif kind == "single":
            pred[b, rng.integers(0, H), rng.integers(0, W)] = cl[0]
            tgt[b, rng.integers(0, H), rng.integers(0, W)] = cl[0]
        elif kind == "full":
            pred[b], tgt[b] = cl[0], cl[0]
        elif kind == "checker":
            yy, xx = np.mgrid[0:H, 0:W]
            odd = ((yy + xx) & 1).astype(bool)
            a, z = cl[0], (cl[1] if len(cl) > 1 else NONE)
            pred[b] = np.where(odd, a, z)
            tgt[b] = np.where(odd, z, a)
        elif kind == "oneside":
            pred[b] = np.where(rng.random((H, W)) < 0.3, cl[0], NONE)          # cl[0] is predicted only
            if len(cl) > 1:
                pred[b, rng.integers(0, H), rng.integers(0, W)] = cl[1]
                tgt[b] = np.where(rng.random((H, W)) < 0.02, cl[1], NONE)
        else:
            raise AssertionError(kind)
    return pred, tgt


KINDS = ("blobs", "lines", "single", "full", "checker", "oneside")


def compare(dev, pred, tgt, C, tol=TOL, pred_lut=None, lut=None, fields=True, label=""):
    """Device against oracle: fields (both sides) bit for bit, integers with ==, sums within the derived bound and bit-identical
    between two calls.  -> (ints, sums) of the oracle."""
    want_i, want_s, d2p, d2g = R.stats(pred, tgt, C, tol, pred_lut=pred_lut, lut=lut, want_d2=True)
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
    runs = []
    for side, ref in (("pred", d2p), ("target", d2g)) if fields else (("pred", None), ("pred", None)):
        out = ops.surface_stats(p, t, C, tol, pred_lut=pred_lut, lut=lut, return_d2=side if fields else None)
        runs.append((out[0].cpu().numpy(), out[1].cpu().numpy()))
        if fields:
            d2 = out[2].cpu().numpy()
            assert d2.dtype == np.int32 and d2.shape == (pred.shape[0], C) + pred.shape[1:]
            for b in range(pred.shape[0]):
                for c in range(C):
                    if (b, c) in ref:
                        bad = int((d2[b, c] != ref[b, c]).sum())
                        assert bad == 0, f"{label} d2 of the {side} side, frame {b} class {c}: {bad} pixels differ from the oracle"
                    else:
                        assert (d2[b, c] == -1).all(), f"{label} {side} frame {b} class {c}: no edge pixels, field must stay -1"
    (gi, gs), (gi2, gs2) = runs
    assert gi.dtype == np.int64 and gi.shape == want_i.shape and gs.dtype == np.float64 and gs.shape == want_s.shape
    assert np.array_equal(gi, want_i), f"{label} integer statistics differ at (frame, class, column) {np.argwhere(gi != want_i)[:8].tolist()}"
    assert np.array_equal(gi2, want_i)
    assert gs.tobytes() == gs2.tobytes(), f"{label} the float64 sums of two calls differ"
    for k in (0, 1):                                              # k = 0: over E(P) (e_pred terms), k = 1: over E(G)
        n = want_i[:, :, 3 + k].astype(np.float64)
        err, bound = np.abs(gs[:, :, k] - want_s[:, :, k]), n * 2.0 ** -52 * want_s[:, :, k]
        print(f"{label} sums[{k}]: max |device - oracle| {err.max():.3e}, bound there {bound.flat[err.argmax()]:.3e}")
        assert (err <= bound).all(), f"{label} sums[{k}] off by {err.max()} (bound {bound.flat[err.argmax()]})"
    return want_i, want_s


# ---- 1. + 2. + 4. field, statistics and sums against the oracle -----------------------------------------------------------------
SMALL = [(1, 1), (1, 37), (37, 1), (64, 83), (301, 517)]
LARGE = [(540, 960), (1080, 1920), (2, 16384), (16384, 2)]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("C", [1, 2, 8, 16])
@pytest.mark.parametrize("hw", SMALL)
def test_field_and_statistics_small(dev, hw, C, B):
    for k, kind in enumerate(KINDS):
        pred, tgt = make_case(kind, B, hw[0], hw[1], C, seed=hw[0] * 131 + hw[1] * 7 + C * 3 + B + k)
        compare(dev, pred, tgt, C, label=f"{kind} {hw} C={C} B={B}:")


@pytest.mark.parametrize("C,B", [(1, 3), (2, 1), (8, 1), (16, 3)])
@pytest.mark.parametrize("hw", LARGE)
def test_field_and_statistics_large(dev, hw, C, B):
    if hw == (1080, 1920):
        B = 1 if B == 1 else 2                        # the oracle's half second per class and frame; still a batch
    for k, kind in enumerate(KINDS):
        pred, tgt = make_case(kind, B, hw[0], hw[1], C, seed=hw[0] + hw[1] * 3 + C * 5 + k)
        compare(dev, pred, tgt, C, label=f"{kind} {hw} C={C} B={B}:")


def test_labels_outside_the_classes_and_encoded_predictions(dev):
    rng = np.random.default_rng(11)
    H, W = 96, 131
    # a label table that sends raw values to classes 0..2, and 100.. to 3.. (>= C = 3: no class)
    lut = np.where(np.arange(256) < 100, np.arange(256) % 3, 3 + np.arange(256) % 5).astype(np.uint8)
    blocks = rng.integers(0, 256, (2, H // 8 + 1, W // 8 + 1)).repeat(8, 1).repeat(8, 2)[:, :H, :W].astype(np.uint8)
    pred = rng.integers(0, 3, (2, H // 4 + 1, W // 4 + 1)).repeat(4, 1).repeat(4, 2)[:, :H, :W].astype(np.uint8)
    want_i, _ = compare(dev, pred, blocks, 3, lut=lut, label="lut with labels >= C:")
    assert want_i[:, :, 2].sum() == int((lut[blocks] < 3).sum()) < blocks.size
    # encoded predictions: binary255 (0 / 255 read through x > 0) and endovis2017 (32 c read through x >> 5)
    for name, C in (("binary255", 2), ("endovis2017", 8)):
        enc, table = FR.encode_table(name, C), FR.ENCODINGS[name][1]
        cls = rng.integers(0, C, (2, H // 16 + 1, W // 16 + 1)).repeat(16, 1).repeat(16, 2)[:, :H, :W]
        raw_t = np.roll(cls, 3, axis=2)
        tgt = (enc[raw_t] if name == "endovis2017" else np.where(raw_t > 0, rng.integers(1, 256, raw_t.shape), 0)).astype(np.uint8)
        wi, _ = compare(dev, enc[cls].astype(np.uint8), tgt, C, pred_lut=table, lut=table, label=f"{name}:")
        assert wi[:, :, 1].sum() == cls.size and [int(v) for v in wi[:, :, 1].sum(0)] == np.bincount(cls.reshape(-1), minlength=C).tolist()


# ---- 3. far apart ---------------------------------------------------------------------------------------------------------------
def test_far_apart(dev):
    H, W = 1080, 1920
    yy, xx = np.mgrid[0:H, 0:W]
    pred = np.zeros((1, H, W), dtype=np.uint8)
    tgt = np.zeros((1, H, W), dtype=np.uint8)
    pred[0][(yy - 60) ** 2 + (xx - 80) ** 2 <= 50 ** 2] = 1
    tgt[0][((yy - 1000) / 40) ** 2 + ((xx - 1800) / 70) ** 2 <= 1.0] = 1
    want_i, _ = compare(dev, pred, tgt, 2, fields=False, label="far apart:")
    assert want_i[0, 1, 0] == 0 and want_i[0, 1, 5] > 1500 ** 2 and want_i[0, 1, 6] > 1500 ** 2      # the maxima are the long way
    assert want_i[0, 1, 7:].sum() == 0                                                              # nothing within 7 pixels


def test_checkerboard_sums_full_size(dev):
    """The bound of the sums at its largest: every pixel of a 1080p frame is an edge pixel."""
    pred, tgt = make_case("checker", 1, 1080, 1920, 2, seed=5)
    want_i, _ = compare(dev, pred, tgt, 2, fields=False, label="1080p checkerboard:")
    assert want_i[0, :, 3].sum() == 1080 * 1920


def test_argument_errors(dev):
    z = torch.zeros((2, 8, 8), dtype=torch.uint8, device=dev)
    for bad, text in [((z.float(), z), "pred must be contiguous uint8"), ((z, z[:, :, ::2]), "target must be contiguous uint8"),
                      ((z, z[:1]), "differ in shape"), ((z[0], z[0]), r"uint8 \[B,H,W\]")]:
        with pytest.raises(ValueError, match=text):
            ops.surface_stats(*bad, 2, [1])
    with pytest.raises(ValueError, match="num_classes=17"):
        ops.surface_stats(z, z, 17, [1])
    with pytest.raises(ValueError, match="return_d2='both'"):
        ops.surface_stats(z, z, 2, [1], return_d2="both")
    with pytest.raises(ValueError, match="lut must be uint8"):
        ops.surface_stats(z, z, 2, [1], lut=np.zeros(16, dtype=np.uint8))
    ints, sums = ops.surface_stats(z, z, 2, [])                   # no tolerances: the seven fixed columns
    assert tuple(ints.shape) == (2, 2, 7) and ints[:, 0].tolist() == [[64, 64, 64, 28, 28, 0, 0]] * 2 and float(sums.abs().sum()) == 0


def test_chunked_calls_agree(dev, monkeypatch):
    """Frames and classes in several calls over one workspace (what a batch of full-size frames does) give the same numbers."""
    pred, tgt = make_case("blobs", 3, 64, 83, 8, seed=21)
    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
    whole = ops.surface_stats(p, t, 8, TOL, return_d2="target")
    monkeypatch.setattr(ops, "SURFACE_WORKSPACE_BYTES", 3 * 2 * 64 * 83 * 2)         # three classes of one frame per call
    assert ops.surface_plan(3, 64, 83, 8) == (1, 3)
    parts = ops.surface_stats(p, t, 8, TOL, return_d2="target")
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)
    compare(dev, pred, tgt, 8, label="chunked:")


# ---- 5. entry points ------------------------------------------------------------------------------------------------------------
def _engine(head, dev, num_classes):
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
    assert head == "mla"
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


def _read_tree(d):
    return {os.path.relpath(os.path.join(r, f), d): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(d) for f in fs}


def test_predict_and_score_entry_points(dev, tmp_path):
    from adaptersis_amd import predict as P
    from adaptersis_amd import score as S
    from adaptersis_amd.segloss.surface import SurfaceMeter
    root = str(tmp_path / "data")
    _write_tree(root, [(192, 288), (256, 320)], 3, seed=2)                    # two native sizes, a short last batch each
    C, tol = 8, [1.0, 3.0]

    def pargs(pred, *extra):
        return P.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "2", "--head", "mla",
                                               "--num_classes", str(C), "--input", os.path.join(root, "frames"), "--masks",
                                               os.path.join(root, "labels"), "--encode", "endovis2017", "--pred_dir",
                                               str(tmp_path / pred), *extra])

    torch.manual_seed(0)
    plain = pargs("plain")
    P.predict_seg(plain, engine=_engine("mla", dev, C))
    torch.manual_seed(0)
    surf = pargs("surf", "--surface", "1", "3")
    P.predict_seg(surf, engine=_engine("mla", dev, C))
    t_plain, t_surf = _read_tree(plain.pred_dir), _read_tree(surf.pred_dir)
    rels = sorted(f"{k}/f{i}.png" for k in range(2) for i in range(3))
    assert sorted(t_plain) == sorted(rels + ["metrics.json"]) == sorted(t_surf)
    assert all(t_plain[r] == t_surf[r] for r in rels), "--surface changed a mask PNG"
    m_plain, m_surf = json.loads(t_plain["metrics.json"]), json.loads(t_surf["metrics.json"])
    assert sorted(m_plain) == ["counts", "frames", "mean_iou", "per_class_iou", "pixel_accuracy", "pixels"]
    assert sorted(m_surf) == sorted(list(m_plain) + ["surface"])
    assert all(m_surf[k] == m_plain[k] for k in m_plain)

    # the oracle on the PNGs predict wrote and the ground-truth PNGs
    meter = SurfaceMeter(C, tol)
    counts = np.zeros((C, 3), dtype=np.int64)
    for r in rels:
        pred = np.array(Image.open(os.path.join(surf.pred_dir, r)))[None]
        gt = np.array(Image.open(os.path.join(root, "labels", r)))[None]
        ints, sums = R.stats(pred, gt, C, tol, pred_lut=FR.LUT_MULTI, lut=FR.LUT_MULTI)
        meter.update(ints, sums)
        counts += ints[0, :, :3]
    want = json.loads(json.dumps(meter.result()))
    assert counts.tolist() == m_plain["counts"]
    _same_surface(m_surf["surface"], want)

    # score on the written masks: the same block and the same region counts, no model
    m_score = S.score(S.get_args_parser().parse_args(["--pred_dir", surf.pred_dir, "--masks", os.path.join(root, "labels"), "--encode",
                                                      "endovis2017", "--num_classes", str(C), "--batch_size_per_gpu", "2", "--surface",
                                                      "1", "3"]))
    on_disk = json.load(open(os.path.join(surf.pred_dir, "metrics.json")))
    assert json.loads(json.dumps(m_score)) == on_disk
    assert sorted(on_disk) == sorted(m_surf) and all(on_disk[k] == m_surf[k] for k in m_plain)
    assert on_disk["surface"] == m_surf["surface"]                 # the same op on the same batches: the same numbers


def _same_surface(got, want):
    """Integers and structure with ==; the means of float metrics within 1e-12 relative (the sums' own bound is far below)."""
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
