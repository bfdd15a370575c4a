"""GPU: test-time augmentation — ``ops.predict_mask_views`` (csrc/predict.hip) against torch's float64 ``F.interpolate`` + softmax +
mean on the CPU, its exact properties (mirrored views, repeated views, repeated calls, ties), tails and unaligned addresses,
overlay and counts against numpy, argument errors; ``SegEngine.predict_views`` against ``predict`` and ``eval_logits``; the
``adaptersis_amd.predict`` entry point with ``--tta_flip --tta_sizes --confidence`` on a two-size EndoVis2017-style PNG tree."""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from adaptersis_amd import ops
from adaptersis_amd.tools import frame_resize as FR

pytestmark = pytest.mark.gpu

TAU = 2e-4            # float64 top-2 margin of the mean probability below which a pixel is left out (20 x torch's own fp32 error)
SECOND_SIZE = 448     # the second input size of the engine and entry-point tests

CASES = {
    "A": ([(42, 42), (42, 42)], [0, 1], (301, 517)),
    "B": ([(32, 32), (42, 42), (42, 42), (53, 37)], [0, 0, 1, 1], (301, 517)),
    "C": ([(37, 53)], [1], (131, 203)),
    "D": ([(32, 32), (32, 32), (42, 42), (42, 42), (52, 52), (52, 52)], [0, 1, 0, 1, 0, 1], (256, 320)),
}


def mean_prob64(views, flips, H, W):
    """float64 [B,C,H,W]: the mean over the views of softmax(F.interpolate(view, mirrored first when flipped))."""
    tot = None
    for v, f in zip(views, flips):
        x = v.permute(0, 3, 1, 2).double()
        if f:
            x = x.flip(-1)
        p = F.interpolate(x, size=(H, W), mode="bilinear", align_corners=False).softmax(1)
        tot = p if tot is None else tot + p
    return tot / len(views)


def margin_rule(prob):
    """-> (argmax [B,H,W], sure [B,H,W] = top-2 margin >= TAU, max [B,H,W])."""
    top = prob.topk(2, dim=1).values
    return prob.argmax(1), (top[:, 0] - top[:, 1]) >= TAU, top[:, 0]


@functools.lru_cache(maxsize=None)
def _case(name, C):
    shapes, flips, (H, W) = CASES[name]
    g = torch.Generator().manual_seed(4321 + C)
    views = [torch.randn(1, h, w, C, generator=g) * 3.0 for (h, w) in shapes]
    return views, flips, H, W, margin_rule(mean_prob64(views, flips, H, W))


def _views(C, B, shapes, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return [(scale * torch.randn((B, h, w, C), generator=g)).contiguous() for h, w in shapes]


# ---- 1. against float64 on the CPU ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("C", [2, 3, 8, 10, 11, 16])
def test_mask_and_confidence_vs_float64(dev, C, name):
    """Pixels whose float64 top-2 margin of the mean probability is below tau = 2e-4 are left out (torch's own fp32 evaluation of
    the formula differs from float64 by at most 1.0e-5 in probability on these inputs; 20 x that for two classes moving in
    opposite directions and taps that round differently); they must stay <= 0.4 % and every other pixel must agree; the
    confidence is within one level of round(255 * max) everywhere."""
    views, flips, H, W, (want, sure, pmax) = _case(name, C)
    mask, conf = ops.predict_mask_views([v.to(dev) for v in views], (H, W), flips=flips, confidence=True)
    assert mask.dtype == torch.uint8 and conf.dtype == torch.uint8 and tuple(mask.shape) == tuple(conf.shape) == (1, H, W)
    left_out = 1.0 - float(sure.double().mean())
    wrong = int(((mask.cpu().long() != want) & sure).sum())
    conf_err = int((conf.cpu().long() - torch.round(255.0 * pmax).long()).abs().max())
    print(f"case {name} C={C} K={len(views)} -> {H}x{W}: left out {100 * left_out:.4f} %, disagreements outside the margin {wrong}, "
          f"largest confidence difference {conf_err} levels")
    assert left_out <= 0.004, f"{100 * left_out:.3f} % of the pixels inside the margin"
    assert wrong == 0
    assert conf_err <= 1
    assert torch.equal(mask, ops.predict_mask_views([v.to(dev) for v in views], (H, W), flips=flips))      # without the confidence


# ---- 2. exact properties ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [203, 517])
@pytest.mark.parametrize("C", [3, 8])
def test_exact_properties(dev, C, W):
    H = 131
    v, u = (t.to(dev) for t in _views(C, 2, [(37, 53), (42, 42)], seed=C * 10 + W))
    enc = torch.arange(C, dtype=torch.uint8) * 7 + 3
    run = lambda views, flips: ops.predict_mask_views(views, (H, W), enc, flips=flips, confidence=True)
    # (a) a mirrored view is the un-mirrored view with its columns reversed, bit for bit
    for views_f, flips_f, views_p in (([v], [True], [v.flip(2).contiguous()]),
                                      ([u, v], [False, True], [u, v.flip(2).contiguous()]),
                                      ([v, u], [True, True], [v.flip(2).contiguous(), u.flip(2).contiguous()])):
        got, want = run(views_f, flips_f), run(views_p, [False] * len(views_p))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(run([v], [True])[0], run([v], [False])[0])            # and the flag does something
    # (b) p + p is exact: a repeated view changes nothing
    one, two = run([v], [False]), run([v, v], [False, False])
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    four = run([v, v, v, v], [True] * 4)
    assert torch.equal(four[0], run([v], [True])[0]) and torch.equal(four[1], run([v], [True])[1])
    # (c) two calls on the same inputs
    a, b = run([u, v, u], [False, True, True]), run([u, v, u], [False, True, True])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_ties_go_to_the_lowest_class(dev):
    # (d) equal logits: class 0 everywhere, confidence 255 / C rounded
    allsame = [torch.full((1, 7, 7, 16), -2.5).to(dev), torch.full((1, 5, 9, 16), 4.0).to(dev)]
    mask, conf = ops.predict_mask_views(allsame, (33, 35), flips=[False, True], confidence=True)
    assert bool((mask == 0).all()) and bool((conf == 16).all())                  # 255 / 16 + 0.5 = 16.4
    const = torch.zeros((2, 9, 11, 8))
    const[..., 2] = 1.0
    const[..., 5] = 1.0                                                          # classes 2 and 5 hold the same maximal value
    enc = torch.arange(8, dtype=torch.uint8) * 10
    for views, flips in (([const], [False]), ([const, const[:, :5, :7].contiguous()], [True, False])):
        got = ops.predict_mask_views([t.to(dev) for t in views], (64, 83), enc, flips=flips)
        assert bool((got == 20).all())


# ---- 3. tails and alignment -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [1, 2, 3, 5, 6, 7, 517])
def test_tails_and_unaligned_rows(dev, W):
    """Widths that are not multiples of the 4-byte store, two frames: the second frame's mask and confidence start at 9 * W bytes
    (every alignment), the last quad of a row is short.  Against float64 with the margin rule of test 1."""
    H, C = 9, 3
    views, flips = _views(C, 2, [(23, 31), (17, 29)], seed=77), [False, True]
    want, sure, pmax = margin_rule(mean_prob64(views, flips, H, W))
    mask, conf = ops.predict_mask_views([v.to(dev) for v in views], (H, W), flips=flips, confidence=True)
    left_out = 1.0 - float(sure.double().mean())
    wrong = int(((mask.cpu().long() != want) & sure).sum())
    print(f"W={W}: left out {100 * left_out:.4f} %, disagreements outside the margin {wrong}")
    assert left_out <= 0.004 and wrong == 0
    assert int((conf.cpu().long() - torch.round(255.0 * pmax).long()).abs().max()) <= 1
    # logit maps whose address is only 4- or 8-byte aligned: the wide channel loads must not be taken, the values are the same
    for Cc, off in ((8, 1), (8, 2), (4, 3), (2, 1)):
        src = _views(Cc, 2, [(23, 31), (17, 29)], seed=W + Cc + off)
        aligned = [s.to(dev) for s in src]
        flat = torch.zeros(2 * 23 * 31 * Cc + 4, device=dev)
        odd = flat[off:off + 2 * 23 * 31 * Cc].view(2, 23, 31, Cc)
        odd.copy_(src[0])
        assert odd.is_contiguous() and odd.data_ptr() % 16 != 0
        for order in ((0, 1), (1, 0)):                                           # the misaligned map first and last
            a = ops.predict_mask_views([aligned[k] for k in order], (40, W), flips=[True, False], confidence=True)
            b = ops.predict_mask_views([(odd, aligned[1])[k] for k in order], (40, W), flips=[True, False], confidence=True)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("off", [0, 1, 2])
@pytest.mark.parametrize("C", range(1, 17))
def test_every_load_width_and_class_bucket(dev, C, off):
    """Every instance of the kernel: the class bucket follows C (4, 8, 16), the load width C and the maps' addresses.  The first
    map starts ``off`` floats into a 16-byte aligned buffer (16-byte loads when C % 4 == 0 and off == 0, 8-byte loads when C is
    even and off is, dword loads otherwise); mask and confidence must equal those of its 16-byte aligned copy bit for bit."""
    B, n = 2, 2 * 5 * 7 * C
    src = _views(C, B, [(5, 7), (6, 4)], seed=100 * C + off)
    aligned = [s.to(dev) for s in src]
    flat = torch.zeros(n + 4, device=dev)
    assert flat.data_ptr() % 16 == 0 and aligned[0].data_ptr() % 16 == 0 and aligned[1].data_ptr() % 16 == 0
    odd = flat[off:off + n].view(B, 5, 7, C)
    odd.copy_(src[0])
    a = ops.predict_mask_views(aligned, (9, 13), flips=[False, True], confidence=True)
    b = ops.predict_mask_views([odd, aligned[1]], (9, 13), flips=[False, True], confidence=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. overlay and counts --------------------------------------------------------------------------------------------------
def _np_counts(mask_idx, label, C):
    return np.array([[int(((mask_idx == c) & (label == c)).sum()), int((mask_idx == c).sum()), int((label == c).sum())]
                     for c in range(C)], dtype=np.int64)


@pytest.mark.parametrize("C,H,W", [(8, 256, 320), (3, 131, 203)])
def test_overlay_and_counts(dev, C, H, W):
    g = torch.Generator().manual_seed(C + H)
    views = _views(C, 2, [(24, 30), (31, 27)], seed=C)
    views[0][..., C - 1] -= 100.0
    views[1][..., C - 1] -= 100.0                                                # a class that is never predicted
    views = [v.to(dev) for v in views]
    frames = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    palette = torch.randint(0, 256, (C, 3), generator=g, dtype=torch.uint8)
    alpha = torch.randint(0, 256, (C,), generator=g, dtype=torch.uint8)
    alpha[0] = 0
    raw = torch.randint(0, 8, (2, H, W), generator=g, dtype=torch.uint8) * 32    # LUT_MULTI labels 0..7: some >= C when C < 8
    lut = FR.LUT_MULTI
    enc = torch.from_numpy(FR.ENCODE_ENDOVIS2017[:C].copy())
    plain = ops.predict_mask_views(views, (H, W), enc, flips=[False, True])
    mask, conf, over, counts = ops.predict_mask_views(views, (H, W), enc, flips=[False, True], confidence=True, frames=frames.to(dev),
                                                      palette=palette, alpha=alpha, target=raw.to(dev), lut=lut)
    assert torch.equal(mask, plain)
    assert torch.equal(conf, ops.predict_mask_views(views, (H, W), enc, flips=[False, True], confidence=True)[1])
    m = mask.cpu().numpy().astype(np.int64) >> 5
    f, p, a = frames.numpy().astype(np.int64), palette.numpy().astype(np.int64), alpha.numpy().astype(np.int64)
    want = (f * (255 - a[m])[..., None] + p[m] * a[m][..., None] + 127) // 255
    assert np.array_equal(over.cpu().numpy(), want.astype(np.uint8))
    assert np.array_equal(over.cpu().numpy()[m == 0], frames.numpy()[m == 0])    # alpha 0 leaves the frame untouched
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (C, 3)
    cw = _np_counts(m, lut[raw.numpy()], C)
    assert np.array_equal(counts.cpu().numpy(), cw)
    assert cw[C - 1, 1] == 0 and int(cw[:, 1].sum()) == 2 * H * W
    m2, o2 = ops.predict_mask_views(views, (H, W), enc, flips=[False, True], frames=frames.to(dev), palette=palette, alpha=alpha)
    m3, c3 = ops.predict_mask_views(views, (H, W), enc, flips=[False, True], target=raw.to(dev), lut=lut)
    assert torch.equal(m2, mask) and torch.equal(o2, over) and torch.equal(m3, mask) and torch.equal(c3, counts)


# ---- 5. argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors(dev):
    v = _views(3, 2, [(8, 8)], seed=0)[0].to(dev)
    for logits, kw, name in (([], {}, "logits"), ([v] * 9, {}, "logits"), (v, {}, "logits"),
                             ([v, torch.zeros((2, 8, 8, 4), device=dev)], {}, r"logits\[1\]"),
                             ([v, torch.zeros((1, 8, 8, 3), device=dev)], {}, r"logits\[1\]"),
                             ([v, v], dict(flips=[True]), "flips"), ([v], dict(flips=[True, False]), "flips"),
                             ([v, v.half()], {}, r"logits\[1\]"), ([v.double()], {}, r"logits\[0\]"),
                             ([v, v.permute(0, 2, 1, 3)], {}, r"logits\[1\]"), ([v[:, :, ::2]], {}, r"logits\[0\]"),
                             ([v], dict(encode=[1, 2]), "encode"), ([v], dict(palette=[[0, 0, 0]] * 3), "frames"),
                             ([v], dict(target=torch.zeros((2, 16, 16), dtype=torch.uint8, device=dev)), "lut")):
        with pytest.raises(ValueError, match=name):
            ops.predict_mask_views(logits, 16, **kw)
    with pytest.raises(ValueError, match="size"):
        ops.predict_mask_views([v], (0, 4))
    with pytest.raises(ValueError, match="C=17"):
        ops.predict_mask_views([torch.zeros((1, 4, 4, 17), device=dev)], 16)
    with pytest.raises(Exception, match="CPU tensor"):
        ops.predict_mask_views([v.cpu()], 16)
    assert tuple(ops.predict_mask_views([v] * 8, 16, flips=[True, False] * 4).shape) == (2, 16, 16)      # 8 views are allowed


# ---- 6. engine --------------------------------------------------------------------------------------------------------------
def _engine(head, dev, num_classes):
    from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
    from adaptersis_amd.backbones.decoders import DecoderMLA, FeatureDecoder
    from adaptersis_amd.backbones.encoders import FeatureEncoder
    from adaptersis_amd.backbones.engines import SegEngine
    from adaptersis_amd.dinov2.models import vision_transformer as vits
    from adaptersis_amd.utils import weights as W
    arch, D = "vit_tiny_test", 128
    model = vits.vit_tiny_test(patch_size=14, img_size=518, init_values=1e-5, block_chunks=0)
    model.load_state_dict(W.make_vit_state_dict(arch))
    enc = FeatureEncoder(embed_dim=D)
    enc.load_state_dict(W.make_encoder_state_dict(D))
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4)
    cv.load_state_dict(W.make_cavit_state_dict(D))
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25)
    cn.load_state_dict(W.make_cacnn_state_dict(D))
    if head == "mla":
        dec = DecoderMLA(img_size=224, mla_channels=D, mlahead_channels=128, num_classes=num_classes)
        dec.load_state_dict(W.make_decoder_mla_state_dict(D, 128, num_classes))
        kw = dict(lr=0.01, momentum=0.9, weight_decay=0.0, loss="iou")
    else:
        feats = (128, 32, 16, 16, 8)
        dec = FeatureDecoder(embed_dim=D, num_classes=num_classes, features=list(feats))
        dec.load_state_dict(W.make_feature_decoder_state_dict(D, num_classes, features=feats))
        kw = dict(lr=0.05)
    return SegEngine(model.to(dev).eval(), enc.to(dev), cv.to(dev), cn.to(dev), dec.to(dev), num_classes=num_classes, **kw)


def _bn_buffers(eng):
    return {n: b.clone() for n, b in eng.named_buffers() if "running_" in n or "num_batches_tracked" in n}


@pytest.mark.parametrize("head,C", [("feature", 2), ("mla", 8)])
def test_engine_predict_views(dev, head, C):
    from adaptersis_amd.utils import weights as W
    img, tgt = W.synthetic_batch(2, 224, C)
    img, tgt = img.to(dev), tgt.to(dev)
    big = W.synthetic_batch(2, SECOND_SIZE, C)[0].to(dev)
    size = (301, 517)
    inps, flips = [img, img.flip(3).contiguous(), big], [False, True, False]
    losses = {}
    for with_views in (False, True):
        eng = _engine(head, dev, C)
        eng.seg_decoder.train()
        if with_views:
            before = _bn_buffers(eng)
            assert before
            got = eng.predict_views(inps, flips, size, confidence=True)
            assert eng.seg_decoder.training and eng.backbone_encoder.update_running_stats
            after = _bn_buffers(eng)
            assert all(torch.equal(before[n], after[n]) for n in before), "predict_views moved a BatchNorm running buffer"
            assert all(t.dtype == torch.uint8 and tuple(t.shape) == (2,) + size for t in got)
            # one ops.predict_mask_views call on the logits validation sees, view by view
            eng.seg_decoder.eval()
            upd, eng.backbone_encoder.update_running_stats = eng.backbone_encoder.update_running_stats, False
            logits = [eng.eval_logits(x) for x in inps]
            eng.backbone_encoder.update_running_stats = upd
            eng.seg_decoder.train()
            assert logits[0].shape[1:3] != logits[2].shape[1:3]                  # the views differ in size
            want = ops.predict_mask_views(logits, size, flips=flips, confidence=True)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
            # one plain view against predict: exp is monotone, so only ties after rounding can differ
            one, ref = eng.predict_views([img], [False], size), eng.predict(img, size)
            top = ops.resize_bilinear_fwd(logits[0], *size).topk(2, dim=-1).values
            sure = (top[..., 0] - top[..., 1]) >= 1e-5
            left_out = 1.0 - float(sure.double().mean())
            wrong = int(((one != ref) & sure).sum())
            print(f"{head} C={C}: left out {100 * left_out:.4f} %, disagreements with predict outside the margin {wrong}")
            assert left_out <= 0.001 and wrong == 0
            eng.seg_decoder.eval()
            eng.predict_views([img], [True], size)
            assert not eng.seg_decoder.training                                  # restored to what it was, whichever that is
            eng = _engine(head, dev, C)                                          # a fresh engine for the comparison of the losses
            eng.seg_decoder.train()
            eng.predict_views(inps, flips, size)
        losses[with_views] = eng.train_step(img, tgt).clone()
    assert torch.equal(losses[False], losses[True]), "a predict_views call changed the following train_step"


# ---- 7. entry point ---------------------------------------------------------------------------------------------------------
def _write_tree(root, split, seq_sizes, n, seed):
    """EndoVis2017 layout: per sequence n frames and instruments masks (blocky labels 0..7, the colour follows the label)."""
    rng = np.random.default_rng(seed)
    pal = (np.arange(8)[:, None] * np.array([[29, 71, 113]])) % 256
    for s, hw in seq_sizes.items():
        d = os.path.join(root, split, f"instrument_dataset_{s}")
        os.makedirs(os.path.join(d, "images"))
        os.makedirs(os.path.join(d, "instruments_masks"))
        for k in range(n):
            lab = rng.integers(0, 8, (hw[0] // 32, hw[1] // 32)).repeat(32, 0).repeat(32, 1)
            img = np.clip(pal[lab] + rng.integers(-12, 13, hw + (3,)), 0, 255).astype(np.uint8)
            Image.fromarray(img).save(os.path.join(d, "images", f"frame{k:03d}.png"))
            Image.fromarray((lab * 32).astype(np.uint8)).save(os.path.join(d, "instruments_masks", f"frame{k:03d}.png"))


def _read_tree(d):
    return {os.path.relpath(os.path.join(r, f), d): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(d) for f in fs}


def test_predict_entry_point_with_views(dev, tmp_path):
    from adaptersis_amd import predict as P
    from adaptersis_amd import train as T
    from adaptersis_amd import train_multi_class as TMC
    root, out = str(tmp_path / "ev17"), str(tmp_path / "out")
    native = {1: (256, 320), 2: (192, 288)}
    _write_tree(root, "Train", {1: (256, 320)}, 8, seed=0)
    _write_tree(root, "Test", native, 5, seed=1)                                  # two native sizes, short last batches
    model_args = ["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4", "--num_workers", "0", "--output_dir", out]
    T._ENGINES.clear(); T._AUGMENTERS.clear()
    torch.manual_seed(0)
    TMC.train_seg(TMC.get_args_parser().parse_args(model_args + ["--lr", "0.08", "--data_path", root, "--epochs", "1",
                                                                 "--num_classes", "8"]))
    T._ENGINES.clear()

    def pargs(pred, *extra):
        return P.get_args_parser().parse_args(model_args + ["--head", "mla", "--num_classes", "8", "--input", root, "--dataset",
                                                            "endovis2017", "--split", "Test", "--encode", "endovis2017", "--masks",
                                                            "--seed", "0", "--pred_dir", str(tmp_path / pred), *extra])
    args = pargs("tta", "--tta_flip", "--tta_sizes", "224", str(SECOND_SIZE), "--confidence", "--surface")
    eng = P.build_engine(args)
    res = P.predict_seg(args, engine=eng)
    rels = [f"instrument_dataset_{s}/images/frame{k:03d}.png" for s in (1, 2) for k in range(5)]
    assert sorted(res["files"]) == rels
    got = _read_tree(args.pred_dir)
    assert sorted(got) == sorted(rels + [r[:-4] + "_conf.png" for r in rels] + ["metrics.json"])
    views = [(224, False), (224, True), (SECOND_SIZE, False), (SECOND_SIZE, True)]
    met = json.load(open(os.path.join(args.pred_dir, "metrics.json")))
    assert met["views"] == [[s, f] for s, f in views] and met["frames"] == 10 and "surface" in met
    masks, confs = {}, {}
    for r in rels:
        hw = native[int(r.split("/")[0].rsplit("_", 1)[1])]
        for store, path in ((masks, r), (confs, r[:-4] + "_conf.png")):
            im = Image.open(os.path.join(args.pred_dir, path))
            assert im.mode == "L" and im.size == (hw[1], hw[0])
            store[r] = np.array(im)
        assert set(np.unique(masks[r]).tolist()) <= set(range(0, 256, 32))
    # the same batches through engine.predict_views and engine.predict: sizes ascending, sorted paths inside a size, 4 per batch
    enc = FR.encode_table("endovis2017", 8)
    plain = {}
    for batch in ([f"instrument_dataset_2/images/frame{k:03d}.png" for k in range(4)], ["instrument_dataset_2/images/frame004.png"],
                  [f"instrument_dataset_1/images/frame{k:03d}.png" for k in range(4)], ["instrument_dataset_1/images/frame004.png"]):
        frames = torch.from_numpy(np.stack([np.array(Image.open(os.path.join(root, "Test", r)).convert("RGB")) for r in batch])).to(dev)
        inps = []
        for s, f in views:
            small, _ = ops.frame_resize(frames, None, s)
            small = small.flip(2).contiguous() if f else small
            inps.append(T._to_device_batch(small, torch.zeros(small.shape[:3], dtype=torch.uint8, device=dev), train=False)[0])
        m, c = eng.predict_views(inps, [f for _, f in views], tuple(frames.shape[1:3]), encode=enc, confidence=True)
        p = eng.predict(inps[0], size=tuple(frames.shape[1:3]), encode=enc)
        for k, r in enumerate(batch):
            assert np.array_equal(m[k].cpu().numpy(), masks[r]), r
            assert np.array_equal(c[k].cpu().numpy(), confs[r]), r
            plain[r] = p[k].cpu().numpy()
    counts = _np_counts(np.concatenate([masks[r].reshape(-1) >> 5 for r in rels]),
                        np.concatenate([np.array(Image.open(os.path.join(root, "Test", r.replace("/images/", "/instruments_masks/"))))
                                        .reshape(-1) >> 5 for r in rels]), 8)
    assert met["counts"] == counts.tolist()

    # without any new flag: the files of predict_seg as it was (engine.predict on the same batches), byte for byte, no "views"
    a2 = pargs("plain")
    P.predict_seg(a2, engine=eng)
    got2 = _read_tree(a2.pred_dir)
    assert sorted(got2) == sorted(rels + ["metrics.json"])
    assert "views" not in json.load(open(os.path.join(a2.pred_dir, "metrics.json")))
    for r in rels:
        assert np.array_equal(np.array(Image.open(os.path.join(a2.pred_dir, r))), plain[r]), r
    a3 = pargs("plain2")
    P.predict_seg(a3, engine=eng)
    assert _read_tree(a3.pred_dir) == got2
