"""GPU: prediction — ``ops.predict_mask`` (csrc/predict.hip) against the unfused path (bit for bit) and against torch's float64
``F.interpolate`` + ``argmax``; overlay and per-class counts against numpy; ``SegEngine.predict`` against ``validate_step``; the
``adaptersis_amd.predict`` entry point on a two-size EndoVis2017-style PNG tree."""
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


def lowest_argmax(r: torch.Tensor) -> torch.Tensor:
    """Lowest index of the maximum over the last axis, spelled out (no reliance on torch.argmax's tie order)."""
    C = r.shape[-1]
    idx = torch.arange(C, device=r.device).expand(r.shape)
    return torch.where(r == r.max(-1, keepdim=True).values, idx, torch.full_like(idx, C)).min(-1).values


def unfused(logits, H, W, encode):
    return encode.to(logits.device)[lowest_argmax(ops.resize_bilinear_fwd(logits, H, W))]


def _logits(C, B, h, w, seed, scale=3.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn((B, h, w, C), generator=g)).contiguous()


# ---- 1. bit-identity with resize_bilinear_fwd -> lowest-index argmax -> table --------------------------------------------------
@pytest.mark.parametrize("hw", [(168, 168), (147, 147), (42, 42), (37, 53)])
@pytest.mark.parametrize("C", [1, 2, 3, 8, 11, 16])
def test_mask_equals_unfused_path(dev, C, hw):
    h, w = hw
    g = torch.Generator().manual_seed(C * 1000 + h)
    encode = torch.randperm(256, generator=g)[:C].to(torch.uint8)         # distinct values: a wrong class cannot hide
    sizes = [(588, 588), (1024, 1280), (1080, 1920), (301, 517), (1, 1), (h, w), (h // 2 + 1, w // 3 + 2)]
    for B in (1, 3):
        lg = _logits(C, B, h, w, seed=C * 100 + h + B).to(dev)
        for H, W in sizes:
            got = ops.predict_mask(lg, (H, W), encode)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (B, H, W)
            want = unfused(lg, H, W, encode)
            bad = int((got != want).sum())
            assert bad == 0, f"C={C} {h}x{w} -> {H}x{W} B={B}: {bad} pixels differ from the unfused path"
    # encode=None is the class index; an int size is square
    assert torch.equal(ops.predict_mask(lg, 77), unfused(lg, 77, 77, torch.arange(C, dtype=torch.uint8)))


@pytest.mark.parametrize("W", [1, 2, 3, 5, 6, 7, 517, 1279])
def test_tails_and_unaligned_rows(dev, W):
    """Widths that are not multiples of the 4-byte store: rows start at every alignment, the last quad is short."""
    lg = _logits(5, 2, 23, 31, seed=W).to(dev)
    enc = torch.tensor([3, 250, 17, 99, 128], dtype=torch.uint8)
    for H in (1, 9):
        assert torch.equal(ops.predict_mask(lg, (H, W), enc), unfused(lg, H, W, enc))
    # a logit map whose address is only 4- or 8-byte aligned: the wide channel loads must not be taken
    for C, off in ((8, 1), (8, 2), (4, 3), (2, 1)):
        flat = torch.zeros(2 * 23 * 31 * C + 4, device=dev)
        view = flat[off:off + 2 * 23 * 31 * C].view(2, 23, 31, C)
        view.copy_(_logits(C, 2, 23, 31, seed=W + C + off))
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        e = torch.arange(C, dtype=torch.uint8)
        assert torch.equal(ops.predict_mask(view, (40, W), e), unfused(view.clone(), 40, W, e))


def test_ties_go_to_the_lowest_class(dev):
    enc = torch.tensor([10, 20, 30, 40], dtype=torch.uint8)
    const = torch.zeros((2, 9, 11, 4))
    const[..., 1] = 1.0
    const[..., 2] = 1.0                                                      # classes 1 and 2 tie everywhere, above 0 and 3
    got = ops.predict_mask(const.to(dev), (64, 83), enc)
    assert bool((got == 20).all())
    allsame = torch.full((1, 7, 7, 16), -2.5)
    assert bool((ops.predict_mask(allsame.to(dev), (33, 35)) == 0).all())
    lg = _logits(4, 2, 42, 42, seed=5)
    lg[..., 3] = lg[..., 1]                                                  # two equal channels on a varying map
    lg[..., 1] += 2.0
    lg[..., 3] += 2.0
    lg = lg.contiguous().to(dev)
    got = ops.predict_mask(lg, (301, 517), enc)
    assert torch.equal(got, unfused(lg, 301, 517, enc))
    assert int((got == 40).sum()) == 0 and int((got == 20).sum()) > 0


# ---- 2. against the reference's own calls in float64 ----------------------------------------------------------------------
@pytest.mark.parametrize("C,h,H,W", [(2, 168, 1024, 1280), (8, 168, 1024, 1280), (11, 147, 1080, 1920), (8, 168, 588, 588),
                                     (2, 168, 301, 517), (16, 96, 1024, 1280)])
def test_mask_vs_float64_interpolate_argmax(dev, C, h, H, W):
    """`train.py:422,616` on the CPU in float64.  Pixels whose float64 top-2 margin is below tau = 1e-3 are left out (torch's own
    fp32 interpolate differs from float64 by up to 3.7e-4 on these inputs and two classes can each move by that much); they must
    stay <= 0.2 % of the pixels, and every other pixel must agree."""
    tau = 1e-3
    lg = _logits(C, 1, h, h, seed=1234 + C)
    ref = F.interpolate(lg.permute(0, 3, 1, 2).double(), size=(H, W), mode="bilinear", align_corners=False)
    top = ref.topk(2, dim=1)
    sure = (top.values[:, 0] - top.values[:, 1]) >= tau
    want = ref.argmax(1)
    got = ops.predict_mask(lg.to(dev), (H, W)).cpu().long()
    left_out = 1.0 - float(sure.double().mean())
    wrong = int(((got != want) & sure).sum())
    print(f"C={C} {h} -> {H}x{W}: left out {100 * left_out:.4f} %, disagreements outside the margin {wrong}")
    assert left_out <= 0.002, f"{100 * left_out:.3f} % of the pixels inside the margin"
    assert wrong == 0


# ---- 3. overlay and counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", [(8, 256, 320), (3, 131, 203), (2, 64, 61)])
def test_overlay_is_the_integer_formula(dev, C, H, W):
    g = torch.Generator().manual_seed(C + H)
    lg = _logits(C, 2, 24, 30, seed=C).to(dev)
    frames = torch.randint(0, 256, (2, H, W, 3), generator=g, dtype=torch.uint8)
    palette = torch.randint(0, 256, (C, 3), generator=g, dtype=torch.uint8)
    alpha = torch.randint(0, 256, (C,), generator=g, dtype=torch.uint8)
    alpha[0] = 0
    alpha[-1] = 255
    mask, over = ops.predict_mask(lg, (H, W), frames=frames.to(dev), palette=palette, alpha=alpha)
    assert torch.equal(mask, ops.predict_mask(lg, (H, W)))
    m = mask.cpu().numpy().astype(np.int64)
    f, p, a = frames.numpy().astype(np.int64), palette.numpy().astype(np.int64), alpha.numpy().astype(np.int64)
    want = (f * (255 - a[m])[..., None] + p[m] * a[m][..., None] + 127) // 255
    assert np.array_equal(over.cpu().numpy(), want.astype(np.uint8))
    assert np.array_equal(over.cpu().numpy()[m == 0], frames.numpy()[m == 0])          # alpha 0 leaves the frame untouched
    assert np.array_equal(over.cpu().numpy()[m == C - 1], np.broadcast_to(palette.numpy()[C - 1], (int((m == C - 1).sum()), 3)))
    # defaults: green at alpha 128 on every class but 0
    _, over_d = ops.predict_mask(lg, (H, W), frames=frames.to(dev))
    a_d, p_d = FR.default_alpha(C).astype(np.int64), FR.default_palette(C).astype(np.int64)
    assert np.array_equal(over_d.cpu().numpy(), ((f * (255 - a_d[m])[..., None] + p_d[m] * a_d[m][..., None] + 127) // 255).astype(np.uint8))


def _np_counts(mask_idx, label, C):
    return np.array([[int(((mask_idx == c) & (label == c)).sum()), int((mask_idx == c).sum()), int((label == c).sum())]
                     for c in range(C)], dtype=np.int64)


@pytest.mark.parametrize("C,H,W", [(8, 256, 320), (5, 131, 203), (2, 1024, 1280)])
def test_counts_are_the_confusion_sums(dev, C, H, W):
    g = torch.Generator().manual_seed(C * 7 + W)
    lg = _logits(C, 3, 24, 30, seed=C + 50)
    lg[..., C - 1] -= 100.0                                                  # a class that is never predicted
    lg = lg.contiguous().to(dev)
    raw = (torch.randint(0, 8, (3, H, W), generator=g, dtype=torch.uint8) * 32)     # LUT_MULTI labels 0..7: some >= C when C < 8
    raw[raw == 32] = 0                                                       # and a label (1) absent from the batch
    lut = FR.LUT_MULTI
    enc = torch.from_numpy(FR.ENCODE_ENDOVIS2017[:C].copy())
    mask, counts = ops.predict_mask(lg, (H, W), enc, target=raw.to(dev), lut=lut)
    assert counts.dtype == torch.int64 and tuple(counts.shape) == (C, 3)
    pred = mask.cpu().numpy() >> 5
    want = _np_counts(pred, lut[raw.numpy()], C)
    assert np.array_equal(counts.cpu().numpy(), want)
    assert want[C - 1, 1] == 0 and want[1, 2] == 0
    assert int(want[:, 1].sum()) == 3 * H * W and (C == 8 or int(want[:, 2].sum()) < 3 * H * W)
    again = ops.predict_mask(lg, (H, W), enc, target=raw.to(dev), lut=lut)[1]
    assert torch.equal(again, counts)
    # all three outputs of one call, in order
    frames = torch.randint(0, 256, (3, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    m3, o3, c3 = ops.predict_mask(lg, (H, W), enc, frames=frames, target=raw.to(dev), lut=lut)
    assert torch.equal(m3, mask) and torch.equal(c3, counts) and tuple(o3.shape) == (3, H, W, 3)


def test_argument_errors(dev):
    lg = _logits(3, 1, 8, 8, seed=0).to(dev)
    with pytest.raises(Exception, match="CPU tensor"):
        ops.predict_mask(lg.cpu(), 16)
    for kw, name in ((dict(size=(0, 4)), "size"), (dict(size=16, encode=[1, 2]), "encode"),
                     (dict(size=16, frames=torch.zeros((1, 16, 15, 3), dtype=torch.uint8, device=dev)), "frames"),
                     (dict(size=16, palette=[[0, 0, 0]] * 3), "frames"),
                     (dict(size=16, target=torch.zeros((1, 16, 16), dtype=torch.uint8, device=dev)), "lut"),
                     (dict(size=16, target=torch.zeros((1, 16, 16), dtype=torch.int64, device=dev), lut=FR.LUT_BINARY), "target")):
        with pytest.raises(ValueError, match=name):
            ops.predict_mask(lg, **kw)
    with pytest.raises(ValueError, match="logits"):
        ops.predict_mask(lg.half(), 16)
    with pytest.raises(ValueError, match="C=17"):
        ops.predict_mask(torch.zeros((1, 4, 4, 17), device=dev), 16)


# ---- 4. engine ----------------------------------------------------------------------------------------------------------------
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
    enc = FeatureEncoder(embed_dim=D); enc.load_state_dict(W.make_encoder_state_dict(D))
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4); cv.load_state_dict(W.make_cavit_state_dict(D))
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25); cn.load_state_dict(W.make_cacnn_state_dict(D))
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


@pytest.mark.parametrize("head,C", [("feature", 2), ("mla", 2), ("mla", 8)])
def test_engine_predict(dev, head, C):
    from adaptersis_amd.utils import weights as W
    img, tgt = W.synthetic_batch(2, 224, C)
    img, tgt = img.to(dev), tgt.to(dev)
    losses = {}
    for with_predict in (False, True):
        eng = _engine(head, dev, C)
        eng.seg_decoder.train()
        if with_predict:
            before = _bn_buffers(eng)
            assert before
            pred = eng.predict(img)
            assert eng.seg_decoder.training
            after = _bn_buffers(eng)
            assert all(torch.equal(before[n], after[n]) for n in before), "predict moved a BatchNorm running buffer"
            assert pred.dtype == torch.uint8 and tuple(pred.shape) == (2, 224, 224)
            # the logits validate_step sees
            eng.seg_decoder.eval()
            logits = eng.eval_logits(img)
            eng.seg_decoder.train()
            assert torch.equal(pred, ops.predict_mask(logits, (224, 224)))
            m, _ = eng.validate_step(img, tgt)
            assert int((pred.long() == tgt).sum()) == int(round(float(m[2])))
            big, over = eng.predict(img, size=(301, 517), encode=FR.encode_table("endovis2017" if C == 8 else "binary255", C),
                                    frames=torch.zeros((2, 301, 517, 3), dtype=torch.uint8, device=dev))
            assert tuple(big.shape) == (2, 301, 517) and tuple(over.shape) == (2, 301, 517, 3)
            eng.seg_decoder.eval()
            eng.predict(img)
            assert not eng.seg_decoder.training                 # restored to what it was, whichever that is
            eng.seg_decoder.train()
            eng = _engine(head, dev, C)                         # the validate_step above is not part of the comparison
            eng.seg_decoder.train()
            eng.predict(img)
        losses[with_predict] = eng.train_step(img, tgt).clone()
    assert torch.equal(losses[False], losses[True]), "a predict call changed the following train_step"


# ---- 5. entry point -----------------------------------------------------------------------------------------------------------
def _write_frame(rng, d, name, hw):
    """One frame / instruments mask pair: blocky labels 0..7, the frame's colour follows the label."""
    lab = rng.integers(0, 8, (hw[0] // 32, hw[1] // 32)).repeat(32, 0).repeat(32, 1)
    pal = (np.arange(8)[:, None] * np.array([[29, 71, 113]])) % 256
    img = np.clip(pal[lab] + rng.integers(-12, 13, hw + (3,)), 0, 255).astype(np.uint8)
    Image.fromarray(img).save(os.path.join(d, "images", name))
    Image.fromarray((lab * 32).astype(np.uint8)).save(os.path.join(d, "instruments_masks", name))


def _two_size_tree(root, split, seq_sizes, n, seed):
    rng = np.random.default_rng(seed)
    for s, hw in seq_sizes.items():
        d = os.path.join(root, split, f"instrument_dataset_{s}")
        os.makedirs(os.path.join(d, "images"))
        os.makedirs(os.path.join(d, "instruments_masks"))
        for k in range(n):
            _write_frame(rng, d, f"frame{k:03d}.png", hw)


def _read_tree(d):
    return {os.path.relpath(os.path.join(r, f), d): open(os.path.join(r, f), "rb").read() for r, _, fs in os.walk(d) for f in fs}


def test_predict_entry_point(dev, tmp_path):
    from adaptersis_amd import predict as P
    from adaptersis_amd import train as T
    from adaptersis_amd import train_multi_class as TMC
    root, out = str(tmp_path / "ev17"), str(tmp_path / "out")
    _two_size_tree(root, "Train", {1: (256, 320)}, 8, seed=0)
    _two_size_tree(root, "Test", {1: (256, 320), 2: (192, 288)}, 5, seed=1)          # two native sizes, short last batches
    model_args = ["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4", "--num_workers", "0", "--output_dir", out]
    T._ENGINES.clear(); T._AUGMENTERS.clear()
    torch.manual_seed(0)
    TMC.train_seg(TMC.get_args_parser().parse_args(model_args + ["--lr", "0.08", "--data_path", root, "--epochs", "1",
                                                                 "--num_classes", "8"]))
    (eng_tr,) = T._ENGINES.values()                  # the engine that was trained and validated
    T._ENGINES.clear()

    def pargs(pred, *extra):
        return P.get_args_parser().parse_args(model_args + ["--head", "mla", "--num_classes", "8", "--input", root, "--dataset",
                                                            "endovis2017", "--split", "Test", "--encode", "endovis2017", "--overlay",
                                                            "--masks", "--pred_dir", str(tmp_path / pred), *extra])
    # the checkpoint of the reference's flow holds the decoder only: without the training process's seed it is refused
    with pytest.raises(ValueError, match=r"holds no 'backbone_encoder', 'cross_vit', 'cross_cnn'.*--seed"):
        P.predict_seg(pargs("pred0"))
    assert not os.path.exists(tmp_path / "pred0")
    args = pargs("pred1", "--seed", "0")
    res = P.predict_seg(args)
    rels = [f"instrument_dataset_{s}/images/frame{k:03d}.png" for s in (1, 2) for k in range(5)]
    assert sorted(res["files"]) == rels
    got = _read_tree(args.pred_dir)
    assert sorted(got) == sorted(rels + [r[:-4] + "_overlay.png" for r in rels] + ["metrics.json"])
    native = {1: (256, 320), 2: (192, 288)}
    masks = {}
    for r in rels:
        im = Image.open(os.path.join(args.pred_dir, r))
        hw = native[int(r.split("/")[0].rsplit("_", 1)[1])]
        assert im.mode == "L" and im.size == (hw[1], hw[0])
        masks[r] = np.array(im)
        assert set(np.unique(masks[r]).tolist()) <= set(range(0, 256, 32))
        ov = Image.open(os.path.join(args.pred_dir, r[:-4] + "_overlay.png"))
        assert ov.mode == "RGB" and ov.size == im.size

    # the same batches through engine.predict directly, on the engine that train_seg trained and validated (not a rebuilt one):
    # sizes ascending, sorted paths inside a size, 4 per batch
    eng = P.build_engine(args)
    enc = FR.encode_table("endovis2017", 8)
    for batch in ([f"instrument_dataset_2/images/frame{k:03d}.png" for k in range(4)], ["instrument_dataset_2/images/frame004.png"],
                  [f"instrument_dataset_1/images/frame{k:03d}.png" for k in range(4)], ["instrument_dataset_1/images/frame004.png"]):
        frames = torch.from_numpy(np.stack([np.array(Image.open(os.path.join(root, "Test", r)).convert("RGB")) for r in batch])).to(dev)
        small, _ = ops.frame_resize(frames, None, 224)
        inp, _ = T._to_device_batch(small, torch.zeros(small.shape[:3], dtype=torch.uint8, device=dev), train=False)
        m, ov = eng_tr.predict(inp, size=tuple(frames.shape[1:3]), encode=enc, frames=frames, alpha=FR.default_alpha(8, 0.5))
        # the engine predict builds from the checkpoint + seed is the trained one: same masks at the network size, and their
        # agreement with the labels is validate_step's correct-pixel count on the training engine
        raw = torch.from_numpy(np.stack([np.array(Image.open(os.path.join(root, "Test", r.replace("/images/", "/instruments_masks/"))))
                                         for r in batch])).to(dev)
        _, small_lab = ops.frame_resize(None, raw, 224, FR.LUT_MULTI)
        at_net = eng.predict(inp)
        assert torch.equal(at_net, eng_tr.predict(inp))
        vm, _ = eng_tr.validate_step(inp, small_lab.long())
        assert int((at_net == small_lab).sum()) == int(round(float(vm[2])))
        for k, r in enumerate(batch):
            assert np.array_equal(m[k].cpu().numpy(), masks[r]), r
            assert np.array_equal(ov[k].cpu().numpy(), np.array(Image.open(os.path.join(args.pred_dir, r[:-4] + "_overlay.png")))), r

    # metrics.json against numpy on the written PNGs and the ground-truth files
    met = json.load(open(os.path.join(args.pred_dir, "metrics.json")))
    pred = np.concatenate([masks[r].reshape(-1) >> 5 for r in rels])
    gt = np.concatenate([np.array(Image.open(os.path.join(root, "Test", r.replace("/images/", "/instruments_masks/")))).reshape(-1) >> 5
                         for r in rels])
    want = _np_counts(pred, gt, 8)
    assert met["counts"] == want.tolist() and met["frames"] == 10
    ious = [want[c, 0] / (want[c, 1] + want[c, 2] - want[c, 0]) if want[c, 1] + want[c, 2] > want[c, 0] else None for c in range(8)]
    assert all((a is None and b is None) or abs(a - b) < 1e-12 for a, b in zip(met["per_class_iou"], ious))
    assert abs(met["mean_iou"] - np.mean([v for v in ious if v is not None])) < 1e-12
    assert abs(met["pixel_accuracy"] - float((pred == gt).mean())) < 1e-12

    # a second run writes the same bytes
    args2 = pargs("pred2", "--seed", "0")
    P.predict_seg(args2)
    assert _read_tree(args2.pred_dir) == got

    # frames only (no --masks, no --overlay): the ground truth is not opened, no metrics.json, the same mask bytes
    a3 = P.get_args_parser().parse_args(model_args + ["--head", "mla", "--num_classes", "8", "--input", root, "--dataset", "endovis2017",
                                                      "--split", "Test", "--encode", "endovis2017", "--pred_dir", str(tmp_path / "pred4"),
                                                      "--seed", "0"])
    r3 = P.predict_seg(a3)
    assert r3["metrics"] is None
    assert _read_tree(a3.pred_dir) == {r: got[r] for r in rels}

    # wrong class count / head, missing checkpoint: errors that name the file and the key
    ck = os.path.join(out, "checkpoint.pth.tar")
    with pytest.raises(ValueError, match=r"checkpoint\.pth\.tar.*'cls_3\.weight'") as e:
        P.predict_seg(pargs("pred3", "--seed", "0", "--num_classes", "2", "--encode", "index"))
    assert ck in str(e.value)
    with pytest.raises(FileNotFoundError, match="nowhere"):
        P.predict_seg(pargs("pred3", "--seed", "0", "--checkpoint", str(tmp_path / "nowhere.pth.tar")))
    assert not os.path.exists(tmp_path / "pred3")
