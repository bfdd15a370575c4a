"""GPU: the multi-class entry point (`adaptersis_amd.train_multi_class` = reference `train_multi_class.py`) on EndoVis-style PNG
trees: soft-IoU training with ch_iou / isi_iou validation, checkpoint + --evaluate, the binary EndoVis2018 and synthetic runs,
per-batch metrics against segloss.iou_multi on the logits, and the device and host resize routes giving the same batch."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from adaptersis_amd import ops
from adaptersis_amd import train as T
from adaptersis_amd import train_multi_class as TMC
from adaptersis_amd.segloss import iou_multi

pytestmark = pytest.mark.gpu


def _frame_pair(rng, hw, n_classes):
    """Blocky labels; the frame's colour follows the label, so the task is learnable in a few steps."""
    g = rng.integers(0, n_classes, (hw[0] // 32, hw[1] // 32))
    lab = g.repeat(32, 0).repeat(32, 1)
    pal = (np.arange(n_classes)[:, None] * np.array([[29, 71, 113]])) % 256
    img = np.clip(pal[lab] + rng.integers(-12, 13, hw + (3,)), 0, 255).astype(np.uint8)
    return img, lab


def _endovis2017(root, split, seqs, n, hw=(256, 320), seed=0):
    rng = np.random.default_rng(seed)
    for s in seqs:
        d = os.path.join(root, split, f"instrument_dataset_{s}")
        os.makedirs(os.path.join(d, "images"), exist_ok=True)
        os.makedirs(os.path.join(d, "instruments_masks"), exist_ok=True)
        for k in range(n):
            img, lab = _frame_pair(rng, hw, 8)
            Image.fromarray(img).save(os.path.join(d, "images", f"frame{k:03d}.png"))
            Image.fromarray((lab * 32).astype(np.uint8)).save(os.path.join(d, "instruments_masks", f"frame{k:03d}.png"))


def _endovis2018(root, split, seqs, n, hw=(256, 320), seed=0):
    rng = np.random.default_rng(seed)
    for s in seqs:
        d = os.path.join(root, split, f"seq_{s}")
        os.makedirs(os.path.join(d, "images"), exist_ok=True)
        os.makedirs(os.path.join(d, "binary_masks"), exist_ok=True)
        for k in range(n):
            img, lab = _frame_pair(rng, hw, 2)
            Image.fromarray(img).save(os.path.join(d, "images", f"f{k:03d}.png"))
            Image.fromarray((lab * 255).astype(np.uint8)).save(os.path.join(d, "binary_masks", f"f{k:03d}.png"))


def _args(root, out, *extra):
    return TMC.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4",
                                             "--lr", "0.08", "--data_path", str(root), "--num_workers", "0",
                                             "--output_dir", str(out), *extra])


def test_multi_class_run_checkpoint_and_evaluate(dev, tmp_path):
    root = tmp_path / "ev17"
    _endovis2017(str(root), "Train", (1, 2), 8, seed=0)
    _endovis2017(str(root), "Test", (1,), 4, seed=1)
    args = _args(root, tmp_path / "out", "--epochs", "2", "--num_classes", "8")
    T._ENGINES.clear(); T._AUGMENTERS.clear()
    torch.manual_seed(0)
    TMC.train_seg(args)
    lines = [json.loads(l) for l in open(tmp_path / "out" / "log.txt")]
    assert len(lines) == 2
    assert {"train_loss", "test_loss", "test_acc1", "test_dice", "test_ch_iou", "test_isi_iou", "epoch"} <= set(lines[0])
    assert lines[1]["train_loss"] < lines[0]["train_loss"]
    assert 0.0 <= lines[1]["test_ch_iou"] <= 1.0 and 0.0 <= lines[1]["test_isi_iou"] <= 1.0
    ck = torch.load(tmp_path / "out" / "checkpoint.pth.tar", map_location="cpu")
    assert set(ck) == {"epoch", "state_dict", "optimizer", "scheduler", "best_acc"} and ck["epoch"] == 2
    assert all(k.startswith("module.") for k in ck["state_dict"])
    (eng,) = T._ENGINES.values()
    assert eng.num_classes == 8 and eng.loss_kind == "iou" and eng.is_mla
    assert ck["state_dict"]["module.cls_3.weight"].shape[0] == 8

    # per-batch metrics: the counts of the validation kernel against iou_multi on argmax of the resized logits
    ds_tr, ds_val, collate = TMC.open_datasets(args)
    inp, target, _ = collate([ds_val[i] for i in range(4)])
    inp, target = T._to_device_batch(inp, target, train=False)
    m, dloss, counts = eng.validate_step(inp, target, None, with_counts=True)
    was = eng.seg_decoder.training
    eng.seg_decoder.eval()
    with torch.no_grad():
        logits = eng.eval_logits(inp)
    eng.seg_decoder.train(was)
    pred = ops.resize_bilinear_fwd(logits, target.shape[1], target.shape[2]).argmax(-1).cpu().numpy()
    tgt = target.cpu().numpy()
    assert abs(iou_multi.ch_iou_from_counts(counts) - iou_multi.ch_iou(tgt, pred)) < 1e-3
    assert abs(iou_multi.isi_iou_from_counts(counts) - iou_multi.isi_iou(tgt, pred)) < 1e-3

    T._ENGINES.clear()
    args.evaluate = True
    torch.manual_seed(0)
    ev = TMC.train_seg(args)
    for k in ("acc1", "ch_iou", "isi_iou", "dice"):
        assert abs(ev[k] - lines[1][f"test_{k}"]) < 1e-5, k
    T._ENGINES.clear()


def test_binary_endovis2018_run(dev, tmp_path):
    root = tmp_path / "ev18"
    _endovis2018(str(root), "Train", (1, 3), 4)
    _endovis2018(str(root), "Test", (2,), 4, seed=1)
    args = _args(root, tmp_path / "out", "--epochs", "1", "--num_classes", "2", "--dataset", "endovis2018",
                 "--problem_type", "binary")
    T._ENGINES.clear()
    stats = TMC.train_seg(args)
    (eng,) = T._ENGINES.values()
    assert eng.num_classes == 2
    assert {"train_loss", "test_acc1", "test_ch_iou", "test_isi_iou"} <= set(stats)
    assert np.isfinite(stats["train_loss"]) and 0.0 <= stats["test_isi_iou"] <= 1.0
    T._ENGINES.clear()


def test_synthetic_run(dev, tmp_path):
    args = _args("synthetic", tmp_path, "--epochs", "1", "--num_classes", "8")
    T._ENGINES.clear()
    stats = TMC.train_seg(args)
    assert {"train_loss", "test_ch_iou", "test_isi_iou"} <= set(stats) and np.isfinite(stats["train_loss"])
    T._ENGINES.clear()


def test_resize_routes_give_the_same_device_batch(dev, tmp_path):
    root = tmp_path / "ev17"
    _endovis2017(str(root), "Train", (1,), 4)
    _endovis2017(str(root), "Test", (1,), 4, seed=1)
    got = {}
    for route in ("gpu", "host"):
        args = _args(root, tmp_path, "--resize_on", route)
        args.cross_test_path = args.data_path
        ds_tr, ds_val, collate = TMC.open_datasets(args)
        loader = torch.utils.data.DataLoader(ds_tr, batch_size=4, shuffle=False, collate_fn=collate)
        inp, target, _ = next(iter(loader))
        T._AUGMENTERS.clear()                                 # same augmentation draws for both routes
        got[route] = [T._to_device_batch(inp, target, train=False), T._to_device_batch(inp, target, train=True)]
    for (gi, gt), (hi, ht) in zip(got["gpu"], got["host"]):
        assert gi.dtype == torch.float32 and gi.shape == (4, 3, 224, 224) and gt.dtype == torch.int64
        assert torch.equal(gi, hi) and torch.equal(gt, ht)
    T._AUGMENTERS.clear()
