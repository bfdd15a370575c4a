"""GPU: the strong view in the training path — ``train._to_device_batch(strong=, strong_apply=)`` and a ``train_step`` on its
batch, on the tiny engine of tests/test_gpu_mean_teacher.py (``vit_tiny_test``, 224 x 224, B = 3): the teacher's view is the tensor
in front of the strong stage (or the geometry-only one with ``weak``), bit for bit what the call without ``strong`` returns; the
labelled rows stay themselves under an apply mask; the step runs, with ClassMix too; without the keyword nothing is drawn, loaded
or launched; and the flags of the training script."""
import json

import numpy as np
import pytest
import torch

from adaptersis_amd import _lib_strong, ops
from adaptersis_amd import train as T
from adaptersis_amd.tools.augment import TrainAugment
from tests.test_gpu_mean_teacher import _seg_engine

pytestmark = pytest.mark.gpu

EMA = dict(ema_decay=0.5, ema_warmup=False)
CFG = dict(jitter_p=1.0, blur_p=1.0)        # every sample has a draw
B, S = 3, 224


def _u8():
    g = torch.Generator().manual_seed(3)
    img = torch.randint(0, 256, (B, S // 4, S // 4, 3), generator=g, dtype=torch.uint8).repeat_interleave(4, 1).repeat_interleave(4, 2)
    msk = (torch.rand((B, S // 4, S // 4), generator=g) > 0.6).to(torch.uint8).repeat_interleave(4, 1).repeat_interleave(4, 2)
    return img.contiguous(), msk.contiguous()


def _batch(**kw):
    """a training batch under the seed of a fresh process"""
    T._AUGMENTERS.clear()
    try:
        return T._to_device_batch(*_u8(), train=True, **kw)
    finally:
        T._AUGMENTERS.clear()


@pytest.fixture(scope="module")
def views(dev):
    """computed once: the plain batch, the strong one, both with ``weak``, and the strong one under an apply mask"""
    return dict(plain=_batch(), strong=_batch(strong=CFG), weak=_batch(weak=True), weak_strong=_batch(weak=True, strong=CFG),
                masked=_batch(strong=CFG, strong_apply=[False, True, False]))


def test_the_teachers_view_is_the_tensor_in_front_of_the_strong_stage(dev, views):
    (px, py), (x, y, tx) = views["plain"], views["strong"]
    assert torch.equal(tx, px) and torch.equal(y, py)                          # the call without ``strong``, draw for draw
    twin = TrainAugment(size=S, seed=1000, strong=CFG)                         # the augmenter _to_device_batch builds on rank 0
    params = twin.draw(B)
    assert all(p["strong"] is not None for p in params)
    assert torch.equal(x, ops.strong_view(tx, twin.strong_tables(params, dev))) and not torch.equal(x, tx)
    assert x.data_ptr() != tx.data_ptr() and float(x.min()) >= 0.0 and float(x.max()) <= 1.0


def test_with_weak_the_teacher_sees_the_geometry_only_view(dev, views):
    (x, y, tx), (wx, wy, wtx), (sx, sy, _) = views["weak_strong"], views["weak"], views["strong"]
    assert torch.equal(tx, wtx) and torch.equal(y, wy)                         # as today
    assert torch.equal(x, sx) and not torch.equal(x, wx)                       # the student's view is the strong one either way
    assert torch.equal(ops.strong_view(wx, TrainAugment(size=S, seed=1000, strong=CFG).strong_tables(
        TrainAugment(size=S, seed=1000, strong=CFG).draw(B), dev)), x)


def test_an_apply_mask_from_a_labelled_list(dev, views):
    labelled = [True, False, True]
    (x, y, tx), (sx, _, stx) = views["masked"], views["strong"]
    assert torch.equal(tx, stx)
    for b, l in enumerate(labelled):
        assert torch.equal(x[b], tx[b] if l else sx[b]), b
    assert T._LAST_STRONG["applied"] is not None
    with pytest.raises(ValueError, match="strong_apply has 2 entries"):
        _batch(strong=CFG, strong_apply=[True, False])


def test_only_training_uint8_batches(dev, views):
    T._AUGMENTERS.clear()
    val = T._to_device_batch(*_u8(), train=False, strong=CFG)
    ref = T._to_device_batch(*_u8(), train=False)
    T._AUGMENTERS.clear()
    assert len(val) == 2 and torch.equal(val[0], ref[0]) and torch.equal(val[1], ref[1])
    f = torch.rand(2, 3, 32, 32)
    x, y, tx = T._to_device_batch(f, torch.zeros(2, 32, 32, dtype=torch.long), train=True, strong=CFG)
    assert tx is x and torch.equal(x.cpu(), f) and T._LAST_STRONG["applied"] == 0.0   # a float batch is left alone, as for weak
    _batch(strong=CFG)
    assert T._LAST_STRONG["applied"] == 1.0
    _batch(strong=CFG, strong_apply=[True, False, False])
    assert T._LAST_STRONG["applied"] == pytest.approx(1.0 / 3.0)


@pytest.mark.parametrize("mix", [None, "classmix"])
def test_a_step_on_the_strong_batch(dev, views, mix):
    x, y, tx = views["strong"]
    eng = _seg_engine(dev, teacher="ema", **EMA, **({} if mix is None else {"mix": mix, "mix_seed": 1}))
    taps = {}
    for _ in range(2):
        loss = eng.train_step(x, y, taps, tx)
        assert bool(torch.isfinite(loss)) and eng.optimizer.skipped_steps == 0
    assert bool(torch.isfinite(taps["loss_kd"])) and bool(torch.isfinite(taps["logits"]).all())
    if mix is not None:
        assert eng.last_mix_pasted is not None
    semi = _seg_engine(dev, teacher="ema", **EMA)
    mx, my, mtx = views["masked"]
    assert bool(torch.isfinite(semi.train_step(mx, my, None, mtx, labelled=[True, False, True])))


def test_without_the_keyword_nothing_is_drawn_loaded_or_launched(dev, views, monkeypatch):
    monkeypatch.setattr(_lib_strong, "_dlib", None)                            # as in a process that never opened the library
    calls = []
    monkeypatch.setattr(ops, "strong_view", lambda *a, **k: calls.append(a))
    a, b = _batch(), _batch(strong=None, strong_apply=None)
    assert len(a) == len(b) == 2 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], views["plain"][0])
    w = _batch(weak=True, strong=None)
    assert torch.equal(w[0], views["weak"][0]) and torch.equal(w[2], views["weak"][2])
    T._AUGMENTERS.clear()
    T._to_device_batch(*_u8(), train=True)
    assert T._AUGMENTERS[S].strong is None and T._AUGMENTERS[S].strong_rng is None
    T._AUGMENTERS.clear()
    one, two = _seg_engine(dev), _seg_engine(dev)
    ta, tb = {}, {}
    la, lb = one.train_step(*a, ta), two.train_step(*b, tb)
    assert torch.equal(ta["logits"], tb["logits"]) and torch.equal(la, lb)
    assert not calls and not _lib_strong.loaded()


# ---- the scripts ---------------------------------------------------------------------------------------------------------------------
def test_scripts(dev, tmp_path, monkeypatch):
    from PIL import Image
    r = np.random.RandomState(0)
    for split, n in (("training", 8), ("validation", 4)):
        (tmp_path / "data" / "images" / split).mkdir(parents=True)
        (tmp_path / "data" / "annotations" / split).mkdir(parents=True)
        for i in range(n):
            img = (r.randint(0, 256, (56, 56, 3)).astype(np.uint8)).repeat(4, 0).repeat(4, 1)
            msk = ((r.random_sample((56, 56)) > 0.7).astype(np.uint8) * 255).repeat(4, 0).repeat(4, 1)
            Image.fromarray(img).save(tmp_path / "data" / "images" / split / f"f{i:03d}.png")
            Image.fromarray(msk).save(tmp_path / "data" / "annotations" / split / f"f{i:03d}.png")
    common = ["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4", "--epochs", "1", "--lr", "0.05", "--data_path",
              str(tmp_path / "data"), "--num_workers", "0", "--train_adapters", "--train_encoder", "--ema_decay", "0.5", "--distill_teacher", "ema",
              "--unlabelled_path", "synthetic", "--unlabelled_per_batch", "4"]

    def run(out, *flags):
        T._ENGINES.clear(); T._AUGMENTERS.clear()
        try:
            stats = T.train_seg(T.get_args_parser().parse_args(common + ["--output_dir", str(tmp_path / out)] + list(flags)))
            (eng,) = T._ENGINES.values()
            return eng, stats, [json.loads(line) for line in open(tmp_path / out / "log.txt")]
        finally:
            T._ENGINES.clear(); T._AUGMENTERS.clear()

    seen = []
    real = ops.strong_view
    monkeypatch.setattr(ops, "strong_view", lambda x, tables, *a, **k: (seen.append(tables["st_host"]["st_apply"].tolist()), real(x, tables, *a, **k))[1])
    eng, stats, log = run("unl", "--aug_strong", "--aug_strong_on", "unlabelled", "--aug_strong_blur", "1.0")
    assert eng.aug_strong == {"blur_p": 1.0} and eng.aug_strong_on == "unlabelled" and eng.optimizer._steps == 2
    assert seen == [[0, 0, 0, 0, 1, 1, 1, 1]] * 2                               # the labelled list became the apply mask; never validation
    assert log[0]["train_strong_applied"] == 0.5 and np.isfinite(stats["train_loss"]) and np.isfinite(stats["test_loss"])
    del seen[:]
    eng, stats, log = run("all", "--aug_strong", "--mix", "classmix")
    assert eng.aug_strong == {} and eng.aug_strong_on == "all" and seen == [[1] * 8] * 2
    assert 0.5 < log[0]["train_strong_applied"] <= 1.0 and "train_mix_pasted" in log[0] and np.isfinite(stats["train_loss"])
    del seen[:]
    eng, stats, log = run("plain")
    assert eng.aug_strong is None and not seen and "train_strong_applied" not in log[0]
