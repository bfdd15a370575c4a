"""GPU: mean-teacher training — ``SegEngine(teacher=...)`` on the tiny engine of tests/test_gpu_ema.py (``vit_tiny_test``, 224 x 224,
B = 3): the default builds nothing, the EMA teacher's maps are those of ``ema_weights()`` under the guard of ``predict``, the step is
the undistilled step with ``ops.consistency_loss`` added into the hard term's dz (weights equal bit for bit), the checkpoint
teacher, the ramp-up, every mode, and the flags of the training script."""
import copy
import json
import os

import pytest
import torch

from adaptersis_amd import _lib_consist, config, ops
from adaptersis_amd.backbones import engines as E
from adaptersis_amd.dinov2.models import vision_transformer as vits
from adaptersis_amd.optim import consistency_ramp
from adaptersis_amd.utils import weights as W

pytestmark = pytest.mark.gpu

ARCH = "vit_tiny_test"


def _seg_engine(dev, mode="train_adapters", **kw):
    from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
    from adaptersis_amd.backbones.decoders import FeatureDecoder
    from adaptersis_amd.backbones.encoders import FeatureEncoder
    feats = (128, 32, 16, 16, 8)
    D, depth, heads, ffn = W.VIT_CONFIGS[ARCH]
    model = vits.__dict__[ARCH](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0)
    model.load_state_dict(W.make_vit_state_dict(ARCH, layerscale="kernel"))
    enc = FeatureEncoder(embed_dim=D); enc.load_state_dict(W.make_encoder_state_dict(D))
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4); cv.load_state_dict(W.make_cavit_state_dict(D, mode="kernel"))
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25); cn.load_state_dict(W.make_cacnn_state_dict(D, mode="kernel"))
    dec = FeatureDecoder(embed_dim=D, num_classes=2, features=list(feats)); dec.load_state_dict(W.make_feature_decoder_state_dict(D, 2, features=feats))
    if mode == "train_adapters":
        kw.setdefault("train_encoder", True)
    return E.SegEngine(model.to(dev), enc.to(dev), cv.to(dev), cn.to(dev), dec.to(dev), lr=0.05, mode=mode, **kw)


def _batch(dev):
    img, tgt = W.synthetic_batch(3, 224)
    return img.to(dev), tgt.to(dev)


def _weights(eng):
    return [b.flat.clone() for b in eng.optimizer.buckets]


def _equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _buffers(eng):
    return [v.clone() for m in (eng.backbone_encoder, eng.seg_decoder) for v in m.buffers()]


def _guarded(eng, x):
    """the logits ``predict`` sees, written out: decoder in eval mode, the encoder's running statistics not updated, both restored"""
    enc = eng.backbone_encoder
    was, upd = eng.seg_decoder.training, enc.update_running_stats
    eng.seg_decoder.eval()
    enc.update_running_stats = False
    try:
        return eng.eval_logits(x)
    finally:
        eng.seg_decoder.train(was)
        enc.update_running_stats = upd


# ---- the default -------------------------------------------------------------------------------------------------------------------
def test_no_teacher_by_default(dev, monkeypatch):
    monkeypatch.setattr(_lib_consist, "_dlib", None)                           # as in a process that never opened the library
    plain = _seg_engine(dev)
    eng = _seg_engine(dev, teacher=None, distill_weight=3.0, distill_threshold=0.9, distill_flip=True)
    assert plain.teacher is None and eng.teacher is None and eng.distill_step == 0
    img, tgt = _batch(dev)
    for _ in range(2):
        taps = {}
        a, b = plain.train_step(img, tgt), eng.train_step(img, tgt, taps)
        assert torch.equal(a, b) and "loss_kd" not in taps and "teacher_logits" not in taps
    assert _equal(_weights(plain), _weights(eng))
    assert not _lib_consist.loaded() and eng.last_loss_kd is None and eng.distill_step == 0
    assert not hasattr(eng, "_consist_scratch")
    with pytest.raises(ValueError, match="teacher_inp without a teacher"):
        eng.train_step(img, tgt, None, img)
    with pytest.raises(ValueError, match="needs ema_decay"):
        _seg_engine(dev, teacher="ema")
    with pytest.raises(ValueError, match="teacher must be"):
        _seg_engine(dev, teacher="other")


def test_weight_zero_is_the_undistilled_step(dev):
    plain = _seg_engine(dev, ema_decay=0.5, ema_warmup=False)
    eng = _seg_engine(dev, ema_decay=0.5, ema_warmup=False, teacher="ema", distill_weight=0.0, distill_threshold=0.6)
    img, tgt = _batch(dev)
    for _ in range(2):
        taps = {}
        a, b = plain.train_step(img, tgt), eng.train_step(img, tgt, taps)
        assert torch.equal(a, b) and taps["distill_scale"] == 0.0 and float(taps["loss_kd"]) >= 0.0
    assert _equal(_weights(plain), _weights(eng)) and _equal(plain.ema.shadows, eng.ema.shadows)
    assert eng.distill_step == 2


# ---- the EMA teacher ---------------------------------------------------------------------------------------------------------------
def test_ema_teacher_maps_and_guard(dev):
    plain = _seg_engine(dev, ema_decay=0.5, ema_warmup=False)
    eng = _seg_engine(dev, ema_decay=0.5, ema_warmup=False, teacher="ema", distill_flip=True, distill_threshold=0.6)
    img, tgt = _batch(dev)
    plain.train_step(img, tgt)
    eng.train_step(img, tgt)
    # the first step's forward ran on the same weights: the running buffers moved exactly as in an undistilled step
    assert _equal(_buffers(plain), _buffers(eng))
    assert eng.backbone_encoder.update_running_stats is True and eng.seg_decoder.training and not eng.ema.swapped_in
    eng.train_step(img, tgt)                                                   # the average now differs from the live weights
    with eng.ema_weights():
        want = [_guarded(eng, img), _guarded(eng, img.flip(-1))]
    live = _guarded(eng, img)
    assert not torch.equal(want[0], live)
    bufs = _buffers(eng)
    taps = {}
    loss = eng.train_step(img, tgt, taps)
    assert len(taps["teacher_logits"]) == 2
    assert torch.equal(taps["teacher_logits"][0], want[0]) and torch.equal(taps["teacher_logits"][1], want[1])
    assert not eng.ema.swapped_in and eng.seg_decoder.training and eng.backbone_encoder.update_running_stats is True
    assert not _equal(bufs, _buffers(eng))                                     # the student's forward still moves them
    assert torch.isfinite(loss) and eng.optimizer.skipped_steps == 0 and eng.ema.updates == 3
    assert eng.last_loss_kd is taps["loss_kd"] and eng.last_kd_kept is taps["kd_kept"]
    assert 0 <= int(taps["kd_kept"]) <= tgt.numel()
    # teacher_inp: the teacher sees another rendering of the batch
    with eng.ema_weights():
        other = _guarded(eng, (img * 0.9).contiguous())
    taps = {}
    eng.train_step(img, tgt, taps, teacher_inp=(img * 0.9).contiguous())
    assert torch.equal(taps["teacher_logits"][0], other)


def _compose(dev, monkeypatch, a_kw, b_kw, steps=2):
    """engine A steps with a teacher; engine B, without one, steps with ``loss_and_dz`` wrapped to add ``ops.consistency_loss`` on
    A's recorded maps at S lambda_t: the same weights bit for bit"""
    A, B = _seg_engine(dev, **a_kw), _seg_engine(dev, **b_kw)
    img, tgt = _batch(dev)
    original = E.loss_and_dz
    flips = [False, True] if A.distill_flip else [False]
    for t in range(steps):
        taps = {}
        monkeypatch.setattr(E, "loss_and_dz", original)
        la = A.train_step(img, tgt, taps)
        lam = taps["distill_scale"]
        assert lam == A.distill_weight * consistency_ramp(t, A.distill_rampup)
        rec = {}

        def wrapped(engine, logits, target, S):
            loss, dz = original(engine, logits, target, S)
            kd, kept, _ = ops.consistency_loss(logits, taps["teacher_logits"], target, flips=flips, temperature=A.distill_temperature,
                                               threshold=A.distill_threshold, grad_scale=S * lam, dz=dz)
            rec.update(hard=loss.clone(), kd=kd, kept=kept, logits=logits)
            return loss, dz

        monkeypatch.setattr(E, "loss_and_dz", wrapped)
        B.train_step(img, tgt)
        monkeypatch.setattr(E, "loss_and_dz", original)
        assert torch.equal(rec["logits"], taps["logits"])
        assert torch.equal(taps["loss_hard"], rec["hard"]) and torch.equal(taps["loss_kd"], rec["kd"])
        assert torch.equal(taps["kd_kept"], rec["kept"])
        assert torch.equal(taps["loss"], taps["loss_hard"] + lam * taps["loss_kd"]) and torch.equal(la.view(1), taps["loss"].view(1))
        # ... and a direct call of the op on the taps
        kd, kept, _ = ops.consistency_loss(taps["logits"], taps["teacher_logits"], tgt, flips=flips, temperature=A.distill_temperature,
                                           threshold=A.distill_threshold)
        assert torch.equal(kd, taps["loss_kd"]) and torch.equal(kept, taps["kd_kept"])
        assert _equal(_weights(A), _weights(B)), f"step {t}"
    return A, B


def test_step_is_the_hard_step_plus_the_consistency_term(dev, monkeypatch):
    ema = dict(ema_decay=0.5, ema_warmup=False)
    A, B = _compose(dev, monkeypatch, dict(teacher="ema", distill_weight=0.7, distill_temperature=2.0, distill_threshold=0.55,
                                           distill_flip=True, distill_rampup=3, **ema), dict(ema))
    assert _equal(A.ema.shadows, B.ema.shadows) and A.distill_step == 2
    plain = _seg_engine(dev, **ema)
    img, tgt = _batch(dev)
    for _ in range(2):
        plain.train_step(img, tgt)
    assert not _equal(_weights(A), _weights(plain))                            # the term does reach the weights


# ---- the ramp ----------------------------------------------------------------------------------------------------------------------
def test_ramp_and_step_count(dev):
    eng = _seg_engine(dev, ema_decay=0.5, teacher="ema", distill_weight=2.0, distill_rampup=3)
    img, tgt = _batch(dev)
    scales = []
    for _ in range(4):
        taps = {}
        eng.train_step(img, tgt, taps)
        scales.append(taps["distill_scale"])
    assert scales == [2.0 * consistency_ramp(t, 3) for t in range(4)] and scales[3] == 2.0 and scales[0] < scales[1] < scales[2] < 2.0
    assert eng.distill_step == 4


# ---- every mode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["reference_exact", "train_adapters", "lora"])
def test_modes(dev, mode):
    kw = {"reference_exact": dict(mode="reference_exact"), "train_adapters": dict(),
          "lora": dict(train_backbone=True, lora_rank=4)}[mode]
    eng = _seg_engine(dev, ema_decay=0.5, teacher="ema", distill_threshold=0.6, distill_flip=True, **kw)
    img, tgt = _batch(dev)
    taps = {}
    loss = eng.train_step(img, tgt, taps)
    assert torch.isfinite(loss) and torch.isfinite(taps["loss_kd"]).all() and eng.optimizer.skipped_steps == 0
    assert loss.dim() == 0 and taps["kd_kept"].dtype == torch.int32 and not eng.ema.swapped_in


# ---- the weak view -----------------------------------------------------------------------------------------------------------------
def test_weak_view_of_a_uint8_batch(dev):
    """--distill_weak: the teacher's rendering is the student's geometry under neutral photometrics, and asking for it draws nothing"""
    from adaptersis_amd import train as T
    from adaptersis_amd.tools.augment import TrainAugment, weak_params
    g = torch.Generator().manual_seed(3)
    batches = [(torch.randint(0, 256, (4, 64, 64, 3), generator=g, dtype=torch.uint8),
                torch.randint(0, 2, (4, 64, 64), generator=g, dtype=torch.uint8)) for _ in range(2)]
    T._AUGMENTERS.clear()
    weak = [T._to_device_batch(i, m, train=True, weak=True) for i, m in batches]
    T._AUGMENTERS.clear()
    plain = [T._to_device_batch(i, m, train=True) for i, m in batches]
    T._AUGMENTERS.clear()
    twin = TrainAugment(size=64, seed=1000)                                    # the augmenter _to_device_batch builds on rank 0
    for (x, y, tx), (a, b), (i, m) in zip(weak, plain, batches):
        assert torch.equal(x, a) and torch.equal(y, b)                         # the run without the flag, draw for draw
        params = twin.draw(4)
        want, wy = twin(i.to(dev), m.to(dev), weak_params(params))
        assert torch.equal(tx, want) and torch.equal(wy, y)                    # same geometry: the labels are the student's
        assert tx.shape == x.shape and not torch.equal(tx, x)
    f = torch.rand(2, 3, 32, 32)
    x, y, tx = T._to_device_batch(f, torch.zeros(2, 32, 32, dtype=torch.long), train=True, weak=True)
    assert tx is x                                                             # no photometric stage on a float batch


# ---- the scripts -------------------------------------------------------------------------------------------------------------------
COMMON =["--arch", ARCH, "--imsize", "224", "--batch_size_per_gpu", "4"]
TRAIN = ["--epochs", "1", "--lr", "0.05", "--data_path", "synthetic", "--train_adapters", "--train_encoder"]


def _run(T, out, *flags):
    T._ENGINES.clear()
    stats = T.train_seg(T.get_args_parser().parse_args(COMMON + TRAIN + ["--output_dir", str(out)] + list(flags)))
    (eng,) = T._ENGINES.values()
    T._ENGINES.clear()
    return eng, stats


def test_scripts(dev, tmp_path):
    from adaptersis_amd import train as T
    run, second, plain = tmp_path / "mt", tmp_path / "second", tmp_path / "plain"
    mt = ["--ema_decay", "0.9", "--distill_teacher", "ema", "--distill_threshold", "0.6", "--distill_flip"]
    eng, stats = _run(T, run, *mt)
    steps = eng.optimizer._steps
    assert eng.teacher == "ema" and eng.distill_flip and eng.distill_threshold == 0.6 and eng.distill_step == steps > 1
    log = [json.loads(line) for line in open(run / "log.txt")]
    assert "train_loss_kd" in log[0] and 0.0 <= log[0]["train_kd_kept"] <= 1.0 and log[0]["train_loss_kd"] >= 0.0
    path = str(run / "checkpoint.pth.tar")
    ck = torch.load(path, map_location="cpu")
    assert ck["distill"] == {"step": steps}
    # a resume restores the step (epoch 1 of 1 is done: nothing trains)
    resumed, _ = _run(T, run, *mt, "--distill_rampup", "40")
    assert resumed.distill_step == steps and resumed.distill_rampup == 40
    # a checkpoint teacher: the maps of predict's guard on the engine that wrote the file, live and averaged
    img, tgt = _batch(dev)
    args = T.get_args_parser().parse_args(COMMON + TRAIN + ["--output_dir", str(second), "--distill_teacher", path])
    teacher = T.build_teacher(args, "feature", 2, dev, resumed.model)
    assert teacher.model is resumed.model and teacher.seg_decoder is not resumed.seg_decoder
    assert torch.equal(_guarded(teacher, img), _guarded(resumed, img))
    args_ema = copy.copy(args)
    args_ema.distill_teacher_ema = True
    with resumed.ema_weights():
        averaged = _guarded(resumed, img)
    assert torch.equal(_guarded(T.build_teacher(args_ema, "feature", 2, dev, resumed.model), img), averaged)
    own = copy.copy(args)
    own.optimize_backbone = True                                               # the student steps its ViT: the teacher owns one
    assert T.build_teacher(own, "feature", 2, dev, resumed.model).model is not resumed.model
    student = _seg_engine(dev, teacher=teacher, distill_threshold=0.6)
    before = _weights(teacher)
    taps = {}
    student.train_step(img, tgt, taps)
    assert torch.equal(taps["teacher_logits"][0], _guarded(teacher, img)) and _equal(before, _weights(teacher))   # never stepped
    assert teacher.optimizer._steps == 0 and "teacher" not in dict(student.named_modules())
    # the second run: that checkpoint's averaged weights as a frozen teacher
    eng2, _ = _run(T, second, "--distill_teacher", path, "--distill_teacher_ema", "--distill_weight", "0.5")
    assert isinstance(eng2.teacher, E.SegEngine) and eng2.teacher.model is eng2.model and eng2.ema is None
    ck2 = torch.load(second / "checkpoint.pth.tar", map_location="cpu")
    assert ck2["distill"] == {"step": eng2.optimizer._steps} and "ema" not in ck2
    assert "train_loss_kd" in open(second / "log.txt").read()
    # without the flags: no key, no meter
    eng3, _ = _run(T, plain)
    ck3 = torch.load(plain / "checkpoint.pth.tar", map_location="cpu")
    assert eng3.teacher is None and "distill" not in ck3 and set(ck3) == set(ck2) - {"distill"}
    assert "loss_kd" not in open(plain / "log.txt").read()
    # what cannot work is refused with its message before anything is built
    with pytest.raises(ValueError, match="--distill_teacher ema needs --ema_decay"):
        T.train_seg(argparse_namespace(T, plain, "--distill_teacher", "ema"))


def argparse_namespace(T, out, *flags):
    """the namespace of a command line the parser itself would refuse"""
    ns = T.get_args_parser().parse_args(COMMON + TRAIN + ["--output_dir", str(out)])
    it = iter(flags)
    for f in it:
        setattr(ns, f.lstrip("-"), next(it))
    return ns
