"""GPU: batch mixing in the training step — ``SegEngine(mix=...)`` on the tiny engine of tests/test_gpu_mean_teacher.py
(``vit_tiny_test``, 224 x 224, B = 3): the default and ``mix_p = 0`` build, draw for the device and load nothing; without a teacher the
step is the plain step on ``ops.mix_batch`` of the drawn tables (weights equal bit for bit); with the EMA teacher the teacher sees
the unmixed batch and the step is the teacher-less step on the mixed batch with ``ops.consistency_loss(..., mix=)`` added into the
hard term's dz; every mode; the draw after a resume; the flags of the training script."""
import json

import pytest
import torch

from adaptersis_amd import _lib_mix, ops
from adaptersis_amd.backbones import engines as E
from adaptersis_amd.optim import consistency_ramp
from adaptersis_amd.tools.mix import MixSampler
from tests.test_gpu_mean_teacher import COMMON, TRAIN, _batch, _equal, _run, _seg_engine, _weights, argparse_namespace

pytestmark = pytest.mark.gpu

EMA = dict(ema_decay=0.5, ema_warmup=False)


def _same_tables(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---- the default -------------------------------------------------------------------------------------------------------------------
def test_no_mixing_by_default_and_at_p_zero(dev, monkeypatch):
    monkeypatch.setattr(_lib_mix, "_dlib", None)                               # as in a process that never opened the library
    plain, off, never = _seg_engine(dev), _seg_engine(dev, mix=None, mix_p=0.3, mix_seed=5), _seg_engine(dev, mix="classmix", mix_p=0.0)
    assert plain.mix_sampler is None and off.mix_sampler is None and never.mix_sampler is not None
    img, tgt = _batch(dev)
    for _ in range(2):
        taps_off, taps_never = {}, {}
        a, b, c = plain.train_step(img, tgt), off.train_step(img, tgt, taps_off), never.train_step(img, tgt, taps_never)
        assert torch.equal(a, b) and torch.equal(a, c)
        assert not any(k.startswith("mix_") for k in list(taps_off) + list(taps_never))
    assert _equal(_weights(plain), _weights(off)) and _equal(_weights(plain), _weights(never))
    assert not _lib_mix.loaded() and off.mix_step == 0 and never.mix_step == 2
    assert off.last_mix_pasted is None and never.last_mix_pasted is None
    with pytest.raises(ValueError, match="mix must be one of"):
        _seg_engine(dev, mix="mixup")
    with pytest.raises(ValueError, match="mix_p"):
        _seg_engine(dev, mix="cutmix", mix_p=1.5)


# ---- without a teacher: augmentation alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["classmix", "cutmix"])
def test_step_is_the_plain_step_on_the_mixed_batch(dev, kind):
    A, B = _seg_engine(dev, mix=kind, mix_seed=3), _seg_engine(dev)
    sampler = MixSampler(kind, seed=3, num_classes=2)
    img, tgt = _batch(dev)
    pasted = []
    for t in range(2):
        taps = {}
        la = A.train_step(img, tgt, taps)
        tables = sampler.draw(3, 224, 224, t)
        assert _same_tables(taps["mix_tables"], tables) and bool(tables["kind"].all())
        x, y, sel, n = ops.mix_batch(img, tgt.long(), tables, 2)
        assert torch.equal(taps["mix_inp"], x) and torch.equal(taps["mix_target"], y) and torch.equal(taps["mix_sel"], sel)
        assert torch.equal(taps["mix_pasted"], n) and A.last_mix_pasted is taps["mix_pasted"]
        assert torch.equal(la, B.train_step(x, y))
        assert _equal(_weights(A), _weights(B)), f"step {t}"
        pasted.append(int(n.sum()))
    print(f"MEASURE mix step {kind}: pasted {pasted} of {tgt.numel()} pixels a step")
    assert A.mix_step == 2 and sum(pasted) > 0
    plain = _seg_engine(dev)
    for _ in range(2):
        plain.train_step(img, tgt)
    assert not _equal(_weights(A), _weights(plain))                            # the mixing does reach the weights


# ---- with the EMA teacher ----------------------------------------------------------------------------------------------------------
def test_teacher_sees_the_unmixed_batch(dev):
    kw = dict(teacher="ema", distill_flip=True, distill_threshold=0.6, **EMA)
    mixed, unmixed = _seg_engine(dev, mix="classmix", **kw), _seg_engine(dev, **kw)
    img, tgt = _batch(dev)
    tm, tu = {}, {}
    mixed.train_step(img, tgt, tm)
    unmixed.train_step(img, tgt, tu)
    assert len(tm["teacher_logits"]) == 2 and all(torch.equal(a, b) for a, b in zip(tm["teacher_logits"], tu["teacher_logits"]))
    assert int(tm["mix_pasted"].sum()) > 0 and not torch.equal(tm["logits"], tu["logits"])


def test_step_is_the_hard_step_on_the_mixed_batch_plus_the_mixed_consistency_term(dev, monkeypatch):
    """the exact test of tests/test_gpu_mean_teacher.py, carried over: engine B has no teacher and mixes nothing; it is stepped on
    A's mixed batch with ``loss_and_dz`` wrapped to add the mixed term on A's recorded maps"""
    A = _seg_engine(dev, teacher="ema", distill_weight=0.7, distill_temperature=2.0, distill_threshold=0.55, distill_flip=True,
                    distill_rampup=3, mix="classmix", mix_seed=2, **EMA)
    B = _seg_engine(dev, **EMA)
    img, tgt = _batch(dev)
    original = E.loss_and_dz
    for t in range(2):
        taps = {}
        la = A.train_step(img, tgt, taps)
        lam = taps["distill_scale"]
        assert lam == 0.7 * consistency_ramp(t, 3)
        mix = (taps["mix_sel"], taps["mix_tables"]["donor"])
        rec = {}

        def wrapped(engine, logits, target, S):
            loss, dz = original(engine, logits, target, S)
            kd, kept, _ = ops.consistency_loss(logits, taps["teacher_logits"], target, flips=[False, True], temperature=2.0,
                                               threshold=0.55, grad_scale=S * lam, dz=dz, mix=mix)
            rec.update(hard=loss.clone(), kd=kd, kept=kept, logits=logits)
            return loss, dz

        monkeypatch.setattr(E, "loss_and_dz", wrapped)
        B.train_step(taps["mix_inp"], taps["mix_target"])
        monkeypatch.setattr(E, "loss_and_dz", original)
        assert torch.equal(rec["logits"], taps["logits"])
        assert torch.equal(taps["loss_hard"], rec["hard"]) and torch.equal(taps["loss_kd"], rec["kd"]) and torch.equal(taps["kd_kept"], rec["kept"])
        assert torch.equal(taps["loss"], taps["loss_hard"] + lam * taps["loss_kd"]) and torch.equal(la.view(1), taps["loss"].view(1))
        unmixed = ops.consistency_loss(taps["logits"], taps["teacher_logits"], tgt, flips=[False, True], temperature=2.0, threshold=0.55)
        print(f"MEASURE mix step teacher t={t}: pasted {taps['mix_pasted'].tolist()} kd {float(taps['loss_kd']):.6e} kept "
              f"{int(taps['kd_kept'])}; the unmixed term on the same logits {float(unmixed[0]):.6e} kept {int(unmixed[1])}")
        assert _equal(_weights(A), _weights(B)), f"step {t}"
    assert _equal(A.ema.shadows, B.ema.shadows) and A.distill_step == 2 and A.mix_step == 2


# ---- every mode --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cutmix", "classmix"])
@pytest.mark.parametrize("mode", ["reference_exact", "train_adapters", "lora"])
def test_modes(dev, mode, kind):
    kw = {"reference_exact": dict(mode="reference_exact"), "train_adapters": dict(), "lora": dict(train_backbone=True, lora_rank=4)}[mode]
    eng = _seg_engine(dev, teacher="ema", distill_threshold=0.6, distill_flip=True, mix=kind, ema_decay=0.5, **kw)
    img, tgt = _batch(dev)
    taps = {}
    loss = eng.train_step(img, tgt, taps)
    assert torch.isfinite(loss) and torch.isfinite(taps["loss_kd"]).all() and eng.optimizer.skipped_steps == 0
    assert loss.dim() == 0 and taps["mix_pasted"].dtype == torch.int32 and taps["mix_sel"].shape == tgt.shape and not eng.ema.swapped_in


# ---- the draw after a resume, the scripts ----------------------------------------------------------------------------------------
def test_resume_repeats_the_draw(dev):
    eng = _seg_engine(dev, mix="cutmix", mix_p=0.7, mix_seed=9)
    eng.mix_step, eng.mix_rank = 41, 2                                         # what a resume and the script set
    img, tgt = _batch(dev)
    taps = {}
    eng.train_step(img, tgt, taps)
    want = MixSampler("cutmix", p=0.7, seed=9, num_classes=2).draw(3, 224, 224, 41, rank=2)
    assert bool(want["kind"].any()) and _same_tables(taps["mix_tables"], want) and eng.mix_step == 42


def test_scripts(dev, tmp_path):
    from adaptersis_amd import train as T
    run = tmp_path / "mix"
    flags = ["--mix", "classmix", "--mix_seed", "4"]
    eng, _ = _run(T, run, *flags)
    steps = eng.optimizer._steps
    assert eng.mix_sampler.kind == "classmix" and eng.mix_sampler.seed == 4 and eng.mix_sampler.p == 1.0 and eng.mix_step == steps > 1
    assert eng.mix_rank == 0 and eng.teacher is None
    log = [json.loads(line) for line in open(run / "log.txt")]
    assert 0.0 <= log[0]["train_mix_pasted"] <= 1.0
    ck = torch.load(run / "checkpoint.pth.tar", map_location="cpu")
    assert ck["mix"] == {"step": steps}
    resumed, _ = _run(T, run, *flags, "--mix_p", "0.5")                        # epoch 1 of 1 is done: nothing trains
    assert resumed.mix_step == steps and resumed.mix_sampler.p == 0.5
    with pytest.raises(ValueError, match="at least 2"):
        T.train_seg(argparse_namespace(T, run, "--mix", "cutmix", "--batch_size_per_gpu", 1))
    a = T.get_args_parser().parse_args(COMMON + TRAIN + ["--mix", "cutmix", "--mix_background"])
    assert T._mix_engine_args(a) == dict(mix="cutmix", mix_p=1.0, mix_seed=0, mix_background=True)
