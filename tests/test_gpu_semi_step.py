"""GPU: the semi-supervised step — ``SegEngine(ignore_index=, distill_labelled_weight=)`` and ``train_step(labelled=)`` on the
tiny engine of tests/test_gpu_mean_teacher.py (``vit_tiny_test``, 224 x 224, B = 3): the default launches what it launched, the
step is the plain step with ``ops.seg_loss_ignore`` as its hard loss and a weighted ``ops.consistency_loss`` (weights equal bit
for bit), what the caller leaves in an unlabelled row does not matter, a batch without labels trains through the soft term alone,
mixing stays inside the labelled and the unlabelled group with the teacher's classes on unlabelled donors, and the flags of the
training script."""
import json

import pytest
import torch

from adaptersis_amd import _lib_semi, config, ops
from adaptersis_amd.backbones import engines as E
from adaptersis_amd.utils import weights as W
from tests.test_gpu_mean_teacher import _batch, _equal, _run, _seg_engine, _weights

pytestmark = pytest.mark.gpu

EMA = dict(ema_decay=0.5, ema_warmup=False)
SEMI = dict(teacher="ema", distill_flip=True, distill_threshold=0.55, distill_labelled_weight=0.5, **EMA)
HW = 224 * 224


# ---- the default -------------------------------------------------------------------------------------------------------------------
def test_default_step_is_the_plain_step_and_opens_nothing(dev, monkeypatch):
    monkeypatch.setattr(_lib_semi, "_dlib", None)                              # as in a process that never opened the library
    plain = _seg_engine(dev)
    eng = _seg_engine(dev, ignore_index=None, distill_labelled_weight=1.0)
    img, tgt = _batch(dev)
    for step in range(2):
        taps = {}
        a, b = plain.train_step(img, tgt), eng.train_step(img, tgt, taps, labelled=None if step == 0 else [True, True, True])
        assert torch.equal(a, b) and "hard_valid" not in taps and "sample_weight" not in taps
    assert _equal(_weights(plain), _weights(eng))
    assert not _lib_semi.loaded() and eng.last_hard_valid is None and eng.ignore_index is None


# ---- the step, composed from the ops -------------------------------------------------------------------------------------------------
def test_step_is_the_ignore_loss_plus_the_weighted_consistency_term(dev, monkeypatch):
    A, B = _seg_engine(dev, **SEMI), _seg_engine(dev, **EMA)
    img, tgt = _batch(dev)
    labelled = [True, False, True]
    sw = torch.tensor([0.5, 1.0, 0.5], device=dev)
    n_region, lmode, eps, n_ce = E.SegEngine.LOSSES["dice"]
    original = E.loss_and_dz
    for t in range(2):
        taps = {}
        la = A.train_step(img, tgt, taps, labelled=labelled)
        lam, rec = taps["distill_scale"], {}

        def wrapped(engine, logits, target, S):
            t255 = target.clone()
            t255[1] = 255
            loss, dz, valid, _ = ops.seg_loss_ignore(logits, t255, 255, n_region, lmode, eps, n_ce, None, S)
            kd, kept, _ = ops.consistency_loss(logits, taps["teacher_logits"], target, flips=[False, True], temperature=1.0,
                                               threshold=0.55, sample_weight=sw, grad_scale=S * lam, dz=dz)
            rec.update(hard=loss.clone(), kd=kd, kept=kept, logits=logits, valid=valid)
            return loss, dz

        monkeypatch.setattr(E, "loss_and_dz", wrapped)
        B.train_step(img, tgt)
        monkeypatch.setattr(E, "loss_and_dz", original)
        assert torch.equal(rec["logits"], taps["logits"])
        assert torch.equal(taps["loss_hard"], rec["hard"]) and torch.equal(taps["loss_kd"], rec["kd"]) and torch.equal(taps["kd_kept"], rec["kept"])
        assert torch.equal(taps["loss"], rec["hard"] + lam * rec["kd"]) and torch.equal(la.view(1), taps["loss"].view(1))
        assert torch.equal(taps["hard_valid"], rec["valid"]) and taps["hard_valid"].tolist() == [HW, 0, HW]
        assert A.last_hard_valid is taps["hard_valid"] and taps["labelled"] == (True, False, True)
        assert torch.equal(taps["sample_weight"], sw) and int(taps["kd_kept"]) > 0
        assert _equal(_weights(A), _weights(B)), f"step {t}"
    assert _equal(A.ema.shadows, B.ema.shadows)
    # the tables are cached per pattern
    assert len(A._semi_cache) == 1
    A.train_step(img, tgt, labelled=labelled)
    assert len(A._semi_cache) == 1


def test_the_content_of_an_unlabelled_row_does_not_matter(dev):
    X, Y = _seg_engine(dev, **SEMI), _seg_engine(dev, **SEMI)
    img, tgt = _batch(dev)
    junk = tgt.clone()
    junk[1] = torch.randint(-5, 1000, junk[1].shape, device=dev)
    kept = junk.clone()
    for _ in range(2):
        a, b = X.train_step(img, tgt, labelled=[True, False, True]), Y.train_step(img, junk, labelled=[True, False, True])
        assert torch.equal(a, b)
    assert _equal(_weights(X), _weights(Y)) and torch.equal(junk, kept)        # and the caller's tensor keeps what it held


def test_a_batch_without_labels_trains_through_the_soft_term(dev):
    eng = _seg_engine(dev, **SEMI)
    img, tgt = _batch(dev)
    eng.train_step(img, tgt)                                                   # a labelled step first: the average leaves the live weights
    before = _weights(eng)
    taps = {}
    loss = eng.train_step(img, tgt, taps, labelled=[False, False, False])
    lam = taps["distill_scale"]
    assert float(taps["loss_hard"]) == 0.0 and taps["hard_valid"].tolist() == [0, 0, 0]
    assert torch.equal(loss.view(1), (lam * taps["loss_kd"]).view(1)) and float(loss) > 0.0 and int(taps["kd_kept"]) > 0
    assert torch.equal(taps["sample_weight"], torch.ones(3, device=dev))
    assert not _equal(before, _weights(eng)) and eng.optimizer.skipped_steps == 0


def test_ignore_index_routes_the_hard_loss(dev):
    eng = _seg_engine(dev, ignore_index=255, loss="ce_dc")
    img, tgt = _batch(dev)
    tgt = tgt.clone()
    tgt[0, :100] = 255
    tgt[2] = 255
    taps = {}
    loss = eng.train_step(img, tgt, taps)
    n_region, lmode, eps, n_ce = E.SegEngine.LOSSES["ce_dc"]
    want, _, valid, _ = ops.seg_loss_ignore(taps["logits"], tgt, 255, n_region, lmode, eps, n_ce, None, config.loss_scale)
    assert torch.equal(loss.view(1), want) and torch.equal(taps["hard_valid"], valid) and valid.tolist() == [HW - 100 * 224, HW, 0]
    assert taps["labelled"] is None and taps["sample_weight"] is None


def test_refusals(dev):
    img, tgt = _batch(dev)
    eng = _seg_engine(dev)
    with pytest.raises(ValueError, match="needs a teacher"):
        eng.train_step(img, tgt, labelled=[True, False, True])
    with pytest.raises(ValueError, match="labelled has 2 entries"):
        eng.train_step(img, tgt, labelled=[True, True])
    for loss in ("lovasz", "ce_lovasz", "topk", "dc_and_topk", "focal"):
        with pytest.raises(ValueError, match="has no ignore label"):
            _seg_engine(dev, ignore_index=255, loss=loss)
    for bad in (0, 1, 255.0, True):
        with pytest.raises(ValueError, match="ignore_index"):
            _seg_engine(dev, ignore_index=bad)
    with pytest.raises(ValueError, match="distill_labelled_weight"):
        _seg_engine(dev, distill_labelled_weight=-1.0)
    lov = _seg_engine(dev, loss="lovasz", **SEMI)                              # no ignore_index: refused where the first unlabelled sample comes
    with pytest.raises(ValueError, match="has no ignore label"):
        lov.train_step(img, tgt, labelled=[True, False, True])


# ---- mixing --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["classmix", "cutmix"])
def test_mixing_stays_inside_the_groups(dev, kind):
    eng = _seg_engine(dev, mix=kind, mix_seed=3, **SEMI)
    img, tgt = W.synthetic_batch(4, 224)
    img, tgt = img.to(dev), tgt.to(dev)
    labelled, unl = [False, True, False, False], [0, 2, 3]
    taps = {}
    loss = eng.train_step(img, tgt, taps, labelled=labelled)
    tables = taps["mix_tables"]
    donor, k = tables["donor"].tolist(), tables["kind"].tolist()
    assert donor[1] == 1 and k[1] == 0 and sorted(donor[b] for b in unl) == unl and all(donor[b] != b for b in unl)
    assert all(k[b] == (2 if kind == "classmix" else 1) for b in unl)
    want = eng.mix_sampler.draw(4, 224, 224, 0, 0, groups=[0, 1, 0, 0])
    assert all(torch.equal(tables[n], want[n]) for n in want)
    src = tgt.clone()
    if kind == "classmix":                                                     # an unlabelled donor's classes are the teacher's
        pseudo = ops.predict_mask_views(taps["teacher_logits"], (224, 224), flips=[False, True])
        assert torch.equal(taps["pseudo_target"], pseudo)
        src[unl] = pseudo[unl].long()
    else:
        assert "pseudo_target" not in taps
        src[unl] = 255
    minp, mtgt, sel, pasted = ops.mix_batch(img, src, tables, 2, False)
    assert torch.equal(taps["mix_inp"], minp) and torch.equal(taps["mix_sel"], sel) and torch.equal(taps["mix_pasted"], pasted)
    assert torch.equal(taps["mix_target"][1], mtgt[1]) and torch.equal(mtgt[1], tgt[1]) and torch.equal(minp[1], img[1])
    assert bool((taps["mix_target"][unl] == 255).all()) and taps["hard_valid"].tolist() == [0, HW, 0, 0]
    if kind == "cutmix":
        assert int(pasted.sum()) > 0
    assert torch.isfinite(loss) and eng.optimizer.skipped_steps == 0


# ---- the scripts ---------------------------------------------------------------------------------------------------------------------
def test_scripts(dev, tmp_path):
    from adaptersis_amd import train as T
    run, plain = tmp_path / "semi", tmp_path / "plain"
    flags = ["--ema_decay", "0.5", "--distill_teacher", "ema", "--unlabelled_path", "synthetic", "--unlabelled_per_batch", "8",
             "--mix", "classmix"]
    eng, stats = _run(T, run, *flags)
    steps = eng.optimizer._steps
    assert steps == 6 and eng.unlabelled.per_batch == 8 and eng.ignore_index is None
    # 24 unlabelled frames, 8 a step: the stream starts over at the fourth of the six steps
    assert eng.unlabelled.epoch == 1
    log = [json.loads(line) for line in open(run / "log.txt")]
    assert abs(log[0]["train_hard_valid"] - 4 / 12) < 1e-12 and "train_loss_kd" in log[0] and "train_mix_pasted" in log[0]
    ck = torch.load(run / "checkpoint.pth.tar", map_location="cpu")
    assert ck["semi"] == {"epoch": 1}
    resumed, _ = _run(T, run, *flags)                                          # epoch 1 of 1 is done: nothing trains
    assert resumed.unlabelled.epoch == 1 and resumed.optimizer._steps == steps
    eng3, _ = _run(T, plain, "--ema_decay", "0.5", "--distill_teacher", "ema", "--mix", "classmix")
    ck3 = torch.load(plain / "checkpoint.pth.tar", map_location="cpu")
    assert eng3.unlabelled is None and "semi" not in ck3 and set(ck3) == set(ck) - {"semi"}
    assert "hard_valid" not in open(plain / "log.txt").read()
