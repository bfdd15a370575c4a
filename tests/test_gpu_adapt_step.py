"""GPU: class-adaptive thresholds in the training step — ``SegEngine(distill_class_thresholds=)`` on the tiny engine of
tests/test_gpu_mean_teacher.py.  The step is the ops in a row: its thresholds are, bit for bit, ``ops.confidence_stats`` and
``ops.adaptive_threshold_update`` called by hand on the teacher's maps it tapped, and its soft term is ``ops.consistency_loss``
called by hand with those thresholds on the logits it passed.  Also: ClassMix and unlabelled samples, a fixed list, the checkpoint
round trip, the collectives in a one-rank group (and two ranks where two devices are visible), the default step, the scripts."""
import json
import os
import socket
import subprocess
import sys
import textwrap

import pytest
import torch

from adaptersis_amd import ops
from adaptersis_amd.backbones import engines as E
from tests import adapt_ref as A
from tests.soft_target_helpers import _bits
from tests.test_gpu_mean_teacher import COMMON, TRAIN, _batch, _run, _seg_engine, _weights

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TEACHER = dict(ema_decay=0.5, ema_warmup=False, teacher="ema")


def _record(monkeypatch):
    """every ``ops.consistency_loss`` call of the engine: its arguments as they were (the logits and dz cloned) and what it returned"""
    calls, real = [], ops.consistency_loss

    def wrapped(logits, maps, size, **kw):
        rec = dict(logits=logits.clone(), maps=maps, size=size, kw={k: v for k, v in kw.items() if k not in ("dz", "scratch")},
                   class_threshold=None if kw.get("class_threshold") is None else kw["class_threshold"].clone())
        out = real(logits, maps, size, **kw)
        rec["out"] = (out[0].clone(), out[1].clone())
        calls.append(rec)
        return out

    monkeypatch.setattr(E.ops, "consistency_loss", wrapped)
    return calls, real


def _by_hand(eng, taps, sample_weight=None, state=None):
    """the thresholds of one update from ``state`` (default: the initial one) on the tapped maps"""
    C = eng.num_classes
    H, W = 224, 224
    sums = ops.confidence_stats(taps["teacher_logits"], (H, W), flips=[False] * len(taps["teacher_logits"]) if not eng.distill_flip
                                else [False, True], temperature=eng.distill_temperature, sample_weight=sample_weight)
    st = torch.tensor(A.init_state(C), dtype=torch.float64, device=sums.device) if state is None else state.clone()
    thr = ops.adaptive_threshold_update(sums, st, torch.empty(C, device=sums.device), eng.adaptive.momentum)
    return sums, st, thr


def _check_soft_term(calls, real, taps):
    (call,) = calls
    assert torch.equal(_bits(call["class_threshold"]), _bits(taps["kd_class_thr"])) and "threshold" in call["kw"] and call["kw"]["threshold"] is None
    kw = dict(call["kw"])
    kw["class_threshold"] = taps["kd_class_thr"]
    loss, kept, _ = real(call["logits"], call["maps"], call["size"], **kw)
    assert torch.equal(_bits(loss), _bits(taps["loss_kd"])) and torch.equal(kept, taps["kd_kept"])
    assert torch.equal(_bits(call["out"][0]), _bits(loss))
    return int(kept)


def test_adaptive_step_is_the_ops_in_a_row(dev, monkeypatch):
    calls, real = _record(monkeypatch)
    eng = _seg_engine(dev, distill_class_thresholds="adaptive", distill_adaptive_momentum=0.5, distill_temperature=2.0, distill_flip=True,
                      **TEACHER)
    img, tgt = _batch(dev)
    taps = {}
    eng.train_step(img, tgt, taps)
    sums, st, thr = _by_hand(eng, taps)
    assert torch.equal(_bits(taps["kd_class_thr"]), _bits(thr)) and torch.equal(taps["kd_conf_sums"].view(torch.int64), sums.view(torch.int64))
    assert torch.equal(eng.adaptive.state.view(torch.int64), st.view(torch.int64)) and float(st[1]) == 1.0
    assert int(sums[-1]) == tgt.numel() and not torch.equal(thr, torch.full_like(thr, 0.5))
    kept = _check_soft_term(calls, real, taps)
    assert 0 <= kept <= tgt.numel()
    # the second step starts from the first one's state
    calls.clear()
    taps2 = {}
    eng.train_step(img, tgt, taps2)
    _, st2, thr2 = _by_hand(eng, taps2, state=st)
    assert torch.equal(_bits(taps2["kd_class_thr"]), _bits(thr2)) and float(eng.adaptive.state[1]) == 2.0
    _check_soft_term(calls, real, taps2)


@pytest.mark.parametrize("weight", [0.0, 0.5])
def test_classmix_and_unlabelled_samples(dev, monkeypatch, weight):
    calls, real = _record(monkeypatch)
    eng = _seg_engine(dev, distill_class_thresholds="adaptive", distill_adaptive_momentum=0.5, mix="classmix", mix_seed=3,
                      distill_labelled_weight=weight, **TEACHER)
    img, tgt = _batch(dev)
    taps = {}
    eng.train_step(img, tgt, taps, labelled=[True, False, False])
    sw = taps["sample_weight"]
    assert sw.tolist() == [weight, 1.0, 1.0]
    sums, st, thr = _by_hand(eng, taps, sw)
    assert torch.equal(_bits(taps["kd_class_thr"]), _bits(thr)) and torch.equal(taps["kd_conf_sums"].view(torch.int64), sums.view(torch.int64))
    per = tgt[0].numel()
    assert int(sums[-1]) == (2 if weight == 0.0 else 3) * per                 # weight 0: the unlabelled samples alone
    (call,) = calls
    assert ("mix" in call["kw"] and call["kw"]["mix"] is not None) == ("mix_sel" in taps)
    _check_soft_term(calls, real, taps)


def test_fixed_list(dev, monkeypatch):
    calls, real = _record(monkeypatch)
    eng = _seg_engine(dev, distill_class_thresholds=[0.9, 0.6], **TEACHER)
    assert eng.adaptive is None
    img, tgt = _batch(dev)
    taps = {}
    eng.train_step(img, tgt, taps)
    assert taps["kd_class_thr"].tolist() == torch.tensor([0.9, 0.6]).tolist() and taps["kd_conf_sums"] is None
    _check_soft_term(calls, real, taps)
    eng.train_step(img, tgt)
    assert eng.class_thresholds.tolist() == torch.tensor([0.9, 0.6]).tolist()  # never updated


def test_state_dict_round_trip(dev):
    eng = _seg_engine(dev, distill_class_thresholds="adaptive", distill_adaptive_momentum=0.5, **TEACHER)
    img, tgt = _batch(dev)
    eng.train_step(img, tgt)
    sd = eng.adaptive.state_dict()
    assert not sd["state"].is_cuda and not sd["thresholds"].is_cuda
    other = _seg_engine(dev, distill_class_thresholds="adaptive", distill_adaptive_momentum=0.5, **TEACHER)
    assert other.adaptive.state.tolist() == A.init_state(2)
    other.adaptive.load_state_dict(sd)
    assert torch.equal(other.adaptive.state.view(torch.int64), eng.adaptive.state.view(torch.int64))
    assert torch.equal(_bits(other.adaptive.thresholds), _bits(eng.adaptive.thresholds)) and other.class_thresholds is other.adaptive.thresholds


def test_default_step_keeps_its_bits_and_opens_nothing(dev, monkeypatch):
    from adaptersis_amd import _lib_adapt
    monkeypatch.setattr(_lib_adapt, "_dlib", None)                             # as in a process that never opened the library
    img, tgt = _batch(dev)
    a = _seg_engine(dev, distill_threshold=0.6, **TEACHER)
    b = _seg_engine(dev, distill_threshold=0.6, **TEACHER)
    ta, tb = {}, {}
    la, lb = a.train_step(img, tgt, ta), b.train_step(img, tgt, tb)
    assert torch.equal(_bits(la), _bits(lb)) and all(torch.equal(x, y) for x, y in zip(_weights(a), _weights(b)))
    assert a.adaptive is None and a.class_thresholds is None and "kd_class_thr" not in ta and "kd_conf_sums" not in ta
    assert not _lib_adapt.loaded()
    c = _seg_engine(dev, distill_class_thresholds=[0.6, 0.6], **TEACHER)      # equal thresholds: the scalar gate's step, bit for bit
    lc = c.train_step(img, tgt)
    assert torch.equal(_bits(la), _bits(lc)) and all(torch.equal(x, y) for x, y in zip(_weights(a), _weights(c)))
    assert _lib_adapt.loaded()


def test_scripts(dev, tmp_path):
    from adaptersis_amd import train as T
    run = tmp_path / "adaptive"
    flags = ["--ema_decay", "0.9", "--distill_teacher", "ema", "--distill_adaptive_threshold", "--distill_adaptive_momentum", "0.9"]
    eng, _ = _run(T, run, *flags)
    assert eng.adaptive is not None and eng.adaptive.momentum == 0.9 and float(eng.adaptive.state[1]) == eng.distill_step > 1
    log = [json.loads(line) for line in open(run / "log.txt")]
    assert 0.0 < log[0]["train_kd_tau"] < 1.0 and len(log[0]["distill_class_thr"]) == 2
    assert log[0]["distill_class_thr"] == eng.class_thresholds.tolist() and max(log[0]["distill_class_thr"]) <= 1.0
    ck = torch.load(run / "checkpoint.pth.tar", map_location="cpu")
    assert set(ck["distill"]) == {"step", "adaptive"}
    assert torch.equal(ck["distill"]["adaptive"]["state"], eng.adaptive.state.cpu())
    resumed, _ = _run(T, run, *flags)                                          # epoch 1 of 1 is done: nothing trains
    assert torch.equal(resumed.adaptive.state.view(torch.int64), eng.adaptive.state.view(torch.int64))
    assert torch.equal(_bits(resumed.adaptive.thresholds), _bits(eng.adaptive.thresholds))
    fixed, _ = _run(T, tmp_path / "fixed", "--ema_decay", "0.9", "--distill_teacher", "ema", "--distill_class_thresholds", "0.9", "0.6")
    assert fixed.adaptive is None and fixed.class_thresholds.tolist() == torch.tensor([0.9, 0.6]).tolist()
    ck = torch.load(tmp_path / "fixed" / "checkpoint.pth.tar", map_location="cpu")
    assert set(ck["distill"]) == {"step"}
    log = [json.loads(line) for line in open(tmp_path / "fixed" / "log.txt")]
    assert "train_kd_tau" not in log[0] and log[0]["distill_class_thr"] == fixed.class_thresholds.tolist()


# ---- collectives: a child process (a process group is process-global state) ---------------------------------------------------
CHILD = textwrap.dedent('''
    import os, sys, torch
    import torch.distributed as dist
    sys.path.insert(0, os.environ["ASIS_ROOT"])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(rank)
    dev = torch.device("cuda", rank)
    from adaptersis_amd import parallel
    from adaptersis_amd.adaptive_threshold import AdaptiveThreshold
    from tests import adapt_ref as A
    from tests.soft_target_helpers import STUDENT, TEACHER_SETS, _maps
    C, size, temp, lam = 3, (13, 11), 1.0, 0.5
    per_rank = [_maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 51, r) for r in range(world)]
    _, ts, flips = per_rank[rank]
    td = [t.to(dev) for t in ts]

    def steps():
        ad = AdaptiveThreshold(C, lam, dev)
        for _ in range(3):
            ad.update(td, flips, size, temp)
        return ad

    base = steps() if world == 1 else None                                  # no process group: no collective is issued
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    parallel.FORCE_COLLECTIVES = world == 1
    assert parallel.collectives_on()
    ad = steps()
    if world == 1:
        assert torch.equal(ad.thresholds.view(torch.int32), base.thresholds.view(torch.int32))
        assert torch.equal(ad.state.view(torch.int64), base.state.view(torch.int64))
    else:
        both = [torch.empty_like(ad.thresholds) for _ in range(world)]
        dist.all_gather(both, ad.thresholds)
        assert all(torch.equal(b.view(torch.int32), both[0].view(torch.int32)) for b in both)
        total = sum(A.stats_ref(p[1], p[2], size, temp) for p in per_rank)
        state, want = A.init_state(C), None
        for _ in range(3):
            state, want = A.update_ref(state, total.tolist(), lam)
        assert float(ad.state[1]) == 3.0 and int(ad.sums[-1]) == world * 2 * size[0] * size[1]
        assert float((ad.thresholds.cpu().double() - want.double()).abs().max()) <= 16 * 2.0 ** -23
    dist.destroy_process_group()
    print("ADAPT_COLLECTIVES_OK", rank)
''')


def _children(world):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for rank in range(world):
        env = dict(os.environ, ASIS_ROOT=ROOT, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("LOCAL_RANK", None)
        procs.append(subprocess.Popen([sys.executable, "-c", CHILD], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                                      cwd=ROOT))
    for rank, p in enumerate(procs):
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0 and f"ADAPT_COLLECTIVES_OK {rank}" in out, (out[-1500:], err[-3000:])


def test_forced_collectives_in_a_one_rank_group_keep_the_bits(dev):
    _children(1)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="two ranks need two devices")
def test_two_ranks_end_with_equal_thresholds(dev):
    _children(2)
