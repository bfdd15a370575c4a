"""CPU: the float64 restatement of the gated consistency loss (tests/consist_ref.py) against tests/distill_ref.py and the closed
form of its gradient; the ABI of libasis_consist.so (include/asis_consist.h: every declared symbol exported and bound, none of them
in libasis_hip.so or libasis_distill.so) and the argument errors of ``asis_consist_loss`` that need no GPU; the ramp-up schedule;
the mean-teacher flag checks of the training scripts; the teacher's weak view of the augmentation."""
import argparse
import ctypes
import math
import os
import re

import pytest
import torch

from adaptersis_amd import _lib, _lib_consist, _lib_distill, ops
from adaptersis_amd import train as T
from adaptersis_amd.optim import consistency_ramp
from adaptersis_amd.segloss.consistency import ConsistencyLoss
from adaptersis_amd.tools.augment import TrainAugment, weak_params
from tests import consist_ref as R
from tests import distill_ref as D
from tests.bound_helpers import _gen


def _maps(C, scale, *key):
    g = _gen(*key)
    z = torch.randn(2, 5, 7, C, generator=g, dtype=torch.float64) * scale
    ts = [torch.randn(2, 6, 4, C, generator=g, dtype=torch.float64) * scale, torch.randn(2, 9, 3, C, generator=g, dtype=torch.float64) * scale]
    return z, ts, [False, True]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("temp", [1.0, 2.0, 4.0])
@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_ungated_unweighted_restatement_is_distill_ref(temp, C, scale):
    z, ts, flips = _maps(C, scale, C, int(temp), int(scale))
    for thr in (None, 0.0, -1.0):
        r = R.consist_ref(z, ts, flips, (13, 11), temp, thr)
        d = D.distill_ref(z, ts, flips, (13, 11), temp)
        assert torch.equal(r.loss, d[0]) and torch.equal(r.dz, d[1]) and torch.equal(r.dlow, d[2])
        assert r.kept == 2 * 13 * 11 and bool(r.gate.all())
    ones = R.consist_ref(z, ts, flips, (13, 11), temp, None, torch.ones(2))
    assert torch.equal(ones.loss, d[0]) and torch.equal(ones.dz, d[1])


@pytest.mark.parametrize("temp", [1.0, 2.0])
@pytest.mark.parametrize("C", [3, 8])
def test_gated_gradient_closed_form(temp, C):
    z, ts, flips = _maps(C, 1.0, 7, C, int(temp))
    H, W = 13, 11
    N = 2 * H * W
    conf = R.confidence(ts, flips, (H, W), temp)
    thr, _ = R.pick_threshold(conf)
    w = torch.tensor([0.25, 2.0], dtype=torch.float64)
    r = R.consist_ref(z, ts, flips, (H, W), temp, thr, w)
    assert torch.equal(r.conf, conf) and torch.equal(r.gate, conf >= thr) and 0 < int(r.gate.sum()) < N
    assert r.kept == int(r.gate.sum())
    m = r.gate.double()
    closed = (temp / N) * (w.view(2, 1, 1, 1) * m.unsqueeze(1) * (r.p - r.q)).permute(0, 2, 3, 1)
    assert float((r.dz - closed).abs().max()) <= 1e-12 * float(closed.abs().max())
    assert bool((r.dz[~r.gate] == 0).all())
    want = temp * temp * float((w.view(2, 1, 1) * m * r.kd).sum()) / N
    assert abs(float(r.loss) - want) <= 1e-12 * abs(want)
    # a sample of weight 0 is not counted, whatever its gate says
    z0 = R.consist_ref(z, ts, flips, (H, W), temp, thr, torch.tensor([0.0, 0.5]))
    assert z0.kept == int(r.gate[1].sum()) and bool((z0.dz[0] == 0).all())
    # the gate drops everything / nothing
    assert R.consist_ref(z, ts, flips, (H, W), temp, 1.0).kept == 0
    assert float(R.consist_ref(z, ts, flips, (H, W), temp, 1.0).loss) == 0.0


def test_pick_threshold_keeps_clear_of_every_confidence():
    conf = torch.tensor([0.5, 0.50001, 0.6, 0.9, 0.91, 0.95, 0.96, 0.97, 0.98, 0.99], dtype=torch.float64)
    thr, note = R.pick_threshold(conf)
    assert 0.6 < thr < 0.9 and "mid-range" in note
    sat = torch.cat([torch.full((50,), 1.0, dtype=torch.float64) - torch.arange(50, dtype=torch.float64) * 1e-9, torch.tensor([0.7], dtype=torch.float64)])
    thr, note = R.pick_threshold(sat)
    assert 0.7 < thr < 0.99 and "overall" in note
    with pytest.raises(AssertionError):
        R.pick_threshold(torch.tensor([0.5, 0.500001, 0.500002], dtype=torch.float64))


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_side_library_abi():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "asis_consist.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(asis_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib_consist.SIGNATURES) == ["asis_consist_loss", "asis_consist_nblk", "asis_consist_tile"]
    assert os.path.dirname(_lib_consist.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    side, main, dist = ctypes.CDLL(_lib_consist.LIB_PATH), ctypes.CDLL(_lib.LIB_PATH), ctypes.CDLL(_lib_distill.LIB_PATH)
    for n in names:
        assert hasattr(side, n) and not hasattr(main, n) and not hasattr(dist, n)
        assert n not in _lib.SIGNATURES and n not in _lib_distill.SIGNATURES
    assert _lib_consist.lib() is _lib_consist.lib() and _lib_consist.loaded()


def test_build_lists_the_library_and_sees_its_header():
    from adaptersis_amd import build
    assert build.SIDE_LIBS["libasis_consist.so"] == ("consist.hip",) and build.SIDE_LIBS["libasis_distill.so"] == ("distill.hip",)
    assert not any(s.endswith(("consist.hip", "distill.hip")) for s in build.sources())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for hdr in ("include/asis_consist.h", "include/asis_distill.h", "adaptersis_amd/csrc/soft_target.h"):
        assert build._deps_mtime() >= os.path.getmtime(os.path.join(root, *hdr.split("/"))), hdr


def test_nblk_and_tile_need_no_gpu():
    lib = _lib_consist.lib()
    tile = lib.asis_consist_tile()
    assert tile > 0 and tile % 64 == 0
    cap = lib.asis_consist_nblk((1 << 31) - 1)
    assert cap >= 256
    for N, want in ((1, 1), (tile - 1, 1), (tile, 1), (tile + 1, 2), (cap * tile, cap), (cap * tile + 1, cap)):
        assert lib.asis_consist_nblk(N) == want
        assert ops.consistency_scratch_bytes(N) == 16 * want
    for N in (0, -5, 1 << 31, 1 << 40):
        assert lib.asis_consist_nblk(N) == -1 and b"2^31" in _lib.lib().asis_last_error()
        with pytest.raises(ValueError):
            ops.consistency_scratch_bytes(N)


def test_argument_errors_before_any_launch():
    lib, last_error = _lib_consist.lib(), _lib.lib().asis_last_error
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(logits=p, teachers="list", V=1, B=1, h=2, w=2, H=2, W=2, C=2, temp=1.0, thr=0.5, partial=p, loss=p, kept=p, dz=p, hs=2,
             ws=2, first=p, flips="list"):
        n = max(V, 1)
        ptrs = (ctypes.c_void_p * n)(*([first] + [p] * (n - 1)))
        th, tw, fl = (ctypes.c_int * n)(*[hs] * n), (ctypes.c_int * n)(*[ws] * n), (ctypes.c_int * n)(*[0] * n)
        return lib.asis_consist_loss(None, logits, B, h, w, ptrs if teachers == "list" else teachers, th, tw,
                                     fl if flips == "list" else flips, V, H, W, C, temp, thr, None, 1.0, 0, partial, loss, kept, dz)

    for kw, word in ((dict(logits=None), b"null"), (dict(teachers=None), b"null"), (dict(flips=None), b"null"),
                     (dict(partial=None), b"null"), (dict(loss=None), b"null"), (dict(kept=None), b"null"), (dict(dz=None), b"null"),
                     (dict(first=None), b"teachers[0]"), (dict(V=0), b"V=0"), (dict(V=9), b"V=9"), (dict(C=0), b"C=0"),
                     (dict(C=17), b"C=17"), (dict(B=0), b"non-positive"), (dict(h=0), b"non-positive"), (dict(W=-3), b"non-positive"),
                     (dict(hs=0), b"teacher map 0"), (dict(temp=0.0), b"temperature"), (dict(temp=-1.0), b"temperature"),
                     (dict(temp=float("nan")), b"temperature"), (dict(thr=1.5), b"threshold"), (dict(thr=float("nan")), b"threshold"),
                     (dict(thr=float("inf")), b"threshold"), (dict(B=1 << 11, H=1 << 10, W=1 << 10), b"2^31"),
                     (dict(partial=p + 4), b"aligned")):
        assert call(**kw) == _lib.ASIS_EINVAL, kw
        assert word in last_error(), (kw, last_error())
    with pytest.raises(ValueError):
        _lib.check(call(thr=1.5), "asis_consist_loss")


def test_op_and_module_have_no_cpu_fallback():
    z, t = torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3)
    with pytest.raises(_lib.AsisError):
        ops.consistency_loss(z, t, (4, 4), threshold=0.5)
    with pytest.raises(_lib.AsisError):
        ConsistencyLoss(2.0, 0.5)(z.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2), (4, 4))
    m = ConsistencyLoss(4.0, 0.7, [False, True])
    assert m.temperature == 4.0 and m.threshold == 0.7 and m.flips == [False, True] and m.last_kept is None
    d = ConsistencyLoss()
    assert d.temperature == 1.0 and d.threshold is None and d.flips is None
    for bad in (dict(temperature=0.0), dict(threshold=1.5), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            ConsistencyLoss(**bad)
    with pytest.raises(NotImplementedError):
        ConsistencyLoss()(torch.zeros(1, 3, 2, 4, 5), t)


# ---- the schedule ------------------------------------------------------------------------------------------------------------------
def test_consistency_ramp():
    assert consistency_ramp(0, 40) == math.exp(-5.0) and 0.0 < consistency_ramp(0, 40) < 0.01
    vals = [consistency_ramp(t, 40) for t in range(0, 60)]
    assert all(b > a for a, b in zip(vals[:40], vals[1:41]))
    assert all(v == 1.0 for v in vals[40:])
    assert abs(consistency_ramp(20, 40) - math.exp(-1.25)) < 1e-15
    assert [consistency_ramp(t, 0) for t in (0, 1, 1000)] == [1.0, 1.0, 1.0]
    assert consistency_ramp(1, 1) == 1.0 and consistency_ramp(0, 1) == math.exp(-5.0)
    for bad in ((-1, 3), (0, -1)):
        with pytest.raises(ValueError):
            consistency_ramp(*bad)


# ---- the flags ---------------------------------------------------------------------------------------------------------------------
def _ns(**kw):
    return argparse.Namespace(arch="vit_large", **kw)


def test_flag_checks(tmp_path):
    ck = tmp_path / "teacher.pth.tar"
    ck.write_bytes(b"x")
    ok = T.check_distill_args
    assert ok(argparse.Namespace()) is None and ok(_ns(distill_teacher=None)) is None
    assert ok(_ns(distill_teacher="ema", ema_decay=0.9)) is None
    assert ok(_ns(distill_teacher="ema", ema_decay=0.9, distill_weight=0.0, distill_temperature=2.0, distill_threshold=0.6,
                  distill_rampup=100, distill_flip=True, distill_weak=True)) is None
    assert ok(_ns(distill_teacher=str(ck), distill_teacher_arch="vit_small", distill_teacher_ema=True)) is None
    assert "needs --ema_decay" in ok(_ns(distill_teacher="ema"))
    assert "no such checkpoint" in ok(_ns(distill_teacher=str(tmp_path / "absent.pth.tar")))
    assert "not with --distill_teacher ema" in ok(_ns(distill_teacher="ema", ema_decay=0.9, distill_teacher_ema=True))
    assert "not with --distill_teacher ema" in ok(_ns(distill_teacher="ema", ema_decay=0.9, distill_teacher_arch="vit_small"))
    assert "--distill_teacher_arch" in ok(_ns(distill_teacher=str(ck), distill_teacher_arch="resnet"))
    for flag, value in (("distill_weight", 0.0), ("distill_temperature", 2.0), ("distill_threshold", 0.5), ("distill_rampup", 10),
                        ("distill_flip", True), ("distill_weak", True), ("distill_teacher_ema", True), ("distill_teacher_arch", "vit_small")):
        assert f"--{flag} needs --distill_teacher" in ok(_ns(**{flag: value}))
    for kw, word in ((dict(distill_weight=-1.0), "--distill_weight"), (dict(distill_weight=float("nan")), "--distill_weight"),
                     (dict(distill_temperature=0.0), "--distill_temperature"), (dict(distill_threshold=1.5), "--distill_threshold"),
                     (dict(distill_threshold=float("nan")), "--distill_threshold"), (dict(distill_rampup=-1), "--distill_rampup")):
        assert word in ok(_ns(distill_teacher="ema", ema_decay=0.9, **kw))
    # the parser refuses them as usage errors, and train_seg before any process group is opened
    p = T.get_args_parser()
    with pytest.raises(SystemExit):
        p.parse_args(["--distill_teacher", "ema"])
    with pytest.raises(SystemExit):
        p.parse_args(["--distill_flip"])
    a = p.parse_args(["--ema_decay", "0.9", "--distill_teacher", "ema", "--distill_threshold", "0.6", "--distill_flip"])
    assert T._distill_engine_args(a, "ema") == dict(teacher="ema", distill_weight=1.0, distill_temperature=1.0, distill_threshold=0.6,
                                                    distill_rampup=0, distill_flip=True)
    assert T._distill_engine_args(p.parse_args([]), None) == {}
    with pytest.raises(ValueError, match="needs --ema_decay"):
        T.train_seg(_ns(distill_teacher="ema"))


def test_teacher_shares_the_backbone_under_the_stated_rule():
    share = T.teacher_shares_backbone
    assert share(_ns(), {"state_dict": {}})
    assert share(_ns(distill_teacher_arch="vit_large", train_backbone=True), {"state_dict": {}})
    assert not share(_ns(distill_teacher_arch="vit_small"), {"state_dict": {}})
    assert not share(_ns(optimize_backbone=True), {"state_dict": {}})
    assert not share(_ns(), {"state_dict": {}, "backbone": {}})
    assert not share(_ns(), {"state_dict": {}, "lora": {}})


# ---- the weak view -----------------------------------------------------------------------------------------------------------------
def test_weak_view_parameters():
    a, b = TrainAugment(size=64, seed=5, non_rigid_p=0.5), TrainAugment(size=64, seed=5, non_rigid_p=0.5)
    drawn = a.draw(64)
    weak = weak_params(drawn)
    assert any(p["clahe"] is not None for p in drawn) and any(p["gamma"] is not None for p in drawn)
    assert any(p["nonrigid"] is not None for p in drawn) and any(p["crop"] is not None for p in drawn)
    for p, q in zip(drawn, weak):
        assert q["clahe"] is None and q["alpha"] == 1.0 and q["beta"] == 0.0 and q["gamma"] is None
        for k in ("crop", "flip", "rotk"):
            assert q[k] == p[k]
        assert q["nonrigid"] is p["nonrigid"] and set(q) == set(p)
    # neutral photometrics: identity tables and no CLAHE flag; the geometry tables are the student's
    ts, tw = a.tables(drawn, "cpu"), a.tables(weak, "cpu")
    assert bool((tw["lut"] == torch.arange(256, dtype=torch.uint8)).all()) and not tw["clahe_any"] and int(tw["clahe"].abs().sum()) == 0
    for k in ("geo", "xofs", "yofs", "xa", "ya", "mx", "my", "nr_kind", "nr_par", "nr_seed", "nr_gx", "nr_gy"):
        assert torch.equal(ts[k], tw[k]), k
    # making the weak view draws nothing: the stream is that of a run without the flag
    b.draw(64)
    nxt_a, nxt_b = a.draw(8), b.draw(8)
    assert repr(nxt_a) == repr(nxt_b)
    assert drawn[0] is not weak[0] and any(p["clahe"] is not None for p in drawn)       # the student's draws are not edited
