"""CPU: the float64 restatement of the class-adaptive thresholds (tests/adapt_ref.py) against hand-worked cases; the ABI of
libasis_adapt.so (include/asis_adapt.h: every declared symbol exported and bound, none of them in libasis_hip.so) and its place in
the build; every argument error of the ops, of ``AdaptiveThreshold``, of ``SegEngine`` and of the scripts' flag check that needs no
GPU; an engine built without the flags has no adaptive state and never imports the binding."""
import argparse
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch

from adaptersis_amd import _lib, ops
from adaptersis_amd import train as T
from tests import adapt_ref as A
from tests import consist_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _logit_map(rows):
    """one teacher map [1,1,P,C] whose softmax rows are ``rows`` (P pixels of C probabilities), and the (1, P) size that reads
    it un-resampled"""
    q = torch.tensor(rows, dtype=torch.float64)
    return q.log().view(1, 1, len(rows), -1), (1, len(rows))


# ---- the restatement against hand-worked cases -----------------------------------------------------------------------------------
def test_two_classes_decide_differently():
    rows = [[0.95, 0.05], [0.85, 0.15], [0.30, 0.70], [0.45, 0.55], [0.08, 0.92]]
    t, size = _logit_map(rows)
    q = A.soft_q([t], None, size, 1.0)
    assert float((q[0, :, 0, :].t() - torch.tensor(rows, dtype=torch.float64)).abs().max()) < 1e-15
    a, conf = A.top_class(q)
    assert a.flatten().tolist() == [0, 0, 1, 1, 1]
    gate = A.class_gate(q, [0.9, 0.6])
    assert gate.flatten().tolist() == [True, False, True, False, True]        # 0.85 of class 0 is dropped, 0.70 of class 1 kept
    assert R.consist_ref(t, [t], None, size, 1.0, 0.9).gate.flatten().tolist() == [True, False, False, False, True]
    z = torch.zeros(1, 1, 5, 2, dtype=torch.float64)
    ref = A.adapt_consist_ref(z, [t], None, size, 1.0, [0.9, 0.6])
    assert ref.kept == 3 and bool((ref.dz[0, 0, [1, 3]] == 0).all()) and bool((ref.dz[0, 0, [0, 2, 4]] != 0).all())
    want = sum(ref.kd.flatten()[i] for i in (0, 2, 4)) / 5
    assert abs(float(ref.loss) - float(want)) <= 1e-15
    assert A.adapt_consist_ref(z, [t], None, size, 1.0, [0.0, -1.0]).kept == 5      # <= 0 keeps every pixel of the class
    assert A.adapt_consist_ref(z, [t], None, size, 1.0, [2.0, 0.6]).gate.flatten().tolist() == [False, False, True, False, True]
    w0 = A.adapt_consist_ref(torch.zeros(2, 1, 5, 2, dtype=torch.float64), [t.repeat(2, 1, 1, 1)], None, size, 1.0, [0.9, 0.6],
                             torch.tensor([0.0, 0.5]))
    assert w0.kept == 3


def test_argmax_tie_goes_to_the_lower_index():
    q = torch.tensor([[0.4, 0.4, 0.2], [0.2, 0.4, 0.4], [0.25, 0.5, 0.25]], dtype=torch.float64).t().reshape(1, 3, 1, 3)
    a, conf = A.top_class(q)
    assert a.flatten().tolist() == [0, 1, 1] and conf.flatten().tolist() == [0.4, 0.4, 0.5]
    assert A.class_gate(q, [0.3, 0.45, 0.0]).flatten().tolist() == [True, False, True]
    assert A.class_gate(q, [0.45, 0.3, 0.0]).flatten().tolist() == [False, True, True]
    near = A.near_pixels(q, [0.3, 0.45, 0.0], 1e-5)
    assert near.flatten().tolist() == [True, True, False]                          # the tied classes decide differently
    assert not bool(A.near_pixels(q, [0.3, 0.3, 0.3], 1e-5).any())               # tied, but both classes keep the pixel
    assert A.near_pixels(q, [0.3, 0.3, 0.500001], 1e-5).flatten().tolist() == [False, True, False]
    assert A.near_pixels(q, [0.6, 0.500001, 0.6], 1e-5).flatten().tolist() == [False, False, True]    # a confidence at its threshold


def test_statistics_by_hand():
    rows = [[0.95, 0.05], [0.30, 0.70]]
    t, size = _logit_map(rows)
    s = A.stats_ref([t], None, size, 1.0)
    assert s.shape == (4,) and torch.allclose(s, torch.tensor([1.25, 0.75, 1.65, 2.0], dtype=torch.float64), rtol=0, atol=1e-15)
    two = t.repeat(2, 1, 1, 1)
    two[0] = float("nan")
    s = A.stats_ref([two], None, size, 1.0, torch.tensor([0.0, 3.0]))              # the weight's size does not enter
    assert torch.allclose(s, torch.tensor([1.25, 0.75, 1.65, 2.0], dtype=torch.float64), rtol=0, atol=1e-15)
    assert A.stats_ref([two], None, size, 1.0, torch.tensor([0.0, 0.0])).tolist() == [0.0] * 4


def test_recursion_over_five_steps_against_a_plain_loop():
    C, lam = 3, 0.9
    g = torch.Generator().manual_seed(5)
    state = A.init_state(C)
    assert state == [1 / 3, 0.0, 1 / 3, 1 / 3, 1 / 3]
    tau, pt = 1 / 3, [1 / 3] * 3
    for step in range(5):
        p = torch.rand(3, generator=g, dtype=torch.float64)
        cnt = 100.0 + step
        sums = [float(v) * cnt for v in p / p.sum()] + [0.5 * cnt + step, cnt]
        state, thr = A.update_ref(state, sums, lam)
        tau = lam * tau + (1 - lam) * (sums[3] / cnt)
        pt = [lam * pt[c] + (1 - lam) * (sums[c] / cnt) for c in range(3)]
        assert state == [tau, float(step + 1)] + pt
        assert thr.dtype == torch.float32
        assert thr.tolist() == [float(torch.tensor(tau * v / max(pt), dtype=torch.float32)) for v in pt]
    assert state[0] > 1 / 3 and abs(sum(state[2:]) - 1.0) < 1e-12


def test_no_pixel_leaves_the_state_unchanged():
    state = [0.7, 4.0, 0.5, 0.3, 0.2]
    new, thr = A.update_ref(state, [1.0, 2.0, 3.0, 4.0, 0.0])
    assert new == state and new is not state and thr is None


def test_largest_class_gets_tau_and_uniform_classes_equal_thresholds():
    state, thr = A.update_ref(A.init_state(4), [10.0, 50.0, 30.0, 10.0, 80.0, 100.0], 0.5)
    tau = state[0]
    assert tau == 0.5 * 0.25 + 0.5 * 0.8 and thr[1] == torch.tensor(tau, dtype=torch.float32)
    assert bool((thr[[0, 2, 3]] < thr[1]).all()) and thr[0] == thr[3]
    state, thr = A.update_ref(A.init_state(4), [25.0, 25.0, 25.0, 25.0, 60.0, 100.0], 0.5)
    assert len(set(thr.tolist())) == 1 and thr[0] == torch.tensor(state[0], dtype=torch.float32)
    assert A.thresholds_of(A.init_state(8)).tolist() == [0.125] * 8


def test_pickers():
    rows = [[0.9, 0.1], [0.8, 0.2], [0.6, 0.4], [0.55, 0.45], [0.3, 0.7], [0.2, 0.8], [0.1, 0.9], [0.05, 0.95]]
    t, size = _logit_map(rows)
    q = A.soft_q([t], None, size, 1.0)
    thr, note = A.pick_class_thresholds(q)
    assert thr.dtype == torch.float32 and 0.6 < float(thr[0]) < 0.8 and 0.7 < float(thr[1]) < 0.8        # the widest mid-range gaps
    assert not bool(A.near_pixels(q, thr, 1e-5).any())
    tied, size = _logit_map(rows + [[0.5, 0.5 - 1e-7]])
    thr, note = A.pick_class_thresholds(A.soft_q([tied], None, size, 1.0))
    assert thr[0] == thr[1]                                                    # one group, one threshold
    mid = A.middle_class_thresholds(q)
    assert abs(float(mid[0]) - 0.7) < 1e-6 and abs(float(mid[1]) - 0.85) < 1e-6


# ---- the library --------------------------------------------------------------------------------------------------------------------
NAMES = ["asis_adapt_consist_loss", "asis_adapt_mix_consist_loss", "asis_adapt_nblk", "asis_adapt_stats", "asis_adapt_stats_nblk",
         "asis_adapt_tile", "asis_adapt_update"]


def test_side_library_abi_and_build():
    from adaptersis_amd import _lib_adapt, _lib_consist, _lib_mix, build
    assert build.SIDE_LIBS["libasis_adapt.so"] == ("adapt.hip",)
    assert not any(s.endswith("adapt.hip") for s in build.sources())
    assert build._deps_mtime() >= os.path.getmtime(os.path.join(ROOT, "include", "asis_adapt.h"))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asis_adapt.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(asis_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib_adapt.SIGNATURES) == NAMES
    assert os.path.dirname(_lib_adapt.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    side = ctypes.CDLL(_lib_adapt.LIB_PATH)
    others = [ctypes.CDLL(p) for p in (_lib.LIB_PATH, _lib_consist.LIB_PATH, _lib_mix.LIB_PATH)]
    for n in names:
        assert hasattr(side, n) and not any(hasattr(o, n) for o in others)
        assert n not in _lib.SIGNATURES
    assert _lib_adapt.lib() is _lib_adapt.lib() and _lib_adapt.loaded()
    lib = _lib_adapt.lib()
    tile = lib.asis_adapt_tile()
    cap = lib.asis_adapt_nblk((1 << 31) - 1)
    assert tile == _lib_consist.lib().asis_consist_tile() and cap == _lib_consist.lib().asis_consist_nblk((1 << 31) - 1) == 2048
    for N, want in ((1, 1), (tile, 1), (tile + 1, 2), (cap * tile + 1, cap)):
        assert lib.asis_adapt_nblk(N) == lib.asis_adapt_stats_nblk(N) == want
        assert ops.confidence_stats_scratch_bytes(N) == 8 * 18 * want
    for N in (0, 1 << 31):
        assert lib.asis_adapt_nblk(N) == -1 and lib.asis_adapt_stats_nblk(N) == -1
        with pytest.raises(ValueError):
            ops.confidence_stats_scratch_bytes(N)


def test_abi_argument_errors_before_any_launch():
    from adaptersis_amd import _lib_adapt
    lib, last_error = _lib_adapt.lib(), _lib.lib().asis_last_error
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def arrays(V, first, hs):
        n = max(V, 1)
        return ((ctypes.c_void_p * n)(*([first] + [p] * (n - 1))), (ctypes.c_int * n)(*[hs] * n), (ctypes.c_int * n)(*[2] * n),
                (ctypes.c_int * n)(*[0] * n))

    def loss(entry="asis_adapt_consist_loss", logits=p, teachers="list", V=1, B=1, h=2, w=2, H=2, W=2, C=2, temp=1.0, thr=p, partial=p,
             out=p, kept=p, dz=p, hs=2, first=p, flips="list", sel=p, donor=p):
        ptrs, th, tw, fl = arrays(V, first, hs)
        mix = (sel, donor) if "mix" in entry else ()
        return getattr(lib, entry)(None, logits, B, h, w, ptrs if teachers == "list" else teachers, th, tw,
                                   fl if flips == "list" else flips, V, H, W, C, temp, thr, None, *mix, 1.0, 0, partial, out, kept, dz)

    cases = ((dict(logits=None), b"null"), (dict(teachers=None), b"null"), (dict(flips=None), b"null"), (dict(partial=None), b"null"),
             (dict(out=None), b"null"), (dict(kept=None), b"null"), (dict(dz=None), b"null"), (dict(thr=None), b"class_threshold"),
             (dict(first=None), b"teachers[0]"), (dict(V=0), b"V=0"), (dict(V=9), b"V=9"), (dict(C=0), b"C=0"), (dict(C=17), b"C=17"),
             (dict(B=0), b"non-positive"), (dict(h=0), b"non-positive"), (dict(W=-3), b"non-positive"), (dict(hs=0), b"teacher map 0"),
             (dict(temp=0.0), b"temperature"), (dict(temp=float("nan")), b"temperature"),
             (dict(B=1 << 11, H=1 << 10, W=1 << 10), b"2^31"), (dict(partial=p + 4), b"aligned"))
    for entry in ("asis_adapt_consist_loss", "asis_adapt_mix_consist_loss"):
        for kw, word in cases:
            assert loss(entry, **kw) == _lib.ASIS_EINVAL, (entry, kw)
            assert word in last_error() and entry.encode() in last_error(), (entry, kw, last_error())
    for kw in (dict(sel=None), dict(donor=None)):
        assert loss("asis_adapt_mix_consist_loss", **kw) == _lib.ASIS_EINVAL and b"sel, donor" in last_error()

    def stats(teachers="list", V=1, B=1, H=2, W=2, C=2, temp=1.0, partial=p, sums=p, hs=2, first=p, flips="list"):
        ptrs, th, tw, fl = arrays(V, first, hs)
        return lib.asis_adapt_stats(None, B, ptrs if teachers == "list" else teachers, th, tw, fl if flips == "list" else flips, V, H, W,
                                    C, temp, None, partial, sums)

    for kw, word in ((dict(teachers=None), b"null"), (dict(flips=None), b"null"), (dict(partial=None), b"null"), (dict(sums=None), b"null"),
                     (dict(first=None), b"teachers[0]"), (dict(V=0), b"V=0"), (dict(V=9), b"V=9"), (dict(C=0), b"C=0"),
                     (dict(C=17), b"C=17"), (dict(B=0), b"non-positive"), (dict(H=0), b"non-positive"), (dict(hs=0), b"teacher map 0"),
                     (dict(temp=0.0), b"temperature"), (dict(B=1 << 11, H=1 << 10, W=1 << 10), b"2^31"),
                     (dict(partial=p + 4), b"aligned"), (dict(sums=p + 4), b"aligned")):
        assert stats(**kw) == _lib.ASIS_EINVAL, kw
        assert word in last_error(), (kw, last_error())

    def update(sums=p, state=p, thr=p, C=2, m=0.9):
        return lib.asis_adapt_update(None, sums, state, thr, C, m)

    for kw, word in ((dict(sums=None), b"null"), (dict(state=None), b"null"), (dict(thr=None), b"null"), (dict(C=0), b"C=0"),
                     (dict(C=17), b"C=17"), (dict(m=1.0), b"momentum"), (dict(m=-0.1), b"momentum"), (dict(m=float("nan")), b"momentum"),
                     (dict(sums=p + 4), b"aligned"), (dict(state=p + 4), b"aligned")):
        assert update(**kw) == _lib.ASIS_EINVAL, kw
        assert word in last_error(), (kw, last_error())


def test_op_argument_errors():
    z, t = torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3)
    thr = torch.zeros(3)
    with pytest.raises(ValueError, match="exclude each other"):
        ops.consistency_loss(z, t, (4, 4), threshold=0.5, class_threshold=thr)
    for bad in ([0.5, 0.5, 0.5], thr.double(), torch.zeros(3, 1), torch.zeros(6)[::2]):
        with pytest.raises(ValueError, match="class_threshold"):
            ops.consistency_loss(z, t, (4, 4), class_threshold=bad)
    with pytest.raises(_lib.AsisError):                                        # no CPU fallback
        ops.consistency_loss(z, t, (4, 4), class_threshold=thr)
    # confidence_stats
    for bad, word in ((dict(maps=[]), "views"), (dict(maps=[t] * 9), "views"), (dict(maps=[t.double()]), "float32"),
                      (dict(maps=[t, torch.zeros(2, 2, 2, 3)]), "same"), (dict(maps=[torch.zeros(1, 2, 2, 17)]), "C=17"),
                      (dict(flips=[True, False]), "flips"), (dict(temperature=0.0), "temperature"), (dict(size=(0, 4)), "size"),
                      (dict(sample_weight=torch.ones(2)), "sample_weight"), (dict(sample_weight=torch.ones(1, dtype=torch.float64)), "sample_weight"),
                      (dict(out=torch.zeros(5)), "out"), (dict(out=torch.zeros(4, dtype=torch.float64)), "out")):
        kw = dict(maps=[t], size=(4, 4))
        kw.update(bad)
        maps, size = kw.pop("maps"), kw.pop("size")
        with pytest.raises(ValueError, match=word):
            ops.confidence_stats(maps, size, **kw)
    with pytest.raises(_lib.AsisError):
        ops.confidence_stats(t, (4, 4))
    # adaptive_threshold_update
    d = lambda n: torch.zeros(n, dtype=torch.float64)
    for args, word in (((d(5), d(5), torch.zeros(3, dtype=torch.float64)), "thr"), ((d(5), d(5), torch.zeros(17)), "C=17"),
                       ((d(4), d(5), torch.zeros(3)), "sums"), ((d(5).float(), d(5), torch.zeros(3)), "sums"),
                       ((d(5), d(6), torch.zeros(3)), "state"), ((d(5), d(5), torch.zeros(3), 1.0), "momentum"),
                       ((d(5), d(5), torch.zeros(3), -0.5), "momentum")):
        with pytest.raises(ValueError, match=word):
            ops.adaptive_threshold_update(*args)
    with pytest.raises(_lib.AsisError):
        ops.adaptive_threshold_update(d(5), d(5), torch.zeros(3))


def test_adaptive_threshold_object():
    from adaptersis_amd.adaptive_threshold import AdaptiveThreshold
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="num_classes"):
            AdaptiveThreshold(bad)
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="momentum"):
            AdaptiveThreshold(3, bad)
    a = AdaptiveThreshold(4, 0.9, "cpu")
    assert a.state.tolist() == A.init_state(4) and a.thresholds.tolist() == [0.25] * 4 and a.thresholds.dtype == torch.float32
    assert a.state.dtype == torch.float64 and a.momentum == 0.9
    sd = a.state_dict()
    sd["state"][0] = 0.75
    sd["thresholds"][2] = 0.5
    b = AdaptiveThreshold(4, 0.9, "cpu")
    b.load_state_dict(sd)
    assert b.state[0] == 0.75 and b.thresholds[2] == 0.5 and a.state[0] == 0.25
    with pytest.raises(ValueError, match="classes"):
        AdaptiveThreshold(3, 0.9, "cpu").load_state_dict(sd)
    with pytest.raises(_lib.AsisError):                                        # the kernels run on the device only
        a.update([torch.zeros(1, 2, 2, 4)], None, (4, 4))


# ---- the engine and the scripts ---------------------------------------------------------------------------------------------------
def test_engine_argument_errors_and_fixed_list():
    from tests.test_lora_cpu import _engine
    kw = dict(train_backbone=False, ema_decay=0.9, teacher="ema")
    with pytest.raises(ValueError, match="needs a teacher"):
        _engine(train_backbone=False, distill_class_thresholds="adaptive")
    with pytest.raises(ValueError, match="exclude each other"):
        _engine(distill_class_thresholds="adaptive", distill_threshold=0.5, **kw)
    with pytest.raises(ValueError, match="'adaptive'"):
        _engine(distill_class_thresholds="freematch", **kw)
    for bad in ([0.5], [0.5, 0.6, 0.7], [0.5, float("nan")], [float("inf"), 0.5]):
        with pytest.raises(ValueError, match="2 finite values"):
            _engine(distill_class_thresholds=bad, **kw)
    for bad in (1.0, -0.1):
        with pytest.raises(ValueError, match="momentum"):
            _engine(distill_class_thresholds="adaptive", distill_adaptive_momentum=bad, **kw)
    eng = _engine(distill_class_thresholds=[0.9, 1.5], **kw)
    assert eng.adaptive is None and eng.class_thresholds.tolist() == [float(torch.tensor(0.9, dtype=torch.float32)), 1.5]
    eng = _engine(distill_class_thresholds="adaptive", distill_adaptive_momentum=0.5, **kw)
    assert eng.adaptive.momentum == 0.5 and eng.class_thresholds is eng.adaptive.thresholds and eng.class_thresholds.tolist() == [0.5, 0.5]


def test_default_engine_has_no_adaptive_state_and_never_imports_the_binding():
    code = ("import sys\n"
            "from tests.test_lora_cpu import _engine\n"
            "eng = _engine(train_backbone=False, ema_decay=0.9, teacher='ema', distill_threshold=0.6)\n"
            "assert eng.adaptive is None and eng.class_thresholds is None\n"
            "import adaptersis_amd.train\n"
            "assert 'adaptersis_amd._lib_adapt' not in sys.modules and 'adaptersis_amd.adaptive_threshold' not in sys.modules\n"
            "print('clean')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and "clean" in r.stdout, r.stderr[-2000:]


def _ns(**kw):
    return argparse.Namespace(arch="vit_large", **kw)


def test_check_distill_args_and_the_parsers():
    from adaptersis_amd import train_mla, train_multi_class
    ok = T.check_distill_args
    base = dict(distill_teacher="ema", ema_decay=0.9)
    assert ok(_ns(**base, distill_adaptive_threshold=True, distill_adaptive_momentum=0.99)) is None
    assert ok(_ns(**base, distill_class_thresholds=[0.9, 0.6])) is None
    assert ok(_ns(**base, distill_class_thresholds=[0.9, 0.6], num_classes=2)) is None
    assert "needs --distill_teacher" in ok(_ns(distill_adaptive_threshold=True))
    assert "needs --distill_teacher" in ok(_ns(distill_class_thresholds=[0.5, 0.5]))
    assert "needs --distill_teacher" in ok(_ns(distill_adaptive_momentum=0.9))
    assert "pick one" in ok(_ns(**base, distill_class_thresholds=[0.5, 0.5], distill_adaptive_threshold=True))
    assert "not with" in ok(_ns(**base, distill_threshold=0.5, distill_adaptive_threshold=True))
    assert "not with" in ok(_ns(**base, distill_threshold=0.5, distill_class_thresholds=[0.5, 0.5]))
    assert "finite" in ok(_ns(**base, distill_class_thresholds=[0.5, float("nan")]))
    assert "3 values for --num_classes 2" in ok(_ns(**base, distill_class_thresholds=[0.5, 0.5, 0.5], num_classes=2))
    assert "needs --distill_adaptive_threshold" in ok(_ns(**base, distill_adaptive_momentum=0.9))
    for bad in (1.0, -0.5):
        assert "[0, 1)" in ok(_ns(**base, distill_adaptive_threshold=True, distill_adaptive_momentum=bad))
    for mod in (T, train_mla, train_multi_class):
        p = mod.get_args_parser()
        a = p.parse_args(["--ema_decay", "0.9", "--distill_teacher", "ema", "--distill_adaptive_threshold", "--distill_adaptive_momentum", "0.99"])
        kw = T._distill_engine_args(a, "ema")
        assert kw["distill_class_thresholds"] == "adaptive" and kw["distill_adaptive_momentum"] == 0.99 and kw["distill_threshold"] is None
        nc = int(p.get_default("num_classes") or 2)                              # the multi-class script knows its class count
        vals = [0.9, 0.6] + [0.5] * (nc - 2)
        a = p.parse_args(["--ema_decay", "0.9", "--distill_teacher", "ema", "--distill_class_thresholds"] + [str(v) for v in vals])
        assert T._distill_engine_args(a, "ema")["distill_class_thresholds"] == vals
        plain = T._distill_engine_args(p.parse_args(["--ema_decay", "0.9", "--distill_teacher", "ema"]), "ema")
        assert "distill_class_thresholds" not in plain and "distill_adaptive_momentum" not in plain
        for bad in (["--distill_adaptive_threshold"], ["--ema_decay", "0.9", "--distill_teacher", "ema", "--distill_adaptive_threshold",
                                                      "--distill_threshold", "0.5"]):
            with pytest.raises(SystemExit):
                p.parse_args(bad)


def test_checkpoint_entry_round_trip_and_older_checkpoint(capsys):
    from adaptersis_amd.adaptive_threshold import AdaptiveThreshold
    eng = argparse.Namespace(distill_step=0, adaptive=AdaptiveThreshold(3, 0.9, "cpu"))
    saved = AdaptiveThreshold(3, 0.9, "cpu")
    saved.state[0], saved.thresholds[1] = 0.8, 0.6
    T._DistillEntry(eng).load_state_dict({"step": 7, "adaptive": saved.state_dict()})
    assert eng.distill_step == 7 and torch.equal(eng.adaptive.state, saved.state) and torch.equal(eng.adaptive.thresholds, saved.thresholds)
    fresh = argparse.Namespace(distill_step=0, adaptive=AdaptiveThreshold(3, 0.9, "cpu"))
    T._DistillEntry(fresh).load_state_dict({"step": 3})
    assert fresh.distill_step == 3 and fresh.adaptive.state.tolist() == A.init_state(3)
    assert "no adaptive thresholds" in capsys.readouterr().out
    T._DistillEntry(argparse.Namespace(distill_step=0)).load_state_dict({"step": 2})           # an engine without them: as before
