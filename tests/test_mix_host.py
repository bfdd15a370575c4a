"""CPU: the host draws of batch mixing (``tools.mix.MixSampler``); the ABI of libasis_mix.so (include/asis_mix.h: every declared
symbol exported and bound, none of them in another library; the build lists the library and sees its header) and the argument
errors of its entries that need no GPU; the restatement tests/mix_ref.py against tests/consist_ref.py where nothing is mixed; the
flag checks of the training scripts."""
import argparse
import ctypes
import os
import re

import pytest
import torch

from adaptersis_amd import _lib, _lib_consist, _lib_distill, _lib_mix, ops
from adaptersis_amd import train as T
from adaptersis_amd import train_mla, train_multi_class
from adaptersis_amd.tools.mix import KINDS, MixSampler
from tests import consist_ref as R
from tests import mix_ref as M
from tests.bound_helpers import _gen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the draws -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cutmix", "classmix"])
@pytest.mark.parametrize("B,H,W", [(2, 5, 7), (3, 224, 224), (12, 588, 588), (7, 1, 9)])
def test_draw_tables(kind, B, H, W):
    s = MixSampler(kind, seed=3, num_classes=8)
    shifts = set()
    for step in range(120):
        t = s.draw(B, H, W, step)
        assert {k: (v.dtype, tuple(v.shape)) for k, v in t.items()} == {
            "donor": (torch.int32, (B,)), "kind": (torch.int32, (B,)), "box": (torch.int32, (B, 4)), "order": (torch.uint8, (B, 16))}
        assert all(not v.is_cuda and v.is_contiguous() for v in t.values())
        d = t["donor"].tolist()
        assert sorted(d) == list(range(B)) and all(d[b] != b for b in range(B))               # a fixed-point-free permutation
        assert len({(d[b] - b) % B for b in range(B)}) == 1                                   # one shift for the whole batch
        shifts.add((d[0] - 0) % B)
        assert bool((t["kind"] == KINDS[kind]).all())                                         # p = 1
        y0, x0, y1, x1 = t["box"].unbind(1)
        assert bool(((0 <= y0) & (y0 <= y1) & (y1 <= H) & (0 <= x0) & (x0 <= x1) & (x1 <= W)).all())
        assert all(sorted(row) == list(range(16)) for row in t["order"].tolist())
    assert shifts == set(range(1, B))


def test_draw_is_a_function_of_seed_rank_step():
    s = MixSampler("classmix", p=0.5, seed=11, num_classes=3)
    same = lambda a, b: all(torch.equal(a[k], b[k]) for k in a)
    a = s.draw(6, 64, 48, 5, rank=1)
    s.draw(6, 64, 48, 9, rank=1)                                                              # stateless: a draw in between changes nothing
    assert same(a, s.draw(6, 64, 48, 5, rank=1)) and same(a, MixSampler("classmix", p=0.5, seed=11, num_classes=3).draw(6, 64, 48, 5, 1))
    assert not same(a, s.draw(6, 64, 48, 6, rank=1)) and not same(a, s.draw(6, 64, 48, 5, rank=0))
    assert not same(a, MixSampler("classmix", p=0.5, seed=12, num_classes=3).draw(6, 64, 48, 5, 1))
    # p thins the kinds and nothing else: the other tables are those of p = 1
    full = MixSampler("classmix", p=1.0, seed=11, num_classes=3).draw(6, 64, 48, 5, 1)
    assert all(torch.equal(a[k], full[k]) for k in ("donor", "box", "order"))
    kinds = torch.cat([s.draw(8, 16, 16, t)["kind"] for t in range(200)])
    assert set(kinds.tolist()) == {0, 2} and 0.4 < float((kinds == 2).float().mean()) < 0.6


def test_nothing_is_mixed_at_p_zero_and_in_a_batch_of_one():
    for step in range(10):
        assert not bool(MixSampler("cutmix", p=0.0).draw(4, 8, 8, step)["kind"].any())
        one = MixSampler("classmix").draw(1, 8, 8, step)
        assert one["kind"].tolist() == [0] and one["donor"].tolist() == [0]
    for bad in (dict(kind="mixup"), dict(kind="cutmix", p=1.5), dict(kind="cutmix", p=-0.1), dict(kind="cutmix", num_classes=17)):
        with pytest.raises(ValueError):
            MixSampler(**bad)
    with pytest.raises(ValueError):
        MixSampler("cutmix").draw(0, 8, 8, 0)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def test_restatement_of_the_sets_and_of_an_unmixed_loss():
    tgt = torch.tensor([[[0, 0, 3], [3, 5, 255]], [[0, 0, 0], [0, 0, 0]], [[1, -100, 2], [7, 7, 9]]])
    assert M.presence(tgt, 8) == [{0, 3, 5}, {0}, {1, 2, 7}] and M.presence(tgt, 16)[2] == {1, 2, 7, 9}
    order = torch.arange(16, dtype=torch.uint8).flip(0).repeat(3, 1)                          # 15, 14, ..., 0
    t = {"donor": torch.tensor([2, 0, 1], dtype=torch.int32), "kind": torch.tensor([2, 2, 2], dtype=torch.int32),
         "box": torch.zeros((3, 4), dtype=torch.int32), "order": order}
    assert M.pasted_sets(tgt, t, 8) == [{7, 2}, {5}, set()]                                   # ceil(3/2), ceil(2/2), an empty P
    assert M.pasted_sets(tgt, t, 8, background=True) == [{7, 2}, {5, 3}, {0}]
    out, tout, sel, pasted = M.mix_ref(torch.arange(54, dtype=torch.float32).view(3, 3, 2, 3), tgt, t, 8)
    assert sel.tolist() == [[[0, 0, 1], [1, 1, 0]], [[0, 0, 0], [0, 1, 0]], [[0, 0, 0], [0, 0, 0]]] and pasted.tolist() == [3, 1, 0]
    assert tout.tolist() == [[[0, 0, 2], [7, 7, 255]], [[0, 0, 0], [0, 5, 0]], tgt[2].tolist()]
    assert out[0, 1].tolist() == [[6.0, 7.0, 44.0], [45.0, 46.0, 11.0]]
    # sel == 0: the mixed loss is consist_ref's; sel == 1: consist_ref's on the maps of the donors
    g = _gen(4)
    z = torch.randn(2, 5, 7, 3, generator=g, dtype=torch.float64)
    ts, flips = [torch.randn(2, 6, 4, 3, generator=g, dtype=torch.float64), torch.randn(2, 9, 3, 3, generator=g, dtype=torch.float64)], [False, True]
    plain = R.consist_ref(z, ts, flips, (13, 11), 2.0, 0.5)
    none = M.mixed_consist_ref(z, ts, flips, (13, 11), 2.0, torch.zeros(2, 13, 11, dtype=torch.uint8), [1, 0], 0.5)
    swap = M.mixed_consist_ref(z, ts, flips, (13, 11), 2.0, torch.ones(2, 13, 11, dtype=torch.uint8), [1, 0], 0.5)
    want = R.consist_ref(z, [t[[1, 0]] for t in ts], flips, (13, 11), 2.0, 0.5)
    assert torch.equal(none.loss, plain.loss) and torch.equal(none.dz, plain.dz) and none.kept == plain.kept
    assert torch.equal(swap.loss, want.loss) and torch.equal(swap.dz, want.dz) and swap.kept == want.kept
    assert torch.equal(M.mixed_confidence(ts, flips, (13, 11), 2.0, torch.ones(2, 13, 11, dtype=torch.uint8), [1, 0]), want.conf)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_side_library_abi():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "asis_mix.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(asis_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib_mix.SIGNATURES) == ["asis_mix_apply", "asis_mix_class_sets", "asis_mix_consist_loss", "asis_mix_consist_nblk",
                                                    "asis_mix_consist_tile", "asis_mix_nblk", "asis_mix_tile"]
    assert os.path.dirname(_lib_mix.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    side = ctypes.CDLL(_lib_mix.LIB_PATH)
    others = [ctypes.CDLL(p) for p in (_lib.LIB_PATH, _lib_distill.LIB_PATH, _lib_consist.LIB_PATH)]
    for n in names:
        assert hasattr(side, n) and not any(hasattr(o, n) for o in others)
        assert n not in _lib.SIGNATURES and n not in _lib_distill.SIGNATURES and n not in _lib_consist.SIGNATURES
    assert _lib_mix.lib() is _lib_mix.lib() and _lib_mix.loaded()


def test_build_lists_the_library_and_sees_its_header():
    from adaptersis_amd import build
    assert build.SIDE_LIBS["libasis_mix.so"] == ("mix.hip",)
    assert not any(s.endswith("mix.hip") for s in build.sources())
    for hdr in ("include/asis_mix.h", "adaptersis_amd/csrc/soft_target.h"):
        assert build._deps_mtime() >= os.path.getmtime(os.path.join(ROOT, *hdr.split("/"))), hdr


def test_nblk_and_tile_need_no_gpu():
    lib = _lib_mix.lib()
    tile = lib.asis_mix_tile()
    assert tile > 0 and tile % 256 == 0
    cap = lib.asis_mix_nblk(1, (1 << 31) - 1)
    assert cap >= 256
    for B, HW, want in ((1, 1, 1), (3, tile - 1, 3), (3, tile, 3), (3, tile + 1, 6), (2, cap // 2 * tile, cap), (2, cap // 2 * tile + 1, cap)):
        assert lib.asis_mix_nblk(B, HW) == want, (B, HW)
    for B, HW in ((0, 5), (-1, 5), (1, 0), (1, 1 << 31), (2, 1 << 30), (1 << 16, 1 << 15)):
        assert lib.asis_mix_nblk(B, HW) == -1 and b"2^31" in _lib.lib().asis_last_error()
    assert lib.asis_mix_consist_tile() == _lib_consist.lib().asis_consist_tile()
    for N in (1, 1000, 1 << 20, (1 << 31) - 1):
        assert lib.asis_mix_consist_nblk(N) == _lib_consist.lib().asis_consist_nblk(N)
    for N in (0, -5, 1 << 31):
        assert lib.asis_mix_consist_nblk(N) == -1 and b"2^31" in _lib.lib().asis_last_error()


def test_argument_errors_before_any_launch():
    lib, last_error = _lib_mix.lib(), _lib.lib().asis_last_error
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    q = p + 256

    def sets(target=p, donor=p, kind=p, order=p, B=1, H=2, W=2, C=2, out=p):
        return lib.asis_mix_class_sets(None, target, donor, kind, order, B, H, W, C, 0, out)

    def apply(inp=p, target=p, donor=p, kind=p, box=p, B=1, H=2, W=2, inp_out=q, target_out=q, sel=q, pasted=q):
        return lib.asis_mix_apply(None, inp, target, donor, kind, box, None, B, H, W, inp_out, target_out, sel, pasted)

    def loss(logits=p, teachers="list", V=1, B=1, h=2, w=2, H=2, W=2, C=2, temp=1.0, thr=0.5, sel=p, donor=p, partial=p, out=p, kept=p,
             dz=p, hs=2, first=p):
        ptrs = (ctypes.c_void_p * max(V, 1))(*([first] + [p] * (max(V, 1) - 1)))
        th, tw, fl = ((ctypes.c_int * max(V, 1))(*[v] * max(V, 1)) for v in (hs, 2, 0))
        return lib.asis_mix_consist_loss(None, logits, B, h, w, ptrs if teachers == "list" else teachers, th, tw, fl, V, H, W, C, temp,
                                         thr, None, sel, donor, 1.0, 0, partial, out, kept, dz)

    cases = [(sets, dict(target=None), b"null"), (sets, dict(donor=None), b"null"), (sets, dict(kind=None), b"null"),
             (sets, dict(order=None), b"null"), (sets, dict(out=None), b"null"), (sets, dict(C=17), b"C=17"), (sets, dict(C=0), b"C=0"),
             (sets, dict(B=0), b"non-positive"), (sets, dict(H=0), b"non-positive"), (sets, dict(W=-2), b"non-positive"),
             (sets, dict(B=1 << 11, H=1 << 10, W=1 << 10), b"2^31"),
             (apply, dict(inp=None), b"null"), (apply, dict(target=None), b"null"), (apply, dict(donor=None), b"null"),
             (apply, dict(kind=None), b"null"), (apply, dict(box=None), b"null"), (apply, dict(inp_out=None), b"null"),
             (apply, dict(target_out=None), b"null"), (apply, dict(sel=None), b"null"), (apply, dict(pasted=None), b"null"),
             (apply, dict(B=0), b"non-positive"), (apply, dict(H=-1), b"non-positive"), (apply, dict(W=0), b"non-positive"),
             (apply, dict(inp_out=p), b"aliases"), (apply, dict(target_out=p), b"aliases"),
             (apply, dict(B=1 << 11, H=1 << 10, W=1 << 10), b"2^31"), (apply, dict(B=1, H=1 << 16, W=1 << 16), b"2^31"),
             (loss, dict(sel=None), b"null"), (loss, dict(donor=None), b"null"), (loss, dict(logits=None), b"null"),
             (loss, dict(teachers=None), b"null"), (loss, dict(partial=None), b"null"), (loss, dict(out=None), b"null"),
             (loss, dict(kept=None), b"null"), (loss, dict(dz=None), b"null"), (loss, dict(first=None), b"teachers[0]"),
             (loss, dict(V=0), b"V=0"), (loss, dict(V=9), b"V=9"), (loss, dict(C=0), b"C=0"), (loss, dict(C=17), b"C=17"),
             (loss, dict(B=0), b"non-positive"), (loss, dict(hs=0), b"teacher map 0"), (loss, dict(temp=0.0), b"temperature"),
             (loss, dict(thr=1.5), b"threshold"), (loss, dict(thr=float("nan")), b"threshold"),
             (loss, dict(B=1 << 11, H=1 << 10, W=1 << 10), b"2^31"), (loss, dict(partial=p + 4), b"aligned")]
    for fn, kw, word in cases:
        assert fn(**kw) == _lib.ASIS_EINVAL, (fn.__name__, kw)
        assert word in last_error() and b"asis_mix_" in last_error(), (fn.__name__, kw, last_error())
    with pytest.raises(ValueError):
        _lib.check(sets(C=17), "asis_mix_class_sets")


def test_ops_have_no_cpu_fallback_and_check_on_the_host():
    t = MixSampler("cutmix").draw(2, 4, 4, 0)
    with pytest.raises(_lib.AsisError):
        ops.mix_batch(torch.zeros(2, 3, 4, 4), torch.zeros(2, 4, 4, dtype=torch.int64), t, 2)
    z = torch.zeros(1, 2, 2, 3)
    with pytest.raises(_lib.AsisError):
        ops.consistency_loss(z, z, (4, 4), mix=(torch.zeros(1, 4, 4, dtype=torch.uint8), [0]))
    for bad in ([2, 0], [-1, 0], [0], torch.tensor([0, 1]), torch.tensor([0.0, 1.0])):
        with pytest.raises(ValueError, match="donor"):
            ops._host_donor("op", bad, 2)
    assert ops._host_donor("op", (1, 0), 2).tolist() == [1, 0] and ops._host_donor("op", torch.tensor([1, 0], dtype=torch.int32), 2).dtype == torch.int32


# ---- the flags ---------------------------------------------------------------------------------------------------------------------
def test_flag_checks():
    ok = T.check_mix_args
    ns = lambda **kw: argparse.Namespace(**kw)
    assert ok(ns()) is None and ok(ns(mix=None, mix_p=None, mix_seed=None, mix_background=False)) is None
    assert ok(ns(mix="cutmix")) is None and ok(ns(mix="classmix", mix_p=0.5, mix_seed=0, mix_background=True, batch_size_per_gpu=2)) is None
    for flag, value in (("mix_p", 0.5), ("mix_seed", 0), ("mix_seed", 7), ("mix_background", True)):
        assert f"--{flag} needs --mix" in ok(ns(**{flag: value}))
    assert "--mix must be one of" in ok(ns(mix="mixup"))
    for p in (-0.1, 1.5, float("nan")):
        assert "--mix_p must be a probability" in ok(ns(mix="cutmix", mix_p=p))
    assert "--batch_size_per_gpu of at least 2" in ok(ns(mix="cutmix", batch_size_per_gpu=1))
    assert T._mix_engine_args(ns()) == {} and T._mix_engine_args(ns(mix="classmix", mix_p=None, mix_seed=None)) == dict(
        mix="classmix", mix_p=1.0, mix_seed=0, mix_background=False)
    # every script's parser refuses them as usage errors, and train_seg before any process group is opened
    for mod in (T, train_mla, train_multi_class):
        p = mod.get_args_parser()
        a = p.parse_args(["--mix", "classmix", "--mix_p", "0.25", "--mix_seed", "5", "--mix_background"])
        assert T._mix_engine_args(a) == dict(mix="classmix", mix_p=0.25, mix_seed=5, mix_background=True)
        assert T._mix_engine_args(p.parse_args([])) == {}
        for bad in (["--mix_p", "0.5"], ["--mix_background"], ["--mix", "cutmix", "--mix_p", "2"], ["--mix", "other"],
                    ["--mix", "cutmix", "--batch_size_per_gpu", "1"]):
            with pytest.raises(SystemExit):
                p.parse_args(bad)
    with pytest.raises(ValueError, match="at least 2"):
        T.train_seg(argparse.Namespace(arch="vit_large", mix="cutmix", batch_size_per_gpu=1))
    with pytest.raises(ValueError, match="needs --mix"):
        T.train_seg(argparse.Namespace(arch="vit_large", mix_p=0.5))
