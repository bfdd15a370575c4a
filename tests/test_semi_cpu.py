"""CPU: the float64 restatement of the loss with an ignore label (tests/semi_ref.py) against ``_loss_ref`` of
tests/test_gpu_loss_kernels.py; the ABI of libasis_semi.so (include/asis_semi.h: every declared symbol exported and bound, none of
them in libasis_hip.so) and the argument errors of ``asis_semi_loss`` that need no GPU; ``MixSampler.draw(groups=)``;
``tools.dataset.UnlabelledFrames`` on a folder built as tests/test_endovis_datasets.py builds its folders; the refusals of the
training scripts' semi-supervision flags."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from adaptersis_amd import _lib, _lib_semi, ops
from tests import semi_ref as R
from tests.bound_helpers import _gen
from tests.test_gpu_loss_kernels import GS, LOSSES, _loss_ref

SHAPE = (3, 4, 6, 5, 17, 13)      # B, C, h, w, H, W


def _inputs(*key):
    B, C, h, w, H, W = SHAPE
    gen = _gen(41, *key)
    lg = torch.randn(B, h, w, C, generator=gen, dtype=torch.float64) * 1.5 + 1.0
    tg = torch.randint(0, C, (B, H, W), generator=gen)
    wts = torch.linspace(0.2, 2.0, C, dtype=torch.float64)
    wts[1] = 0.0
    return lg, tg, wts


def _close(a, b) -> bool:
    return bool(torch.allclose(a, b, rtol=1e-12, atol=1e-13 * max(1.0, float(b.abs().max()))))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LOSSES))
def test_nothing_ignored_is_loss_ref(name):
    n_region, mode, eps, n_ce, weighted = LOSSES[name]
    lg, tg, wts = _inputs(1)
    wts = wts if weighted else None
    r = R.semi_ref(lg, tg, 255, n_region, mode, eps, n_ce, wts, torch.float64, GS)
    d = _loss_ref(lg, tg, n_region, mode, eps, n_ce, wts, torch.float64)
    assert _close(r["loss"], d["loss"]) and _close(r["sums"], d["sums"]) and _close(r["dz"], d["dz"])
    assert r["P"] == SHAPE[0] and bool((r["valid"] == SHAPE[4] * SHAPE[5]).all())
    assert abs(r["rho"] - d["rho"]) <= 1e-12 and abs(r["D"] - d["D"]) <= 1e-12 and abs(r["A"] - d["A"]) <= 1e-12


@pytest.mark.parametrize("name", list(LOSSES))
@pytest.mark.parametrize("absent", [(0,), (1,), (0, 2)])
def test_whole_samples_ignored_is_loss_ref_of_the_rest(name, absent):
    n_region, mode, eps, n_ce, weighted = LOSSES[name]
    lg, tg, wts = _inputs(2)
    wts = wts if weighted else None
    keep = [b for b in range(SHAPE[0]) if b not in absent]
    ig = tg.clone()
    ig[list(absent)] = -1
    r = R.semi_ref(lg, ig, -1, n_region, mode, eps, n_ce, wts, torch.float64, GS)
    d = _loss_ref(lg[keep], tg[keep], n_region, mode, eps, n_ce, wts, torch.float64)
    assert _close(r["loss"], d["loss"]) and _close(r["sums"][keep], d["sums"]) and _close(r["dz"][keep], d["dz"])
    assert float(r["dz"][list(absent)].abs().max()) == 0.0 and float(r["sums"][list(absent)].abs().max()) == 0.0
    assert r["P"] == len(keep) and r["valid"].tolist() == [0 if b in absent else SHAPE[4] * SHAPE[5] for b in range(SHAPE[0])]


@pytest.mark.parametrize("name", list(LOSSES))
def test_no_label_at_all_and_no_weight_at_all(name):
    n_region, mode, eps, n_ce, weighted = LOSSES[name]
    lg, tg, wts = _inputs(3)
    r = R.semi_ref(lg, torch.full_like(tg, 255), 255, n_region, mode, eps, n_ce, wts if weighted else None, torch.float64, GS)
    assert r["P"] == 0 and float(r["loss"]) == 0.0 and float(r["dz"].abs().max()) == 0.0 and bool(torch.isfinite(r["dz"]).all())
    # only pixels of the class without CE weight are valid: sum v w = 0, the CE term is 0, everything stays finite
    ig = R.ignore_pattern(tg, "zero_w", 255, None)
    z = R.semi_ref(lg, ig, 255, n_region, mode, eps, n_ce, wts, torch.float64, GS)
    assert z["ce"] == 0.0 and bool(torch.isfinite(z["loss"])) and bool(torch.isfinite(z["dz"]).all())
    assert float(z["dz"][ig == 255].abs().max()) == 0.0
    if mode == ops.LOSS_NONE:
        assert float(z["loss"]) == 0.0 and float(z["dz"].abs().max()) == 0.0


def test_partly_ignored_gradient_is_zero_where_ignored_and_sums_count_valid_pixels():
    lg, tg, wts = _inputs(4)
    gen = _gen(42)
    for pattern in ("rand30", "onepix", "oneclass", "sample0"):
        ig = R.ignore_pattern(tg, pattern, 255, gen)
        v = ig != 255
        r = R.semi_ref(lg, ig, 255, 1, ops.LOSS_DICE, 10e-20, 1, wts, torch.float64, GS)
        assert float(r["dz"][~v].abs().max()) == 0.0 and float(r["dz"][v].abs().max()) > 0.0
        assert torch.equal(r["valid"], v.sum((1, 2)))
        assert torch.equal(r["sums"][..., 2].long(), torch.stack([torch.bincount(ig[b][v[b]], minlength=SHAPE[1]) for b in range(SHAPE[0])]))
        assert abs(float(r["sums"][..., 2].sum()) - float(v.sum())) == 0.0


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------
def test_side_library_abi():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "asis_semi.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(asis_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib_semi.SIGNATURES) == ["asis_semi_loss", "asis_semi_partial_stride"]
    assert os.path.dirname(_lib_semi.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    side, main = ctypes.CDLL(_lib_semi.LIB_PATH), ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(side, n) and not hasattr(main, n) and n not in _lib.SIGNATURES
    for n in ("asis_seg_loss_fwd", "asis_seg_loss_bwd", "asis_dice_nblk"):       # the parent loss stays where it was
        assert hasattr(main, n) and n in _lib.SIGNATURES
    assert _lib_semi.lib() is _lib_semi.lib() and _lib_semi.loaded()


def test_build_lists_the_library_and_sees_its_headers():
    from adaptersis_amd import build
    assert build.SIDE_LIBS["libasis_semi.so"] == ("semi.hip",)
    assert not any(s.endswith("semi.hip") for s in build.sources()) and any(s.endswith("loss.hip") for s in build.sources())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for hdr in ("include/asis_semi.h", "adaptersis_amd/csrc/seg_loss_body.h"):
        assert build._deps_mtime() >= os.path.getmtime(os.path.join(root, *hdr.split("/"))), hdr
    # one copy of the loss: the kernel bodies live in the header, both sources include it
    csrc = os.path.join(root, "adaptersis_amd", "csrc")
    for f in ("loss.hip", "semi.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "seg_loss_body.h"' in text and not re.search(r"void seg_loss_\w+_kernel", text), f
    assert len(re.findall(r"void seg_loss_\w+_kernel", open(os.path.join(csrc, "seg_loss_body.h")).read())) == 3


def test_partial_stride_needs_no_gpu():
    lib = _lib_semi.lib()
    for C in (1, 2, 8, 16):
        assert lib.asis_semi_partial_stride(C) == C * 3 + 3


def test_argument_errors_before_any_launch():
    lib, last_error = _lib_semi.lib(), _lib.lib().asis_last_error
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(logits=p, target=p, B=1, h=2, w=2, H=2, W=2, C=2, g=255, n_region=1, mode=0, n_ce=0, partial=p, loss=p, coef=p, valid=p,
             dz=p):
        return lib.asis_semi_loss(None, logits, target, None, B, h, w, H, W, C, g, n_region, mode, 1.0, n_ce, 1.0, partial, None, loss,
                                  coef, valid, dz)

    for kw, word in ((dict(logits=None), b"null"), (dict(target=None), b"null"), (dict(partial=None), b"null"), (dict(loss=None), b"null"),
                     (dict(coef=None), b"null"), (dict(valid=None), b"null"), (dict(dz=None), b"null"), (dict(B=0), b"non-positive"),
                     (dict(H=-1), b"non-positive"), (dict(g=0), b"ignore_index=0"), (dict(g=1), b"ignore_index=1"),
                     (dict(C=17), b"C=17"), (dict(C=0, g=-1), b"C=0"), (dict(B=129), b"B*C=258"), (dict(B=257, C=1), b"B*C=257"),
                     (dict(n_region=3), b"n_region"), (dict(n_ce=3), b"n_ce"), (dict(mode=5), b"mode"),
                     (dict(mode=4), b"needs a CE term")):
        assert call(**kw) == _lib.ASIS_EINVAL, kw
        assert word in last_error() and b"asis_semi_loss" in last_error(), (kw, last_error())
    with pytest.raises(ValueError):
        _lib.check(call(g=1), "asis_semi_loss")


def test_op_has_no_cpu_fallback_and_checks_its_arguments():
    lg, tg = torch.zeros(1, 2, 2, 3), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(_lib.AsisError):
        ops.seg_loss_ignore(lg, tg, 255, 1)


# ---- MixSampler with groups ----------------------------------------------------------------------------------------------------------
def test_mix_groups_none_and_one_group_are_the_ungrouped_tables():
    from adaptersis_amd.tools.mix import MixSampler
    for kind in ("cutmix", "classmix"):
        m = MixSampler(kind, 0.7, 5, 4)
        for B in (1, 2, 5):
            for step in range(4):
                a, b, c = m.draw(B, 20, 30, step, 1), m.draw(B, 20, 30, step, 1, groups=None), m.draw(B, 20, 30, step, 1, groups=[3] * B)
                for k in a:
                    assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]) and a[k].dtype == c[k].dtype, (kind, B, step, k)


@pytest.mark.parametrize("groups", [[0, 1, 0, 0], [1, 1, 0, 0, 1, 0, 1], [2, 0, 1], [0, 0, 1, 1, 1, 1, 1, 1], [True, False, True, True]])
def test_mix_groups_keep_donors_inside_their_group(groups):
    from adaptersis_amd.tools.mix import MixSampler
    B, g = len(groups), np.asarray(groups).astype(np.int64)
    m = MixSampler("classmix", 1.0, 11, 3)
    seen = set()
    for step in range(40):
        t = m.draw(B, 16, 16, step, 2, groups=groups)
        donor, kind = t["donor"].numpy(), t["kind"].numpy()
        assert t["donor"].dtype == torch.int32 and sorted(donor.tolist()) == list(range(B))          # a permutation
        for b in range(B):
            assert g[donor[b]] == g[b]
            if int((g == g[b]).sum()) == 1:      # a group of one: not mixed, its own donor
                assert donor[b] == b and kind[b] == 0
            else:                                # nobody else is their own donor; p = 1 mixes everyone
                assert donor[b] != b and kind[b] == 2
        for gid in np.unique(g):                 # a cyclic shift over the group's members
            mem = np.nonzero(g == gid)[0]
            shift = {(int(np.nonzero(mem == donor[b])[0][0]) - i) % len(mem) for i, b in enumerate(mem)}
            assert len(shift) == 1
        seen.add(tuple(donor.tolist()))
        # a function of (seed, rank, step) alone
        u = MixSampler("classmix", 1.0, 11, 3).draw(B, 16, 16, step, 2, groups=list(groups))
        assert all(torch.equal(t[k], u[k]) for k in t)
    if max(int((g == gid).sum()) for gid in np.unique(g)) > 2:
        assert len(seen) > 1
    with pytest.raises(ValueError, match="groups has"):
        m.draw(B, 16, 16, 0, 0, groups=list(groups) + [0])
    other = m.draw(B, 16, 16, 3, 3, groups=groups)
    assert not all(torch.equal(other[k], m.draw(B, 16, 16, 3, 2, groups=groups)[k]) for k in other)      # every rank its own


# ---- the unlabelled frames -----------------------------------------------------------------------------------------------------------
def _png(path, arr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def test_unlabelled_frames(tmp_path):
    from adaptersis_amd.tools import dataset as D
    S, root = 24, str(tmp_path / "video")
    rng = np.random.default_rng(0)
    names = ["seq_2/frame001.png", "seq_1/frame002.png", "seq_1/frame000.png", "seq_1/deep/frame001.jpg", "frame9.png"]
    for n in names:                                   # written out of order, at several depths and sizes
        hw = (S, S) if n == "frame9.png" else (30, 40)
        _png(os.path.join(root, n), rng.integers(0, 256, hw + (3,), dtype=np.uint8))
    _png(os.path.join(root, "seq_1", "notes.bmp"), np.zeros((4, 4, 3), np.uint8))        # not a frame
    open(os.path.join(root, "seq_1", "readme.txt"), "w").write("x")
    ds = D.UnlabelledFrames(root, S)
    assert [os.path.relpath(f, root) for f in ds.files] == sorted(names) and len(ds) == 5
    for i, f in enumerate(ds.files):
        img, mask, idx = ds[i]
        want = Image.open(f).convert("RGB")
        if want.size != (S, S):
            want = want.resize((S, S), resample=Image.BILINEAR)
        assert idx == i and img.dtype == torch.uint8 and tuple(img.shape) == (S, S, 3) and torch.equal(img, torch.from_numpy(np.array(want)))
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == (S, S) and bool((mask == 255).all())
    frames, masks, idx = D.collate_u8([ds[0], ds[3]])
    assert tuple(frames.shape) == (2, S, S, 3) and tuple(masks.shape) == (2, S, S) and idx.tolist() == [0, 3]
    syn, again = D.UnlabelledFrames("synthetic", S), D.UnlabelledFrames("synthetic", S)
    assert len(syn) == 24 and torch.equal(syn[5][0], again[5][0]) and not torch.equal(syn[5][0], syn[6][0])
    assert syn[0][0].dtype == torch.uint8 and tuple(syn[0][0].shape) == (S, S, 3) and bool((syn[0][1] == 255).all())
    with pytest.raises(ValueError, match="no such directory"):
        D.UnlabelledFrames(str(tmp_path / "absent"), S)
    os.makedirs(tmp_path / "empty")
    with pytest.raises(ValueError, match="no \\*.png"):
        D.UnlabelledFrames(str(tmp_path / "empty"), S)


def test_unlabelled_stream_cycles_and_counts_its_epochs():
    from adaptersis_amd import train as T
    from adaptersis_amd.tools.dataset import UnlabelledFrames
    st = T.UnlabelledStream(UnlabelledFrames("synthetic", 16, n_synth=5), 2)
    got = [st.next() for _ in range(5)]
    assert all(tuple(f.shape) == (2, 16, 16, 3) and f.dtype == torch.uint8 and bool((m == 255).all()) for f, m in got)
    assert st.epoch == 2                              # 5 frames, 2 a step, the short batch dropped: two steps an epoch
    twin = T.UnlabelledStream(UnlabelledFrames("synthetic", 16, n_synth=5), 2)
    assert "unlabelled epoch 2" in twin.load_state_dict({"epoch": 2}) and torch.equal(twin.next()[0], got[4][0])
    few = T.UnlabelledStream(UnlabelledFrames("synthetic", 16, n_synth=3), 4)         # fewer frames than a step asks for: all of them
    assert tuple(few.next()[0].shape) == (3, 16, 16, 3) and tuple(few.next()[0].shape) == (3, 16, 16, 3) and few.epoch == 1


# ---- the flags -----------------------------------------------------------------------------------------------------------------------
def _ns(**kw):
    return argparse.Namespace(arch="vit_large", **kw)


def test_script_refusals(tmp_path):
    from adaptersis_amd import train as T
    from adaptersis_amd import train_mla, train_multi_class
    from adaptersis_amd.backbones.engines import SegEngine
    ok = T.check_semi_args
    assert ok(argparse.Namespace()) is None and ok(_ns(unlabelled_path=None, ignore_index=None)) is None
    assert ok(_ns(unlabelled_path="synthetic", distill_teacher="ema", ema_decay=0.9, unlabelled_per_batch=3, ignore_index=255,
                  distill_labelled_weight=0.0)) is None
    assert ok(_ns(unlabelled_path=str(tmp_path), distill_teacher="ema")) is None and ok(_ns(ignore_index=-1)) is None
    assert "--unlabelled_path needs --distill_teacher" in ok(_ns(unlabelled_path="synthetic"))
    assert "--unlabelled_per_batch needs --unlabelled_path" in ok(_ns(unlabelled_per_batch=2))
    assert "--distill_labelled_weight needs --distill_teacher" in ok(_ns(distill_labelled_weight=0.5))
    assert "--distill_labelled_weight must be" in ok(_ns(distill_labelled_weight=-1.0, distill_teacher="ema"))
    assert "no such directory" in ok(_ns(unlabelled_path=str(tmp_path / "absent"), distill_teacher="ema"))
    assert "at least 1" in ok(_ns(unlabelled_path="synthetic", distill_teacher="ema", unlabelled_per_batch=0))
    hard = ("lovasz", "ce_lovasz", "topk", "dc_and_topk", "focal")
    assert set(hard) | set(SegEngine.IGNORE_LOSSES) == set(SegEngine.LOSSES)
    for loss in hard:
        assert "--ignore_index needs a loss with an ignore label" in ok(_ns(ignore_index=255, loss=loss))
        assert "--unlabelled_path needs a loss with an ignore label" in ok(_ns(unlabelled_path="synthetic", distill_teacher="ema", loss=loss))
        assert "--ignore_index" in ok(_ns(ignore_index=255, loss="dice"), loss)            # the loss a script passes wins
    for loss in SegEngine.IGNORE_LOSSES:
        assert ok(_ns(ignore_index=255, loss=loss)) is None
    # the parsers of the three scripts refuse them as usage errors, and train_seg before any process group is opened
    for mod in (T, train_mla, train_multi_class):
        p = mod.get_args_parser()
        for bad in (["--unlabelled_path", "synthetic"], ["--ignore_index", "255", "--loss", "lovasz"], ["--ignore_index", "255", "--loss", "focal"],
                    ["--unlabelled_per_batch", "4"], ["--distill_labelled_weight", "0.5"]):
            with pytest.raises(SystemExit):
                p.parse_args(bad)
        a = p.parse_args(["--ema_decay", "0.9", "--distill_teacher", "ema", "--unlabelled_path", "synthetic", "--unlabelled_per_batch", "3",
                          "--ignore_index", "255", "--distill_labelled_weight", "0.5"])
        assert T._semi_engine_args(a) == dict(ignore_index=255, distill_labelled_weight=0.5) and a.unlabelled_per_batch == 3
        assert T._semi_engine_args(p.parse_args([])) == {}
    with pytest.raises(ValueError, match="--unlabelled_path needs --distill_teacher"):
        T.train_seg(_ns(unlabelled_path="synthetic"))
    with pytest.raises(ValueError, match="--ignore_index needs a loss"):
        T.train_seg(_ns(ignore_index=255, loss="topk"))
