"""CPU: sliding-window prediction of ``adaptersis_amd.predict`` — the tile plan (``plan_tiles``), the new arguments, argument errors
raised before any file is read or any model is built, and the argument errors of ``asis_predict_mask_tiles`` that need no GPU."""
import ctypes

import pytest

from adaptersis_amd import _lib
from adaptersis_amd import predict as P

GRIDS = [(96, 48, 32), (80, 48, 32), (112, 48, 16), (48, 48, 48), (1176, 588, 392)]
# written out by hand from n = max(L - S + T - 1, 0) // T + 1, o_i = min(i T, L - S)
ORIGINS = {(96, 48, 32): [0, 32, 48], (80, 48, 32): [0, 32], (112, 48, 16): [0, 16, 32, 48, 64], (48, 48, 48): [0],
           (1176, 588, 392): [0, 392, 588]}


def _formula(L, S, T):
    n = max(L - S + T - 1, 0) // T + 1
    return [min(i * T, L - S) for i in range(n)]


@pytest.mark.parametrize("L,S,T", GRIDS)
def test_plan_tiles_origins_follow_the_formula(L, S, T):
    org = _formula(L, S, T)
    assert org == ORIGINS[(L, S, T)] and P.slide_origins(L, S, T) == org
    tiles = P.plan_tiles(L, S, T, False, False)
    assert tiles == [(oy, ox, S, S, False) for oy in org for ox in org]          # row-major
    assert org[0] == 0 and org[-1] + S == L and all(b - a <= S for a, b in zip(org, org[1:]))      # the windows cover [0, L)


def test_plan_tiles_order_flip_and_context():
    win = [(0, 0), (0, 32), (32, 0), (32, 32)]
    assert P.plan_tiles(80, 48, 32, False, False) == [(oy, ox, 48, 48, False) for oy, ox in win]
    assert P.plan_tiles(80, 48, 32, True, False) == [(oy, ox, 48, 48, False) for oy, ox in win] + [(0, 0, 80, 80, False)]
    flipped = P.plan_tiles(80, 48, 32, True, True)
    assert len(flipped) == 10
    assert flipped[0::2] == P.plan_tiles(80, 48, 32, True, False)               # every tile is followed by its mirrored twin
    assert flipped[1::2] == [t[:4] + (True,) for t in flipped[0::2]]
    assert flipped[-2:] == [(0, 0, 80, 80, False), (0, 0, 80, 80, True)]        # the context tile comes last
    assert P.plan_tiles(48, 48, 48, True, True) == [(0, 0, 48, 48, False), (0, 0, 48, 48, True)] * 2
    assert P.plan_tiles(48, 48, 1, False, False) == [(0, 0, 48, 48, False)]


def test_plan_tiles_cap():
    assert len(P.plan_tiles(112, 48, 16, True, False)) == 26
    assert len(P.plan_tiles(84, 48, 12, False, True)) == 32                     # 4 x 4 windows mirrored: 32 tiles are allowed
    assert len(P.plan_tiles(96, 48, 32, True, True)) == 20
    for args, count in (((112, 48, 16, False, True), 50), ((112, 48, 16, True, True), 52), ((84, 48, 12, True, True), 34),
                        ((96, 48, 8, False, False), 49), ((588 * 4, 588, 392, False, False), 36)):
        with pytest.raises(ValueError, match=f"{count} tiles"):
            P.plan_tiles(*args)


@pytest.mark.parametrize("args,name", [
    ((40, 48, 32, False, False), "--slide_size"), ((0, 48, 32, False, False), "--slide_size"),
    ((96, 48, 0, False, False), "--slide_stride"), ((96, 48, 49, False, False), "--slide_stride"),
    ((96, 48, -3, True, True), "--slide_stride"), ((96, 0, 1, False, False), "--imsize"), ((96, -48, 1, False, False), "--imsize"),
    ((96.0, 48, 32, False, False), "--slide_size"), ((96, 48, 32.5, False, False), "--slide_stride"),
    ((96, True, 1, False, False), "--imsize")])
def test_plan_tiles_names_the_bad_argument(args, name):
    with pytest.raises(ValueError, match=name):
        P.plan_tiles(*args)


def _args(tmp_path, *extra):
    return P.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", "224", "--output_dir", str(tmp_path / "nowhere"),
                                           "--input", str(tmp_path), "--pred_dir", str(tmp_path / "pred"), *extra])


def test_parser_accepts_the_new_flags(tmp_path):
    a = _args(tmp_path)
    assert a.slide_size is None and a.slide_stride is None and a.slide_blend is None and a.slide_context is False
    assert P.tiles_of(a) is None                                                  # no flag: the paths that were there
    plan = P.tiles_of(_args(tmp_path, "--slide_size", "336"))
    assert plan == {"size": 336, "stride": 149, "blend": "ramp", "context": False, "flip": False, "ramp": 75,
                    "tiles": P.plan_tiles(336, 224, 149, False, False)}
    assert [t[0] for t in plan["tiles"][::2]] == [0, 112] and len(plan["tiles"]) == 4
    plan = P.tiles_of(_args(tmp_path, "--slide_size", "336", "--slide_stride", "112", "--slide_blend", "uniform", "--slide_context",
                            "--tta_flip", "--confidence"))
    assert plan["tiles"] == P.plan_tiles(336, 224, 112, True, True) and len(plan["tiles"]) == 10
    assert (plan["stride"], plan["blend"], plan["context"], plan["flip"], plan["ramp"]) == (112, "uniform", True, True, 112)
    assert P.tiles_of(_args(tmp_path, "--slide_size", "224", "--slide_stride", "224"))["ramp"] == 1      # max(S - T, 1)
    with pytest.raises(SystemExit):
        _args(tmp_path, "--slide_size", "336", "--slide_blend", "gauss")


@pytest.mark.parametrize("extra,msg", [
    (("--slide_size", "336", "--tta_sizes", "224"), "--tta_sizes"),
    (("--slide_size", "336", "--tta_sizes", "224", "448", "--tta_flip"), "--tta_sizes"),
    (("--slide_size", "200"), "--slide_size"),
    (("--slide_size", "336", "--slide_stride", "0"), "--slide_stride"),
    (("--slide_size", "336", "--slide_stride", "225"), "--slide_stride"),
    (("--slide_size", "2240", "--slide_stride", "224"), "100 tiles"),
    (("--slide_size", "672", "--slide_stride", "112", "--tta_flip"), "50 tiles"),
    (("--slide_stride", "112"), "--slide_stride needs --slide_size"),
    (("--slide_context",), "--slide_context needs --slide_size"),
    (("--slide_blend", "uniform"), "--slide_blend needs --slide_size")])
def test_argument_errors_come_before_files_and_model(tmp_path, extra, msg):
    """--input is an empty directory and there is no checkpoint: the error must be the one of the flags."""
    with pytest.raises(ValueError, match=msg):
        P.predict_seg(_args(tmp_path, *extra))
    assert not (tmp_path / "pred").exists()


def test_valid_slide_flags_reach_the_file_list(tmp_path):
    with pytest.raises(ValueError, match="no frames"):                            # valid tiles: the empty input is what is wrong
        P.predict_seg(_args(tmp_path, "--slide_size", "336", "--slide_stride", "112", "--slide_context", "--tta_flip", "--confidence"))


GRID4 = [(0, 0, 5, 5), (0, 3, 5, 5), (3, 0, 5, 5), (3, 3, 5, 5)]


def _call(K=4, null_view=None, B=1, C=3, H=9, W=9, Lh=8, Lw=8, hs=(4, 5), ws=(4, 5), rects=GRID4, blend=1, ramp=2.0, frames=False,
          overlay=False, target=False, counts=None):
    """asis_predict_mask_tiles with made-up non-null addresses: every case here is refused before anything is launched."""
    lib = _lib.lib()
    a = 4096
    n = max(K, 1)
    ptrs = (ctypes.c_void_p * n)(*[None if k == null_view else a for k in range(n)])
    h = (ctypes.c_int * n)(*[hs[k % len(hs)] for k in range(n)])
    w = (ctypes.c_int * n)(*[ws[k % len(ws)] for k in range(n)])
    r = (ctypes.c_int * (4 * n))(*[v for k in range(n) for v in rects[k % len(rects)]])
    f = (ctypes.c_int * n)(*[k & 1 for k in range(n)])
    return lib.asis_predict_mask_tiles(None, ptrs, h, w, r, f, K, Lh, Lw, blend, ramp, B, C, H, W, a, a, None, a if frames else None,
                                       a if frames else None, a if frames else None, a if overlay else None, a if target else None,
                                       a if target else None, counts)


@pytest.mark.parametrize("kw,msg", [
    (dict(K=0), "K=0"), (dict(K=33), "K=33"), (dict(null_view=1), r"logits\[1\]"), (dict(C=17), "C=17"), (dict(C=0), "C=0"),
    (dict(B=65536), "65535"), (dict(H=16385), "16384"), (dict(W=0), "non-positive"), (dict(Lh=0), "non-positive"),
    (dict(Lw=16385, rects=[(0, 0, 8, 16385)], K=1), "16384"), (dict(hs=(4, 16385)), "hs=16385"), (dict(ws=(0, 4)), "ws=0"),
    (dict(blend=2), "blend=2"), (dict(ramp=0.0), "ramp=0"), (dict(ramp=0.5), "ramp=0.5"), (dict(ramp=float("nan")), "ramp="),
    (dict(rects=[(0, 0, 5, 5), (0, 3, 5, 5), (3, 0, 5, 5), (4, 3, 5, 5)]), "tile 3"),
    (dict(rects=[(0, 0, 5, 5), (0, -1, 5, 5)], K=2), "tile 1"), (dict(rects=[(0, 0, 0, 8)], K=1), "tile 0"),
    (dict(rects=[(0, 0, 8, 9)], K=1), "tile 0"), (dict(rects=[(0, 0, 2 ** 31 - 1, 8), (2, 0, 2 ** 31 - 1, 8)], K=2), "tile 0"),
    (dict(rects=[(0, 0, 3, 8), (4, 0, 4, 8)], K=2), "rows do not cover"), (dict(rects=[(0, 0, 8, 4), (0, 4, 8, 3)], K=2), "columns do not cover"),
    (dict(rects=[(1, 0, 7, 8)], K=1), "rows do not cover"),
    (dict(overlay=True), "overlay requested without frames"), (dict(counts=4096), "counts requested without"),
    (dict(counts=4100, target=True), "8-byte aligned")])
def test_abi_argument_errors_without_a_gpu(kw, msg):
    rc = _call(**kw)
    assert rc == _lib.ASIS_EINVAL
    with pytest.raises(ValueError, match=msg):
        _lib.check(rc, "asis_predict_mask_tiles")
