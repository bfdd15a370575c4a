"""CPU: the boundary-metric definitions — the scipy oracle on the worked case, ``metrics_from_stats`` / ``SurfaceMeter`` on hand-made
statistics, the argument errors of ``asis_surface_stats`` that need no GPU, and ``predict``'s ``--surface`` argument."""
import ctypes

import numpy as np
import pytest

from adaptersis_amd import _lib
from adaptersis_amd.segloss.surface import SurfaceMeter, metrics_from_stats

from . import surface_ref as R


# ---- 1. the oracle on the worked case ------------------------------------------------------------------------------------------
def test_oracle_reproduces_the_worked_case():
    P = np.zeros((12, 16), dtype=bool)
    G = np.zeros((12, 16), dtype=bool)
    P[2:8, 3:9] = True
    G[3:10, 5:12] = True
    ints, sums, dP, dG = R.frame_class_stats(P, G, [0, 1, 2, 3])
    assert ints.tolist() == [20, 36, 49, 20, 24, 9, 13, 2, 9, 18, 20, 2, 8, 15, 22]
    assert sums.tolist() == [29.650281539872886, 46.83232403787835]
    assert dP.dtype == np.int64 and dP[0, 0] == 2 * 2 + 3 * 3 and dG[11, 15] == 2 * 2 + 4 * 4
    # through the label maps: class 1 = the squares, class 0 the rest, a value >= C is no class
    pred = np.where(P, 1, 0).astype(np.uint8)[None]
    tgt = np.where(G, 1, 0).astype(np.uint8)[None]
    tgt[0, 0, 0] = 7
    bi, bs = R.stats(pred, tgt, 2, [0, 1, 2, 3])
    assert bi[0, 1].tolist() == ints.tolist() and bs[0, 1].tolist() == sums.tolist()
    assert bi[0, 0, 1] == 12 * 16 - 36 and bi[0, 0, 2] == 12 * 16 - 49 - 1


def test_edge_pixels_definition():
    rng = np.random.default_rng(3)
    M = rng.random((9, 13)) < 0.6
    pad = np.pad(M, 1)
    inner = pad[:-2, 1:-1] & pad[2:, 1:-1] & pad[1:-1, :-2] & pad[1:-1, 2:]        # all four neighbours in the mask
    assert np.array_equal(R.edges_of(M), M & ~inner)
    full = np.ones((5, 7), dtype=bool)
    e = R.edges_of(full)
    assert e.sum() == 2 * 5 + 2 * 7 - 4 and not e[1:-1, 1:-1].any()


# ---- 2. metrics and aggregation on hand-made statistics ------------------------------------------------------------------------
def _row(inter, n_pred, n_lab, e_pred, e_lab, max_pred, max_lab, hit_pred, hit_lab):
    return [inter, n_pred, n_lab, e_pred, e_lab, max_pred, max_lab, *hit_pred, *hit_lab]


def test_metrics_from_stats_cases():
    tol = [0, 2]
    ints = np.array([_row(90, 100, 95, 30, 28, 9, 16, (10, 25), (12, 20)),     # class 0: on both sides
                     _row(0, 0, 0, 0, 0, 0, 0, (0, 0), (0, 0)),                # class 1: absent on both sides
                     _row(0, 40, 0, 12, 0, 0, 0, (0, 0), (0, 0)),              # class 2: predicted only
                     _row(0, 0, 17, 0, 9, 0, 0, (0, 0), (0, 0)),               # class 3: labelled only
                     _row(50, 50, 50, 20, 20, 0, 0, (20, 20), (20, 20))],      # class 4: identical masks
                    dtype=np.int64)
    sums = np.array([[40.5, 37.25], [0, 0], [0, 0], [0, 0], [0, 0]], dtype=np.float64)
    m = metrics_from_stats(ints, sums, tol)
    assert m[1] is None
    assert m[0] == {"dice": 2 * 90 / 195, "nsd": [22 / 58, 45 / 58], "hd": 4.0, "assd": (40.5 + 37.25) / 58, "unmatched": False}
    for c in (2, 3):
        assert m[c] == {"dice": 0.0, "nsd": [0.0, 0.0], "hd": None, "assd": None, "unmatched": True}
    assert m[4] == {"dice": 1.0, "nsd": [1.0, 1.0], "hd": 0.0, "assd": 0.0, "unmatched": False}
    with pytest.raises(ValueError, match="tolerances"):
        metrics_from_stats(ints, sums, [0, 1, 2])


def test_surface_meter_aggregation():
    tol = [0, 2]
    f0 = np.array([_row(90, 100, 95, 30, 28, 9, 16, (10, 25), (12, 20)),
                   _row(0, 0, 0, 0, 0, 0, 0, (0, 0), (0, 0)),
                   _row(0, 40, 0, 12, 0, 0, 0, (0, 0), (0, 0)),
                   _row(50, 50, 50, 20, 20, 0, 0, (20, 20), (20, 20))], dtype=np.int64)
    s0 = np.array([[40.5, 37.25], [0, 0], [0, 0], [0, 0]], dtype=np.float64)
    f1 = np.array([_row(10, 20, 20, 8, 8, 4, 1, (4, 8), (6, 8)),
                   _row(0, 0, 0, 0, 0, 0, 0, (0, 0), (0, 0)),
                   _row(6, 10, 14, 5, 7, 25, 9, (1, 2), (2, 4)),
                   _row(0, 0, 0, 0, 0, 0, 0, (0, 0), (0, 0))], dtype=np.int64)
    s1 = np.array([[3.0, 1.0], [0, 0], [12.0, 6.0], [0, 0]], dtype=np.float64)
    meter = SurfaceMeter(4, tol)
    meter.update(f0, s0)                                   # one frame's rows
    meter.update(f1[None], s1[None])                       # a batch of one
    r = meter.result()
    assert r["tolerances"] == [0.0, 2.0] and r["frames"] == 2
    pc = r["per_class"]
    assert pc[1] == {"dice": None, "nsd": None, "hd": None, "assd": None, "frames": 0, "frames_matched": 0, "unmatched": 0}
    # class 2: unmatched in frame 0 (dice 0, nsd 0), matched in frame 1
    assert pc[2]["frames"] == 2 and pc[2]["frames_matched"] == 1 and pc[2]["unmatched"] == 1
    assert pc[2]["dice"] == (0.0 + 12 / 24) / 2 and pc[2]["nsd"] == [(0.0 + 3 / 12) / 2, (0.0 + 6 / 12) / 2]
    assert pc[2]["hd"] == 5.0 and pc[2]["assd"] == 18.0 / 12
    assert pc[3] == {"dice": 1.0, "nsd": [1.0, 1.0], "hd": 0.0, "assd": 0.0, "frames": 1, "frames_matched": 1, "unmatched": 0}
    assert pc[0]["frames"] == 2 and pc[0]["dice"] == (180 / 195 + 0.5) / 2
    # headline means: classes 1.. that have a value; the background (class 0) is left out
    assert r["mean_dice"] == np.mean([pc[2]["dice"], 1.0])
    assert r["mean_nsd"] == [np.mean([pc[2]["nsd"][0], 1.0]), np.mean([pc[2]["nsd"][1], 1.0])]
    assert r["mean_hd"] == 2.5 and r["mean_assd"] == np.mean([1.5, 0.0])
    empty = SurfaceMeter(1, tol).result()
    assert empty["mean_dice"] is None and empty["mean_nsd"] == [None, None] and empty["mean_hd"] is None


# ---- 3. argument errors that need no GPU ---------------------------------------------------------------------------------------
def _call(lib, pred=1 << 12, B=1, H=8, W=8, C=2, c0=0, nc=None, T=1, thr=(1,)):
    """Non-null fake addresses: every check is made before anything is launched or dereferenced."""
    a = 1 << 12
    t = (ctypes.c_int32 * 8)(*thr)
    return lib.asis_surface_stats(None, pred, a, a, a, B, H, W, C, c0, C if nc is None else nc, t, T, a, a, a, a, a, None, 0)


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.lib()
    cases = [(dict(pred=None), b"null pointer"), (dict(C=17), b"C=17 must be in 1..16"), (dict(H=16385), b"H=16385"),
             (dict(W=16385), b"W=16385"), (dict(T=9), b"T=9 tolerances"), (dict(thr=(-1,)), b"negative"),
             (dict(c0=1, nc=2), b"class range c0=1 nc=2"), (dict(B=0), b"non-positive size B=0")]
    for kw, text in cases:
        rc = _call(lib, **kw)
        assert rc == -1 and text in lib.asis_last_error(), (kw, lib.asis_last_error())
        with pytest.raises(ValueError):
            _lib.check(rc, "asis_surface_stats")


def test_op_argument_errors():
    import torch
    from adaptersis_amd import ops
    z = torch.zeros((1, 4, 4), dtype=torch.uint8)
    with pytest.raises(_lib.AsisError, match="no CPU fallback"):
        ops.surface_stats(z, z, 2, [1])
    with pytest.raises(ValueError, match="9 tolerances"):
        ops.surface_thresholds(range(9))
    with pytest.raises(ValueError, match="-1.0"):
        ops.surface_thresholds([1, -1])
    with pytest.raises(ValueError, match="nan"):
        ops.surface_thresholds([float("nan")])
    assert ops.surface_thresholds([0, 1, 1.5, 2.9, 5]) == [0, 1, 2, 8, 25]
    # chunking: the vertical-distance maps of one call stay under the budget whenever one class of one frame fits
    for B, H, W, C in [(12, 1080, 1920, 8), (12, 1080, 1920, 16), (3, 16384, 16384, 16), (1, 1, 1, 1), (5, 540, 960, 2)]:
        nb, nc = ops.surface_plan(B, H, W, C)
        assert 1 <= nb <= B and 1 <= nc <= C
        assert nb * nc * 2 * H * W * 2 <= ops.SURFACE_WORKSPACE_BYTES or (nb == 1 and nc == 1)
    assert ops.surface_plan(12, 1080, 1920, 8) == (8, 8)


# ---- 4. predict's argument ------------------------------------------------------------------------------------------------------
def test_predict_surface_argument(monkeypatch):
    from adaptersis_amd import predict as P
    base = ["--input", "/nonexistent/frames", "--pred_dir", "/nonexistent/pred"]

    def no_model(*a, **k):
        raise AssertionError("a model was built before the argument error")

    monkeypatch.setattr(P, "build_engine", no_model)
    monkeypatch.setattr(P, "_Frames", no_model)
    with pytest.raises(ValueError, match="--surface needs --masks"):
        P.predict_seg(P.get_args_parser().parse_args(base + ["--surface"]))
    with pytest.raises(ValueError, match="--surface needs --masks"):
        P.predict_seg(P.get_args_parser().parse_args(base + ["--surface", "1", "3"]))
    with pytest.raises(ValueError, match="tolerance -2.0"):
        P.predict_seg(P.get_args_parser().parse_args(base + ["--masks", "/nonexistent/m", "--surface", "-2"]))
    assert P.surface_tolerances(P.get_args_parser().parse_args(base)) is None
    assert P.surface_tolerances(P.get_args_parser().parse_args(base + ["--masks", "/m", "--surface"])) == [1.0, 2.0, 5.0]
    assert P.surface_tolerances(P.get_args_parser().parse_args(base + ["--masks", "--surface", "1", "3.5"])) == [1.0, 3.5]
    assert P.DEFAULT_TOLERANCES == (1.0, 2.0, 5.0)
