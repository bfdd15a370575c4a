"""CPU: the host side of the percentile Hausdorff distance — ``surface_ranks`` against exact fractions, ``percentile_from_order``
bit for bit against the same formula on the sorted list and within 1e-9 relative of ``numpy.percentile`` (numpy forms the rank in
floating point: an index error of at most n 2^-52 times gap / value, below 1e-9 for n <= 1e5), ``SurfaceMeter`` with and without
percentiles, the ``--hd_percentile`` flag, and the argument errors of ``asis_surface_quantiles`` and of ``ops`` that need no GPU."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

from adaptersis_amd import _lib, ops
from adaptersis_amd.segloss import surface as S
from adaptersis_amd.segloss.surface import SurfaceMeter, metrics_from_stats, percentile_from_order, surface_ranks

QS = (0, 1, 2500, 5000, 9500, 9950, 9999, 10000)


# ---- 1. ranks ---------------------------------------------------------------------------------------------------------------------
def test_surface_ranks_against_exact_fractions():
    for n in range(1, 61):
        for q in QS:
            pos = Fraction(n - 1) * Fraction(q, 10000)              # the exact fractional rank
            lo, hi, rem = surface_ranks(n, q)
            assert all(type(v) is int for v in (lo, hi, rem))
            assert lo == math.floor(pos) and hi == math.ceil(pos) and Fraction(rem, 10000) == pos - lo
            assert 0 <= lo <= hi <= n - 1 and hi - lo == (rem != 0)
    assert surface_ranks(1, 9500) == (0, 0, 0) and surface_ranks(2, 5000) == (0, 1, 5000)
    r = ((1 << 29) - 1) * 9999                                      # the largest pooled set: the product needs 64 bits
    assert r > 1 << 32 and r % 10000 and surface_ranks(1 << 29, 9999) == (r // 10000, r // 10000 + 1, r % 10000)
    for bad in ((0, 5000), (5, -1), (5, 10001)):
        with pytest.raises(ValueError):
            surface_ranks(*bad)


# ---- 2. the value from two order statistics -----------------------------------------------------------------------------------------
def test_percentile_from_order_against_the_sorted_list_and_numpy():
    rng = np.random.default_rng(7)
    worst = 0.0
    for n in (1, 2, 3, 7, 60, 1000, 100000):
        for top in (1, 4, 300, 1 << 29):
            v = np.sort(rng.integers(0, top + 1, n))
            d = np.sqrt(v.astype(np.float64))                      # correctly rounded, as math.sqrt
            for q in QS:
                lo, hi, rem = surface_ranks(n, q)
                got = percentile_from_order(int(v[lo]), int(v[hi]), rem)
                a = math.sqrt(int(v[lo]))
                assert got == a + (rem / 10000) * (math.sqrt(int(v[hi])) - a)          # the same formula: the same bits
                ref = float(np.percentile(d, q / 100))
                err = abs(got - ref) / ref if ref else abs(got - ref)
                worst = max(worst, err)
                assert err <= 1e-9, (n, top, q, got, ref)
    print(f"max relative difference from numpy.percentile: {worst:.3e}")
    assert percentile_from_order(9, 16, 5000) == 3.5 and percentile_from_order(25, 25, 0) == 5.0


# ---- 3. metrics and aggregation ----------------------------------------------------------------------------------------------------
def _row(inter, n_pred, n_lab, e_pred, e_lab, max_pred, max_lab, hit_pred, hit_lab):
    return [inter, n_pred, n_lab, e_pred, e_lab, max_pred, max_lab, *hit_pred, *hit_lab]


def _frames():
    """Two frames, four classes, two tolerances (the hand-made statistics of test_surface_host.py) and order statistics for the
    percentiles [50, 95]: ord[c, p, set] = (v[lo], v[hi])."""
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
    o0 = np.full((4, 2, 3, 2), -1, dtype=np.int64)
    o0[0] = [[[1, 4], [4, 4], [1, 4]], [[9, 9], [9, 16], [9, 16]]]
    o0[3] = 0
    o1 = np.full((4, 2, 3, 2), -1, dtype=np.int64)
    o1[0] = [[[1, 1], [0, 1], [1, 1]], [[4, 4], [1, 1], [1, 4]]]
    o1[2] = [[[4, 4], [1, 4], [4, 4]], [[16, 25], [4, 9], [9, 16]]]
    return (f0, s0, o0), (f1, s1, o1)


def test_metrics_from_stats_with_percentiles():
    (f0, s0, o0), _ = _frames()
    plain = metrics_from_stats(f0, s0, [0, 2])
    m = metrics_from_stats(f0, s0, [0, 2], o0, [50, 95])
    assert m[1] is None and plain[1] is None
    for c in (0, 2, 3):
        assert {k: v for k, v in m[c].items() if k not in ("hd_pct", "hd_pct_sym")} == plain[c]
        assert sorted(plain[c]) == ["assd", "dice", "hd", "nsd", "unmatched"]
    assert m[2]["hd_pct"] is None and m[2]["hd_pct_sym"] is None
    assert m[3]["hd_pct"] == [0.0, 0.0] and m[3]["hd_pct_sym"] == [0.0, 0.0]
    # class 0: e_pred 30, e_lab 28, pooled 58; rem of (n - 1) q: 29 * 5000 -> 5000, 27 * 5000 -> 5000, 57 * 5000 -> 5000;
    # 29 * 9500 -> 5500, 27 * 9500 -> 6500, 57 * 9500 -> 1500
    assert [surface_ranks(n, q)[2] for q in (5000, 9500) for n in (30, 28, 58)] == [5000, 5000, 5000, 5500, 6500, 1500]
    assert m[0]["hd_pct"] == [1.0 + 0.5 * (2.0 - 1.0), 3.0 + 0.15 * (4.0 - 3.0)]
    assert m[0]["hd_pct_sym"] == [max(1.5, 2.0), max(3.0, 3.0 + 0.65 * (4.0 - 3.0))]
    with pytest.raises(ValueError, match="go together"):
        metrics_from_stats(f0, s0, [0, 2], o0)
    with pytest.raises(ValueError, match="go together"):
        metrics_from_stats(f0, s0, [0, 2], percentiles=[95])
    with pytest.raises(ValueError, match="ord"):
        metrics_from_stats(f0, s0, [0, 2], o0, [95])
    bad = o0.copy()
    bad[0, 1, 2, 1] = -1
    with pytest.raises(ValueError, match="missing"):
        metrics_from_stats(f0, s0, [0, 2], bad, [50, 95])


def test_surface_meter_with_and_without_percentiles():
    (f0, s0, o0), (f1, s1, o1) = _frames()
    tol = [0, 2]
    plain = SurfaceMeter(4, tol)
    plain.update(f0, s0)
    plain.update(f1[None], s1[None])
    r = plain.result()
    # without percentiles: key for key and value for value what the meter gave before the percentiles existed
    assert sorted(r) == ["frames", "mean_assd", "mean_dice", "mean_hd", "mean_nsd", "per_class", "tolerances"]
    pc = r["per_class"]
    assert all(sorted(p) == ["assd", "dice", "frames", "frames_matched", "hd", "nsd", "unmatched"] for p in pc)
    assert pc[1] == {"dice": None, "nsd": None, "hd": None, "assd": None, "frames": 0, "frames_matched": 0, "unmatched": 0}
    assert pc[2] == {"dice": (0.0 + 12 / 24) / 2, "nsd": [(0.0 + 3 / 12) / 2, (0.0 + 6 / 12) / 2], "hd": 5.0, "assd": 18.0 / 12,
                     "frames": 2, "frames_matched": 1, "unmatched": 1}
    assert pc[3] == {"dice": 1.0, "nsd": [1.0, 1.0], "hd": 0.0, "assd": 0.0, "frames": 1, "frames_matched": 1, "unmatched": 0}
    assert pc[0] == {"dice": (180 / 195 + 0.5) / 2, "nsd": [(22 / 58 + 10 / 16) / 2, (45 / 58 + 1.0) / 2], "hd": (4.0 + 2.0) / 2,
                     "assd": (77.75 / 58 + 4.0 / 16) / 2, "frames": 2, "frames_matched": 2, "unmatched": 0}
    assert r["tolerances"] == [0.0, 2.0] and r["frames"] == 2 and r["mean_hd"] == 2.5 and r["mean_assd"] == np.mean([1.5, 0.0])
    assert r["mean_dice"] == np.mean([pc[2]["dice"], 1.0])
    assert r["mean_nsd"] == [np.mean([pc[2]["nsd"][0], 1.0]), np.mean([pc[2]["nsd"][1], 1.0])]

    meter = SurfaceMeter(4, tol, [50, 95])
    meter.update(f0, s0, o0)
    meter.update(f1[None], s1[None], o1[None])
    rp = meter.result()
    assert sorted(rp) == sorted(list(r) + ["percentiles", "mean_hd_pct", "mean_hd_pct_sym"])
    assert {k: rp[k] for k in r if k != "per_class"} == {k: r[k] for k in r if k != "per_class"}
    for p, q in zip(pc, rp["per_class"]):
        assert {k: v for k, v in q.items() if k not in ("hd_pct", "hd_pct_sym")} == p
    assert rp["percentiles"] == [50.0, 95.0]
    qc = rp["per_class"]
    assert qc[1]["hd_pct"] is None and qc[1]["hd_pct_sym"] is None
    assert qc[3]["hd_pct"] == [0.0, 0.0] and qc[3]["hd_pct_sym"] == [0.0, 0.0]
    # class 2: frame 1 only (unmatched in frame 0, which has no value, like hd); e_pred 5, e_lab 7, pooled 12:
    # rem of 4 * 5000, 6 * 5000, 11 * 5000 = 0, 0, 5000; of 4 * 9500, 6 * 9500, 11 * 9500 = 8000, 7000, 4500
    assert qc[2]["hd_pct"] == [2.0 + 0.5 * 0.0, 3.0 + 0.45 * (4.0 - 3.0)]
    assert qc[2]["hd_pct_sym"] == [max(2.0, 1.0), max(4.0 + 0.8 * (5.0 - 4.0), 2.0 + 0.7 * (3.0 - 2.0))]
    # class 0, frame 1: e 8, 8, 16: rem of 7 * 5000 = 5000, 15 * 5000 = 5000; 7 * 9500 = 6500, 15 * 9500 = 2500
    f1_pct = [1.0 + 0.5 * 0.0, 1.0 + 0.25 * (2.0 - 1.0)]
    f1_sym = [max(1.0, 0.0 + 0.5 * 1.0), max(2.0, 1.0)]
    f0_pct, f0_sym = [1.5, 3.0 + 0.15 * 1.0], [2.0, 3.0 + 0.65 * 1.0]
    assert qc[0]["hd_pct"] == [(a + b) / 2 for a, b in zip(f0_pct, f1_pct)]
    assert qc[0]["hd_pct_sym"] == [(a + b) / 2 for a, b in zip(f0_sym, f1_sym)]
    assert rp["mean_hd_pct"] == [float(np.mean([qc[2]["hd_pct"][j], 0.0])) for j in range(2)]
    assert rp["mean_hd_pct_sym"] == [float(np.mean([qc[2]["hd_pct_sym"][j], 0.0])) for j in range(2)]
    empty = SurfaceMeter(1, tol, [95]).result()
    assert empty["mean_hd_pct"] == [None] and empty["mean_hd_pct_sym"] == [None] and empty["per_class"][0]["hd_pct"] is None
    with pytest.raises(ValueError, match="exactly when"):
        meter.update(f0, s0)
    with pytest.raises(ValueError, match="exactly when"):
        plain.update(f0, s0, o0)
    with pytest.raises(ValueError, match="5 percentiles"):
        SurfaceMeter(2, tol, [1, 2, 3, 4, 5])


# ---- 4. the flag -------------------------------------------------------------------------------------------------------------------
def test_hd_percentile_flag(monkeypatch):
    from adaptersis_amd import predict as P
    from adaptersis_amd import score as SC
    base = ["--input", "/nonexistent/frames", "--pred_dir", "/nonexistent/pred"]

    def no_model(*a, **k):
        raise AssertionError("a model was built before the argument error")

    monkeypatch.setattr(P, "build_engine", no_model)
    monkeypatch.setattr(P, "_Frames", no_model)
    parse = P.get_args_parser().parse_args
    with pytest.raises(ValueError, match="--hd_percentile needs --surface"):
        P.predict_seg(parse(base + ["--masks", "/m", "--hd_percentile"]))
    with pytest.raises(ValueError, match="--hd_percentile needs --surface"):
        P.predict_seg(parse(base + ["--masks", "/m", "--hd_percentile", "95"]))
    with pytest.raises(ValueError, match="multiple of 0.01"):
        P.predict_seg(parse(base + ["--masks", "/m", "--surface", "--hd_percentile", "95.001"]))
    with pytest.raises(ValueError, match="0..100"):
        P.predict_seg(parse(base + ["--masks", "/m", "--surface", "--hd_percentile", "101"]))
    with pytest.raises(ValueError, match="5 percentiles"):
        P.predict_seg(parse(base + ["--masks", "/m", "--surface", "--hd_percentile", "1", "2", "3", "4", "5"]))
    assert P.hd_percentiles(parse(base)) is None
    assert P.hd_percentiles(parse(base + ["--masks", "/m", "--surface"])) is None
    assert P.hd_percentiles(parse(base + ["--masks", "/m", "--surface", "--hd_percentile"])) == [95.0]
    assert P.hd_percentiles(parse(base + ["--masks", "/m", "--surface", "1", "--hd_percentile", "95", "99.5"])) == [95.0, 99.5]
    sparse = SC.get_args_parser().parse_args
    with pytest.raises(ValueError, match="--hd_percentile needs --surface"):
        SC.score(sparse(["--pred_dir", "/nonexistent/pred", "--masks", "/m", "--hd_percentile", "95"]))
    assert sparse(["--pred_dir", "/p", "--surface", "--hd_percentile"]).hd_percentile == []
    # the line of the run: the first percentile, and nothing new without the flag
    s = {"tolerances": [1.0], "mean_nsd": [0.5], "mean_dice": 0.9, "mean_hd": 7.0, "mean_assd": 1.25, "per_class": [{"unmatched": 2}]}
    line = P.surface_line(s)
    assert "HD" not in line.replace("Hausdorff", "") and "Hausdorff 7.0  mean surface distance 1.25" in line
    s.update(percentiles=[95.0, 99.5], mean_hd_pct=[3.5, 6.0], mean_hd_pct_sym=[4.0, 6.5])
    assert "Hausdorff 7.0  HD95 3.5 (directed maximum 4.0)  mean surface distance" in P.surface_line(s)


# ---- 5. argument errors that need no GPU -------------------------------------------------------------------------------------------
def test_scratch_bytes_need_no_gpu():
    lib = _lib.lib()
    last = 0
    for B, nc, P in ((1, 1, 1), (1, 8, 1), (12, 8, 1), (12, 8, 4), (12, 16, 4)):
        n = lib.asis_surface_quantile_scratch_bytes(B, nc, P)
        # a 256-bin histogram per (frame, class, side) and per (frame, class, percentile, set), and the state of every select
        assert n >= 4 * 256 * B * nc * (2 + 3 * P) and n > last and n % 16 == 0
        assert ops.surface_quantile_scratch_bytes(B, nc, P) == n
        last = n
    assert last < 4 << 20
    for bad in ((0, 1, 1), (1, 0, 1), (1, 17, 1), (1, 1, 0), (1, 1, 5), (32768, 1, 1)):
        assert lib.asis_surface_quantile_scratch_bytes(*bad) == -1 and b"asis_surface_quantile_scratch_bytes" in lib.asis_last_error()
        with pytest.raises(ValueError):
            ops.surface_quantile_scratch_bytes(*bad)


def test_entry_argument_errors_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    a += -a % 16                                      # 16-byte aligned, inside the buffer

    def call(edges=a, g=a, ints=a, B=1, H=8, W=8, C=2, c0=0, nc=None, T=1, q=(9500,), P=None, dq=a, scratch=a, ord_=a):
        qa = (ctypes.c_int32 * 8)(*q) if q is not None else None
        return lib.asis_surface_quantiles(None, edges, g, ints, B, H, W, C, c0, C if nc is None else nc, T, qa,
                                          len(q) if P is None else P, dq, scratch, ord_)

    cases = [(dict(edges=None), b"null pointer"), (dict(g=None), b"null pointer"), (dict(ints=None), b"null pointer"),
             (dict(q=None, P=1), b"null pointer"), (dict(dq=None), b"null pointer"), (dict(scratch=None), b"null pointer"),
             (dict(ord_=None), b"null pointer"), (dict(P=0), b"P=0 percentiles"), (dict(P=5), b"P=5 percentiles"),
             (dict(q=(-1,)), b"q=-1 must be in 0..10000"), (dict(q=(9500, 10001)), b"q=10001 must be in 0..10000"),
             (dict(C=17), b"C=17 must be in 1..16"), (dict(C=0), b"C=0"), (dict(c0=1, nc=2), b"class range c0=1 nc=2"),
             (dict(B=0), b"non-positive size B=0"), (dict(H=16385), b"H=16385"), (dict(W=16385), b"W=16385"), (dict(T=9), b"T=9"),
             (dict(ints=a + 4), b"misaligned"), (dict(ord_=a + 4), b"misaligned"), (dict(scratch=a + 8), b"misaligned"),
             (dict(dq=a + 2), b"misaligned"), (dict(g=a + 1), b"misaligned")]
    for kw, text in cases:
        rc = call(**kw)
        assert rc == _lib.ASIS_EINVAL and text in lib.asis_last_error(), (kw, lib.asis_last_error())
    with pytest.raises(ValueError):
        _lib.check(call(P=5), "asis_surface_quantiles")


def test_op_argument_errors():
    import torch
    assert ops.surface_percentiles([0, 50, 95, 100]) == [0, 5000, 9500, 10000]
    assert ops.surface_percentiles([99.5]) == [9950] and ops.surface_percentiles([0.01, 99.99, 33.33]) == [1, 9999, 3333]
    assert ops.surface_percentiles([95 + 5e-10]) == [9500]                    # a multiple of 0.01 to within 1e-9
    for bad, text in (([], "0 percentiles"), ([1, 2, 3, 4, 5], "5 percentiles"), ([95.001], "multiple of 0.01"),
                      ([-1], "0..100"), ([100.01], "0..100"), ([float("nan")], "0..100"), ([95 + 1e-6], "multiple of 0.01")):
        with pytest.raises(ValueError, match=text):
            ops.surface_percentiles(bad)
        with pytest.raises(ValueError, match=text):                           # before the device is looked at
            ops.surface_stats(torch.zeros((1, 4, 4), dtype=torch.uint8), torch.zeros((1, 4, 4), dtype=torch.uint8), 2, [1],
                              percentiles=bad)
    z = torch.zeros((1, 4, 4), dtype=torch.uint8)
    with pytest.raises(_lib.AsisError, match="no CPU fallback"):
        ops.surface_stats(z, z, 2, [1], percentiles=[95])
    assert S.percentile_q(99.5) == 9950 and S.QSCALE == 10000
    # the plan: unchanged without percentiles, and with them the int32 distances of both sides count against the budget
    for B, H, W, C in [(12, 1080, 1920, 8), (12, 1080, 1920, 16), (3, 16384, 16384, 16), (1, 1, 1, 1), (5, 540, 960, 2)]:
        assert ops.surface_plan(B, H, W, C, percentiles=False) == ops.surface_plan(B, H, W, C)
        nb, nc = ops.surface_plan(B, H, W, C, percentiles=True)
        assert 1 <= nb <= B and 1 <= nc <= C
        assert nb * (nc * 2 * H * W * 2 + 2 * H * W * 4) <= ops.SURFACE_WORKSPACE_BYTES or (nb == 1 and nc == 1)
    assert ops.surface_plan(12, 1080, 1920, 8) == (8, 8) and ops.surface_plan(12, 1080, 1920, 8, percentiles=True) == (6, 8)
