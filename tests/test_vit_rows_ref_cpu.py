"""No GPU: the float64 references of tests/vit_rows_ref.py against float64 autograd of the torch operations, every entry of
its case tables against the dispatch rules of the host code (the branch an entry claims is the branch it reaches), and the
input rules the bounds of tests/test_gpu_vit_rows.py rest on."""
import math

import torch
import torch.nn.functional as F

from adaptersis_amd import _lib
from tests import vit_rows_ref as R
from tests.bound_helpers import DT, _gen

F64 = torch.float64
MAX16 = {torch.float16: 65504.0, torch.bfloat16: float(torch.finfo(torch.bfloat16).max)}


def _close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale, float((a - b).abs().max())


def test_layernorm_reference_is_autograd():
    gen = _gen(1, 2)
    for rows, D in ((1, 4), (5, 260), (33, 1028)):
        x = (torch.randn(rows, D, generator=gen, dtype=F64) + 3).requires_grad_()
        w, b = (torch.randn(D, generator=gen, dtype=F64) for _ in range(2))
        w.requires_grad_(), b.requires_grad_()
        dy, res = torch.randn(rows, D, generator=gen, dtype=F64), torch.randn(rows, D, generator=gen, dtype=F64)
        y = F.layer_norm(x, (D,), w, b, R.EPS)
        y.backward(dy)
        y_ref, mean, rstd = R.layernorm(x.detach(), w.detach(), b.detach())
        _close(y_ref, y.detach())
        _close(mean, x.detach().mean(-1))
        _close(rstd, (x.detach().var(-1, unbiased=False) + R.EPS).rsqrt())
        for r in (None, res):
            dx, dw, db = R.layernorm_bwd(dy, x.detach(), w.detach(), R.EPS, r)
            _close(dx, x.grad if r is None else x.grad + r)
            _close(dw, w.grad)
            _close(db, b.grad)


def test_gelu_and_swiglu_references_are_autograd():
    x = torch.linspace(-12, 12, 4801, dtype=F64).requires_grad_()
    y = F.gelu(x)
    y.sum().backward()
    _close(R.gelu(x.detach()), y.detach())
    _close(R.gelu_grad(x.detach()), x.grad)
    gen = _gen(3, 4)
    x12 = (64 * torch.rand(7, 2 * 36, generator=gen, dtype=F64) - 32)
    x12[:, 0], x12[:, 35] = -100.0, 100.0
    x12.requires_grad_()
    dh = torch.randn(7, 36, generator=gen, dtype=F64)
    (F.silu(x12[:, :36]) * x12[:, 36:]).backward(dh)
    _close(R.swiglu_bwd(x12.detach(), dh), x12.grad)


def test_packing_and_finish_references():
    gen = _gen(5, 6)
    img = torch.randn(2, 3, 28, 42, generator=gen)
    assert torch.equal(R.im2col(img, 14), F.unfold(img, 14, stride=14).transpose(1, 2).reshape(-1, 3 * 14 * 14))
    k = 2 * 196 + 5 * 14 + 3           # c = 2, i = 5, j = 3 of patch (1, 2) of image 1
    assert float(R.im2col(img, 14)[1 * 6 + 1 * 3 + 2, k]) == float(img[1, 2, 14 + 5, 28 + 3])
    x, cls, pos = torch.randn(3, 5, 8, generator=gen), torch.randn(8, generator=gen), torch.randn(6, 8, generator=gen)
    out = R.add_cls_pos(x, cls, pos)
    assert torch.equal(out[:, 0], (cls + pos[0]).expand(3, 8)) and torch.equal(out[:, 1:], x + pos[1:])
    # the finish against autograd of x + gamma (A W^T + b) in float64
    N, K, M = 5, 12, 9
    A, dout = torch.randn(M, K, generator=gen, dtype=F64), torch.randn(M, N, generator=gen, dtype=F64)
    W, b, ga = (torch.randn(s, generator=gen, dtype=F64).requires_grad_() for s in ((N, K), (N,), (N,)))
    ((ga * (A @ W.t() + b)) * dout).sum().backward()
    dW, db, dga = R.ls_linear_finish(dout.t() @ A, W.detach(), b.detach(), ga.detach(), dout.sum(0), 0.5)
    _close(dW, 0.5 * W.grad), _close(db, 0.5 * b.grad), _close(dga, 0.5 * ga.grad)
    dW, db, dga = R.ls_linear_finish(dout.t() @ A, None, None, None, dout.sum(0), 0.5)
    assert dga is None and torch.equal(dW, 0.5 * (dout.t() @ A)) and torch.equal(db, 0.5 * dout.sum(0))
    for dt in DT:
        v = torch.randn(1000, generator=gen) * 3
        hi, lo = R.split(v, dt)
        assert torch.equal(hi, v.to(dt)) and float((hi.double() + lo.double() - v.double()).abs().max()) <= 2.0 ** -15 * 16
        assert len(R.all_values(dt)) % 8 == 0
        for u in (v, v * 1e-5, R.all_values(dt).float()):          # normal, subnormal, every value itself
            assert torch.equal(R.round_to(u.double(), dt), u.to(dt).double())
    assert len(R.all_values(torch.float16)) == 63488


def test_row_block_rule_is_the_library_s():
    lib = _lib.lib()
    for rows in sorted({c[0] for c in R.LN_BWD} | {c[0] for c in R.COLSUM_CASES} | {32, 64, 65536, 65569, 1 << 20}):
        assert lib.asis_rowblock_nblk(rows) == min(-(-rows // 32), 2048) == R.rowblock(rows)[0], rows


def test_layernorm_forward_tables_reach_their_branches():
    assert {c[1] // 4 for c in R.LN_GENERIC} >= {1, 63, 64, 65, 512} and max(c[1] for c in R.LN_GENERIC) == 256 * 8
    assert {R.lane_trips(D) for D in R.LN_D} >= {1, 2, 4, 8}
    assert {c[0] % 4 for c in R.LN_GENERIC} == {0, 1, 2, 3} and {c[0] for c in R.LN_GENERIC} >= {1, 3, 4, 5}   # partial / full blocks
    for rows, D, ld in R.LN_GENERIC + R.STATS_CASES:
        assert not R.ln_fixed(rows, D, False) and (ld is None or (ld > D and ld % 4 == 0))
    assert any(c[2] for c in R.LN_GENERIC) and any(c[2] for c in R.STATS_CASES) and any(c[2] for c in R.LN_FIXED)
    for rows, D, ld, fixed, clamped, last in R.LN_FIXED:
        assert R.ln_fixed(rows, D, False) == fixed and not R.ln_fixed(rows, D, True) and not R.ln_fixed(rows, D, False, form=0)
        if fixed:
            assert clamped == (rows % 2 == 1) and last == (rows % 8 or 8)
    assert {(c[1], c[4], c[5] < 8) for c in R.LN_FIXED if c[3]} == {(D, cl, pl) for D in (768, 1024, 1536)
                                                                    for cl, pl in ((False, False), (True, True))}


def test_layernorm_backward_table_reaches_its_branches():
    seen = set()
    for rows, D, strided, maxc, nblk, rpb, waves, empty in R.LN_BWD:
        assert R.ln_bwd_maxc(D) == maxc and R.rowblock(rows) == (nblk, rpb, empty) and R.wave_rows(rows) == waves, (rows, D)
        seen.add((maxc, max(waves) >= 2))
    assert seen == {(m, pf) for m in (4, 6, 8) for pf in (False, True)}          # each MAXC with and without a second row
    assert {c[3] for c in R.LN_BWD if c[2]} == {4, 6, 8}                          # one strided case per MAXC
    assert {R.ln_bwd_maxc(D) for D in (1024, 1028, 1536, 1540)} == {4, 6, 8} and R.ln_bwd_maxc(1024) != R.ln_bwd_maxc(1028)
    assert any(c[7] is not None and c[4] == 2048 for c in R.LN_BWD)
    assert {R.lane_trips(c[1]) for c in R.LN_BWD} >= {1, 2, 4, 5, 6, 7, 8}


def test_colsum_table_reaches_its_branches():
    for rows, C16, C32, pad, nblk, rpb, unrolled, tail, gy16, gy32, trips in R.COLSUM_CASES:
        assert R.rowblock(rows)[:2] == (nblk, rpb) and (rpb // 4, rpb % 4) == (unrolled, tail), rows
        assert R.colsum_gy(C16, 8) == gy16 and R.colsum_gy(C32, 4) == gy32
        assert R.cdiv(C16 // 8, 256 * gy16) == trips == R.cdiv(C32 // 4, 256 * gy32)
        assert C16 % 8 == 0 and C32 % 8 == 0 and pad % 8 == 0
    assert any(c[0] == 65537 and R.rowblock(c[0])[2] == 1986 for c in R.COLSUM_CASES)
    assert 2 * R._BIG16 * 2 < 34e6 and 2 * R._BIG32 * 4 < 34e6


def test_finish_and_packing_tables_reach_their_branches():
    for N, K, trips, what in R.LS_CASES:
        assert R.lane_trips(K) == trips and K % 4 == 0
    assert {c[2] for c in R.LS_CASES} >= {1, 2, 4, 16} and {c[0] % 4 for c in R.LS_CASES} == {0, 1, 3}
    assert {c[3] for c in R.LS_CASES} >= {"all", "plain", "nobias", "nocs", "nodb", "nodgamma"}
    for rows, cols, ld_dst, ld_src, scale, part, over in R.CAST_PAD_CASES:
        assert ld_dst % 8 == 0 and ld_dst >= cols and ld_src >= cols and (rows * (ld_dst // 8) > R.PACK_GRID) == over
    assert {c[1] for c in R.CAST_PAD_CASES} >= {1, 7, 8, 9, 588} and any(c[6] for c in R.CAST_PAD_CASES)
    assert any(c[2] > -(-c[1] // 8) * 8 for c in R.CAST_PAD_CASES) and any(c[3] > c[1] for c in R.CAST_PAD_CASES)
    assert {(c[4], c[5]) for c in R.CAST_PAD_CASES} == {(1.0, 0), (0.37, 0), (1.0, 1), (0.37, 1)}
    for B, H, W, P, ldk, over in R.IM2COL_CASES:
        assert H % P == 0 and W % P == 0 and ldk % 8 == 0 and ldk >= 3 * P * P
        assert (B * (H // P) * (W // P) * (ldk // 8) > R.PACK_GRID) == over
    assert {(c[3], c[4] == -(-3 * c[3] ** 2 // 8) * 8) for c in R.IM2COL_CASES} == {(14, True), (14, False), (16, True), (16, False)}
    assert any(c[1] != c[2] for c in R.IM2COL_CASES) and any(c[5] for c in R.IM2COL_CASES)
    for B, N, D, over in R.CLS_POS_CASES:
        assert (B * (N + 1) * (D // 4) > R.PACK_GRID) == over
    assert 0 < 2 * 1370 * 384 - R.PACK_GRID < 4096                 # "just above the cap"


def test_input_rules_layernorm():
    """no row is constant, the yardstick of every bounded output is non-zero, no 16-bit value overflows"""
    for rows, D, _ in R.LN_GENERIC + R.STATS_CASES + [c[:3] for c in R.LN_FIXED]:
        x, w, b, y64, y32, mean64, rstd64, mean32, rstd32 = R.ln_fwd_case(rows, D)
        assert float(x.double().std(-1, unbiased=False).min()) > 0.01, (rows, D)
        assert float((x.double().mean(-1) / x.double().std(-1, unbiased=False)).abs().min()) > 15       # a heavy mean
        assert float((y32.double() - y64).abs().max()) > 0 and float(y64.abs().max()) < 100, (rows, D)
        if (rows, D, _) in R.STATS_CASES:
            assert float((mean32.double() - mean64).abs().max()) > 0 and float((rstd32.double() - rstd64).abs().max()) > 0, (rows, D)
    for rows, D, *_ in R.LN_BWD:
        dy, x, w, res, refs = R.ln_bwd_case(rows, D)
        assert float(x.detach().double().std(-1, unbiased=False).min()) > 0.01, (rows, D)
        for with_res in (True, False):
            for name, ref, f32 in zip(("dx", "dweight", "dbias"), *refs[with_res]):
                # one row: dbias is dy itself, exact in any precision, and the ulp term is the whole bound
                assert float((f32.double() - ref).abs().max()) > 0 or (rows == 1 and name == "dbias"), (rows, D, with_res, name)


def test_input_rules_elementwise_and_sums():
    for dt in DT:
        pre = R.all_values(dt)
        assert float(R.gelu(pre).abs().max()) <= MAX16[dt] and float(pre.float().abs().max()) <= 65504.0
        assert float((R.gelu_grad(pre) * 3).abs().max()) <= MAX16[dt]
    assert float(R.gelu_grid().abs().max()) <= 65504.0
    for rows, Hd in R.SWIGLU_CASES:
        x12, dhs = R.swiglu_case(rows, Hd)
        assert bool((x12[:, 0] == -100).all()) and bool((x12[:, Hd - 1] == 100).all())
        mid = x12[:, 1:Hd - 1]
        assert float(mid.abs().max()) <= 32 and (Hd < 100 or float(mid.min()) < -30 and float(mid.max()) > 30)
        for dt in DT:
            ref = R.swiglu_bwd(x12, dhs[dt])
            assert float(ref.abs().max()) <= MAX16[dt] and bool(torch.isfinite(ref).all())
            assert float((R.swiglu_f32(x12, dhs[dt]).double() - ref).abs().max()) > 0
            # the two extreme columns: exactly 0, dh x2 (exact in fp32) and dh x1
            assert bool((ref[:, 0].to(dt) == 0).all()) and bool((ref[:, Hd].to(dt) == 0).all())
            prod = dhs[dt][:, -1].float() * x12[:, -1]
            assert torch.equal(prod.double(), dhs[dt][:, -1].double() * x12[:, -1].double())
    for rows, C16, C32, *_ in R.COLSUM_CASES:
        for dt, C in ((torch.float16, C16), (torch.bfloat16, C16), (torch.float32, C32)):
            x = R.colsum_input(rows, C, dt)
            # a handful of 16-bit rows (or one fp32 row) sums exactly in fp32: Y = 0 there and the ulp term is the whole bound
            assert float((x.float().sum(0).double() - R.colsum(x)).abs().max()) > 0 or rows <= 7, (rows, C, dt)
    for N, K, trips, what in R.LS_CASES:
        t = R.ls_case(N, K, what)
        if t["gamma"] is not None:
            ref = R.ls_linear_finish(t["G"], t["W"], t["bias"], t["gamma"], t["cs"], t["gs"])[2]
            assert float((R.ls_f32(t).double() - ref).abs().max()) > 0, (N, K, what)
    assert math.isclose(float(R.gelu(torch.tensor([4.0]))), 4.0 * (1 - 3.167124183311998e-05), rel_tol=1e-12)
