"""GPU: every route of the deformable-attention sampling kernels (csrc/msda.hip, the MSDA half of csrc/adapter_bwd.hip) against
the float64 restatement of tests/msda_ref.py, element by element: |got - ref| <= tol for ALL elements, a failure names the worst
element and its (b, q / pixel, head*Dh + channel).  tests/test_msda_ref_cpu.py shows on the CPU that these bounds hold for a float32
evaluation of the reference and are broken by a wrong corner weight, a clamped border and a swapped level size.

Bounds.  u = 2^-24 (fp32), u16 = 2^-11 for fp16 / 2^-8 for bf16: the most a round-to-nearest 16-bit store is off by, relative (half
an ulp just above a power of two).  `S_abs` is the sum of the absolute values of the terms of an element, `S_pos` the first-order
effect of the fp32 sampling position on it (both from the reference, see tests/msda_ref.py).

  out        u16 |ref| + 2^-16 S_abs + S_pos (+ 2^-25 for fp16: half the spacing of its subnormals)
             the fp32 path sums <= 64 tap products, each with <= 12 roundings in its weight chain: < 2^7 u = 2^-17; the softmax
             through __expf is within 2^-20 when the logits lie within 4 of their maximum (one rounding of x log2(e) at |x| <= 4 and
             a 1-ulp exp2, numerator and denominator), and the generator keeps the spread <= 4.  Rounded up once: 2^-16, 32 times
             under fp16's output rounding and 2^15 times under an O(1) tap error.
  out + lo   u16^2 |ref| + 2^-16 S_abs + S_pos + 2^-24   (both halves widened to fp32, then float64; 2^-24: fp16 out_lo may underflow)
  d off      (n + 16) 2 u S_abs + S_pos,  n = 4 Dh products along the kernel's path      (fp32 worst case n u; the 2 covers the softmax)
  d logit    the same with n = 4 Dh + L P
  d value    n = the number of taps on that pixel, from the reference.   scatter routes: (n + 16) 2 u S_abs + S_pos
             sorted route: + n max(amax 2^-29, 2^-126): the fixed-point grid, half a step per record, doubled; the step is
                           2^(e - 29) <= amax 2^-29 with e the exponent of amax, which the kernel keeps >= -97
             matrix route: + u16 S_abs: the merged weights are stored in 16 bits
  and the sorted route is bit for bit equal run to run.

Two terms are not in the list the bounds were first written from; both come from the arithmetic, not from what the kernels gave:
  * u16, not u16 / 2, multiplies |ref|: a correctly rounded fp16 of 1 + 2^-11 is off by 2^-11.
  * S_pos.  px = (rx + ox / W) W - 0.5 takes four fp32 roundings of numbers up to W + |ox|, |px_fp32 - px| <= 4 u (|rx| W + |ox| + 0.5):
    2^-16 px on a 128-pixel level.  A tap whose weight is 2^-7 then has a RELATIVE error of 2^-9, which no multiple of u S_abs
    covers.  The float32 restatement misses the bounds without it (test_bounds_without_the_position_term_...).
Random cases never sit within 2^-8 px of a cell boundary (the generator moves such offsets by 2^-6 px, none is excluded), so both
sides choose the same cell; "exact" cases make the kernel's fp32 px exact (power-of-two levels, dyadic ref and offsets)."""
import functools
import math

import pytest
import torch

from adaptersis_amd import ops
from adaptersis_amd._lib import AsisError
from tests import msda_ref as R

pytestmark = pytest.mark.gpu
REFUSED = (ValueError, AsisError)
_ID = {torch.float16: "fp16", torch.bfloat16: "bf16"}


@functools.lru_cache(maxsize=None)
def _case(kind, i, dtype, scale=1.0):
    if kind == "fwd":
        case = R.fwd_case(R.FWD_CASES[i], dtype)
    elif kind == "red":
        case = R.red_case(R.RED_CASES[i], dtype)
    elif kind == "lin":
        case = R.lin_case(R.LIN_CASES[i], dtype)
    else:
        case = R.sm_case(R.SM_CASES[i], dtype, scale)
    assert case["excluded"] == 0
    return case, R.reference_of(case)


def _geom(case, dev):
    sh = torch.tensor(case["shapes"], dtype=torch.int32, device=dev)
    st = torch.tensor(R.starts_of(case["shapes"]), dtype=torch.int32, device=dev)
    return case["ref"].to(dev), sh, st


def _value(case, dev):
    """value with one more image behind it, all NaN: a kernel that reads past its image shows up"""
    B, Lin, D = case["value"].shape
    buf = torch.full((B + 1, Lin, D), float("nan"), dtype=case["dtype"], device=dev)
    buf[:B] = case["value"].to(dev)
    return buf[:B]


def _bwd(case, dev, dense, sorted_route=True):
    ref, sh, st = _geom(case, dev)
    old = ops.MSDA_SORTED
    ops.MSDA_SORTED = sorted_route
    try:
        return ops.msda_bwd(_value(case, dev), case["offaw"].to(dev), ref, sh, st, case["dout"].to(dev), case["B"], case["Lq"],
                            case["M"], len(case["shapes"]), case["P"], dense=dense)
    finally:
        ops.MSDA_SORTED = old


def _check_doffaw(tag, case, r, doffaw, rows=None):
    M, Dh, LP = case["M"], case["Dh"], len(case["shapes"]) * case["P"]
    n = M * LP * 2
    sel = slice(None) if rows is None else rows
    got = doffaw.cpu()
    a = R.assert_within(f"{tag} d off", got[sel, :n], r["ref"]["doff"][sel], R.tol_doff(r, Dh)[sel], "b*Lq+q, (m,l,p,xy)")
    b = R.assert_within(f"{tag} d logit", got[sel, n:], r["ref"]["dlogit"][sel], R.tol_dlogit(r, Dh, LP)[sel], "b*Lq+q, (m,l,p)")
    return a, b


def _ids(cases, name=lambda c: c[0]):
    return [name(c) for c in cases]


# ---- forward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ID.get)
@pytest.mark.parametrize("i", range(len(R.FWD_CASES)), ids=_ids(R.FWD_CASES))
def test_forward(dev, i, dtype):
    """out and the split pair (out, out_lo) on every case: NC=1 (Dh 8, 24) and NC=2 (Dh 16, 32, 128), L*P from 1 to 16, levels one
    pixel high or wide, random and exact points (centres, the zero-padding border, offsets beyond the int range)"""
    case, r = _case("fwd", i, dtype)
    B, Lq, M, P, L = case["B"], case["Lq"], case["M"], case["P"], len(case["shapes"])
    ref, sh, st = _geom(case, dev)
    value, offaw = _value(case, dev), case["offaw"].to(dev)
    out, lo = ops.msda_fwd(value, offaw, ref, sh, st, B, Lq, M, L, P, split=True)
    plain = ops.msda_fwd(value, offaw, ref, sh, st, B, Lq, M, L, P)
    assert torch.equal(out, plain)
    tag = f"{case['name']} {_ID[dtype]}"
    R.assert_within(f"{tag} out", out.view(B, Lq, -1), r["ref"]["out"], R.tol_out(r, dtype), "b, q, m*Dh+c")
    R.assert_within(f"{tag} out+lo", out.view(B, Lq, -1).double() + lo.view(B, Lq, -1).double(), r["ref"]["out"],
                    R.tol_split(r, dtype), "b, q, m*Dh+c")
    # what the reference gives as exactly zero (every point of the head outside its level, e.g. 3e9 px away) is exactly zero
    dead = (r["abs"]["out"] == 0).to(dev)
    assert float(out.view(B, Lq, -1)[dead].float().abs().sum()) == 0.0 and float(lo.view(B, Lq, -1)[dead].float().abs().sum()) == 0.0


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ID.get)
def test_forward_wide_offaw_rows(dev, dtype):
    """offaw as a column slice of a wider tensor whose other columns hold NaN: ld_offaw > M*L*P*3"""
    i = _ids(R.FWD_CASES).index("m8d32-pyr3-p4")
    case, r = _case("fwd", i, dtype)
    B, Lq, M, P, L = case["B"], case["Lq"], case["M"], case["P"], len(case["shapes"])
    n = M * L * P * 3
    wide = torch.full((B * Lq, n + 13), float("nan"), device=dev)
    wide[:, :n] = case["offaw"].to(dev)
    ref, sh, st = _geom(case, dev)
    out = ops.msda_fwd(_value(case, dev), wide[:, :n], ref, sh, st, B, Lq, M, L, P)
    assert torch.equal(out, ops.msda_fwd(_value(case, dev), case["offaw"].to(dev), ref, sh, st, B, Lq, M, L, P))
    R.assert_within(f"wide offaw {_ID[dtype]} out", out.view(B, Lq, -1), r["ref"]["out"], R.tol_out(r, dtype), "b, q, m*Dh+c")


# ---- d offsets / d logits: both forms of the per-head reduction ----------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ID.get)
@pytest.mark.parametrize("i", range(len(R.RED_CASES)), ids=_ids(R.RED_CASES, lambda c: f"m{c[0]}d{c[1]}-{c[2]}"))
def test_backward_reduction_forms(dev, i, dtype):
    """msda_bwd_kernel's xor-shuffle reduction (head groups of 16, 8, 2, 32, 16 lanes; 256 threads) and its LDS-atomics
    reduction (a group of 12, of 128, D % 512 != 0, D = 48): d off, d logit and the scattered d value against float64"""
    M, Dh, form = R.RED_CASES[i]
    cph, cpq = Dh // 8, M * Dh // 8
    assert ((cph & (cph - 1)) == 0 and cph <= 64 and cpq % 64 == 0) == (form == "shuffle")     # the kernel's own condition
    case, r = _case("red", i, dtype)
    dvalue, doffaw = _bwd(case, dev, dense=False)
    tag = f"{case['name']} {_ID[dtype]} {form}"
    _check_doffaw(tag, case, r, doffaw)
    R.assert_within(f"{tag} d value (scatter)", dvalue, r["ref"]["dvalue"], R.tol_dvalue(r, M, "scatter"), "b, pixel, m*Dh+c")


# ---- d value, scatter: the kernel that Lin selects -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ID.get)
@pytest.mark.parametrize("i", range(len(R.LIN_CASES)), ids=_ids(R.LIN_CASES, lambda c: "%dx%d" % c[0]))
def test_dvalue_scatter_by_lin(dev, i, dtype):
    """Lin = 4096 -> msda_bwd_dvalue_kernel<8>, 4160 -> <4>, 8256 -> <2>, 16512 -> the global-atomics msda_bwd_kernel<T, true>"""
    (H, W), route = R.LIN_CASES[i]
    Lin = H * W
    ch = next((c for c in (8, 4, 2) if Lin * c * 4 <= 128 * 1024), 0)                          # asis_msda_bwd's own choice
    assert {8: "tile<8>", 4: "tile<4>", 2: "tile<2>", 0: "global atomics"}[ch] == route
    case, r = _case("lin", i, dtype)
    dvalue, doffaw = _bwd(case, dev, dense=False)
    tag = f"{case['name']} {_ID[dtype]} {route}"
    R.assert_within(f"{tag} d value", dvalue, r["ref"]["dvalue"], R.tol_dvalue(r, 1, "scatter"), "b, pixel, c")
    _check_doffaw(tag, case, r, doffaw)


# ---- d value, sorted and matrix ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ID.get)
@pytest.mark.parametrize("i", range(len(R.SM_CASES)), ids=_ids(R.SM_CASES))
def test_dvalue_sorted_and_matrix(dev, i, dtype):
    """Dh 16 .. 1024 (msda_vgrad_kernel's lane loop from 256 on), one cell that collects every record while most buckets stay empty,
    Lq = 1; the sorted route twice, bit for bit"""
    case, r = _case("sm", i, dtype)
    M = case["M"]
    assert (M * case["Dh"]) % 64 == 0
    if R.SM_CASES[i][7]:
        assert int(r["count"].max()) > 8 and float((r["count"] == 0).double().mean()) > 0.5
    amax = float(case["dout"].abs().max())
    tag = f"{case['name']} {_ID[dtype]}"
    dv, doffaw = _bwd(case, dev, dense=True, sorted_route=True)
    dv2, _ = _bwd(case, dev, dense=True, sorted_route=True)
    assert torch.equal(dv, dv2), "sorted form is not reproducible run to run"
    R.assert_within(f"{tag} d value (sorted)", dv, r["ref"]["dvalue"], R.tol_dvalue(r, M, "sorted", dtype, amax), "b, pixel, m*Dh+c")
    _check_doffaw(tag, case, r, doffaw)
    dm, _ = _bwd(case, dev, dense=True, sorted_route=False)
    R.assert_within(f"{tag} d value (matrix)", dm, r["ref"]["dvalue"], R.tol_dvalue(r, M, "matrix", dtype), "b, pixel, m*Dh+c")


@pytest.mark.parametrize("scale", R.AMAX_SCALES, ids=lambda s: "0" if s == 0 else "2^%g" % math.log2(s))
def test_sorted_fixed_point_scale_over_the_exponent_range(dev, scale):
    """the fixed-point scale of msda_vgrad_kernel is built from amax's exponent: finite everywhere, within the bound down to
    2^-96, below that within the bound or exactly zero (bf16: its dout16 keeps fp32's exponent range)"""
    case, r = _case("sm", 0, torch.bfloat16, scale)
    amax = float(case["dout"].abs().max())
    dv, _ = _bwd(case, dev, dense=True, sorted_route=True)
    assert bool(torch.isfinite(dv).all()), f"d value is not finite at dout x {scale:g} (amax {amax:g})"
    got = dv.cpu().double()
    if scale < 2.0 ** -96:
        got = torch.where(got == 0, r["ref"]["dvalue"], got)
    R.assert_within(f"sorted, dout x {scale:g}", got, r["ref"]["dvalue"], R.tol_dvalue(r, case["M"], "sorted", torch.bfloat16, amax),
                    "b, pixel, m*Dh+c")
    if scale == 0:
        assert float(dv.abs().sum()) == 0.0


# ---- more rows than blocks ---------------------------------------------------------------------------------------------
def test_backward_grid_stride(dev):
    """B*Lq = 65535*8 + 300: the last 300 rows are a block's second trip through msda_bwd_kernel's loop, on an LDS `red[]` it has
    used before"""
    case = R.grid_stride_case()
    r = R.reference_of(case)
    dvalue, doffaw = _bwd(case, dev, dense=False)
    rows = torch.cat([torch.arange(300) * 1747 % (65535 * 8), torch.arange(R.GS_ROWS - 300, R.GS_ROWS)])
    assert int((rows[:300] < 65535 * 8).all()) and rows[:300].unique().numel() == 300
    _check_doffaw("grid-stride", case, r, doffaw, rows)
    R.assert_within("grid-stride d value", dvalue, r["ref"]["dvalue"], R.tol_dvalue(r, 1, "scatter"), "b, pixel, c")


# ---- refusals: the library's error, no kernel ------------------------------------------------------------------------------
def _tiny(dev, M, Dh, L, P, cols=None, Lq=3):
    shapes = [(2, 2)] * L
    value = torch.zeros((1, 4 * L, M * Dh), dtype=torch.float16, device=dev)
    offaw = torch.zeros((Lq, M * L * P * 3 if cols is None else cols), device=dev)
    ref = torch.full((Lq, 2), 0.5, device=dev)
    sh = torch.tensor(shapes, dtype=torch.int32, device=dev)
    st = torch.tensor(R.starts_of(shapes), dtype=torch.int32, device=dev)
    dout = torch.zeros((Lq, M * Dh), device=dev)
    return (value, offaw, ref, sh, st), dout, (1, Lq, M, L, P)


def test_refusals(dev):
    a, dout, s = _tiny(dev, 1, 12, 1, 4)                         # Dh = 12
    with pytest.raises(REFUSED):
        ops.msda_fwd(*a, *s)
    with pytest.raises(REFUSED):
        ops.msda_bwd(*a, dout, *s, dense=False)
    a, dout, s = _tiny(dev, 1, 8, 1, 17)                         # L*P = 17
    with pytest.raises(REFUSED):
        ops.msda_fwd(*a, *s)
    with pytest.raises(REFUSED):
        ops.msda_bwd(*a, dout, *s, dense=False)
    a, dout, s = _tiny(dev, 33, 8, 1, 2)                         # M = 33: the backward's red[] holds 32 heads
    with pytest.raises(REFUSED):
        ops.msda_bwd(*a, dout, *s, dense=False)
    a, dout, s = _tiny(dev, 1, 2056, 1, 2)                       # M*Dh = 2056: 257 threads
    with pytest.raises(REFUSED):
        ops.msda_bwd(*a, dout, *s, dense=False)
    a, dout, s = _tiny(dev, 2, 8, 1, 4, cols=2 * 4 * 3 - 1)      # ld_offaw one short
    with pytest.raises(REFUSED):
        ops.msda_fwd(*a, *s)
    with pytest.raises(REFUSED):
        ops.msda_bwd(*a, dout, *s, dense=False)
    a, dout, s = _tiny(dev, 2, 8, 1, 4)                          # and the same shapes, whole, are accepted
    ops.msda_fwd(*a, *s)
    ops.msda_bwd(*a, dout, *s, dense=False)
