"""GPU: every kernel form of ``asis_gemm`` (csrc/gemm.hip: gemm_plan; kernels in gemm.hip, gemm_big.h, gemm_p8.h) element by
element against float64, on the smallest shapes that still straddle a tile edge.  The cells, the operands, the float64
restatement and the checker are tests/gemm_ref.py; test_gemm_ref_cpu.py proves on the CPU that every cell plans to the form it
names, that the table has every form, and that the checker fails on realistic mistakes.

Each cell builds its descriptor through ``ops._gemm_desc`` / ``ops._conv_desc`` (the descriptor half of ``ops.conv_gemm``),
asserts that ``ops.gemm_plan`` of THAT descriptor is the cell's form, launches it twice into fresh sentinel-filled buffers,
requires the two results to be bit-identical (pads included), the pads untouched, and runs the checker over all elements.
Guards: A and B carry one NaN row and 8 NaN columns (lda = ldb = K + 8), outputs 8 pad columns and a pad row, convolution inputs
a NaN image on either side, stats / rowstats tables a guard row.  All of it is allocated memory.

Bounds (gemm_ref.py has the derivations):
  exact cells   integer operands, power-of-two scales: fp32 outputs BIT-EQUAL to float64, 16-bit outputs equal to
                ``ref.float().to(dt)`` (to_t16 rounds to nearest even), plane pairs (out, out_lo) both bit-equal.
  random cells  |got - ref| <= max(4 Y, U ulp32 max|ref|), Y = error of torch's float32 CPU evaluation, U = 4 for outputs and 16
                for column / row sums (tests/bound_helpers.py); + 2^-11 (fp16) or 2^-8 (bf16) |ref| + half a subnormal for a
                16-bit output, the pair's 2^-21 / 2^-15 for two planes.
  approximated  gelu_erf: + 5.2e-8 |scale_n|; gelu_erf_grad_fast: + 7.0e-8 |acc| |scale_n|.  Both figures are the worst gap of a
                float64 restatement of the FORMULA (csrc/asis_common.h) to the exact erf form on a dense grid (measured 5.17e-8 on
                [-12, 12] and 6.97e-8 on [-8, 8]; test_gemm_ref_cpu.py pins them), never of a kernel; the float32 rounding of
                the two formulas enters Y (the larger of the exact and the restated formula's float32 error).
  stats         the [ceil(M / 128), 2, N] table row by row: a tile's first row carries the tile's sums within the sum bound,
                the other rows it covers are zero (csrc/gemm_big.h), so the column totals hold too.

The exact-sum assumption (MFMA accumulation keeps exactly representable sums exact) is controlled by the ``generic`` cells, the
simplest kernel.  On the MI355X it HELD: every exact cell of every form, fp16 and bf16, 32x32x16 and 16x16x32 MFMAs, K parts and
split-precision parts included, is bit-equal to float64 (largest error 0), so an inexact exact cell is a finding about the form.

The scalar-epilogue cells (gemm_ref.MISALIGNED): the large-tile kernel picks its vector or scalar epilogue at run time, also from
the alignment of bias_n / scale_n / res, which the plan did not look at; the scalar fallback writes no statistics, applies no
GELU' and adds bias_n in every K part.  OUTCOME: the defect was real.  Run as correctness cells on the MI355X before the fix,
bias_n 4 bytes into its allocation left all 816 statistics of a conv_256x128 launch unwritten, gave 41184 of 42432 elements of
a ksplit = 3 sum three times the bias, and 40632 of 40800 outputs of a dense GELU' launch without the GELU' factor; res 8 bytes
in did the same to 40760 of 40800.  asis_gemm_plan now evaluates the kernel's own predicate (csrc/gemm_big.h:
gemm_big_vec_epilogue) and refuses statistics, GELU' and K parts off the vector epilogue with ASIS_EINVAL, naming the operand;
test_scalar_epilogue_cells asserts the refusal by the plan and by the launch (test_gemm_plan.py: the same four descriptors on
the CPU).  Plain scalar cells (N = 130, N = 262: no statistics, no GELU', no K
parts) are ordinary correctness cells here.

Left out on purpose: the MX forms (ph8_mx, conv_*_mx: their accuracy is the fp8 plane's; test_gpu_mx.py), the LayerNorm-fold
consumer (ln_mr: p8_ln, and ph8_ln with ln; inexact by nature; test_gpu_lnfold.py), and the forms reachable only through
ASIS_GEMM_* / ASIS_CONV_* environment switches, which are read once per process (ph8_m32, big_256x128, big_256x128_k64,
big_256x256, conv_512x64_split_m16, conv_256x128_split_m16, conv_256x128_split_bk32)."""
import ctypes as C

import pytest
import torch

from adaptersis_amd import ops
from adaptersis_amd._lib import ACT_SILU_MUL
from tests import gemm_ref as G

pytestmark = pytest.mark.gpu


@pytest.fixture
def p8_option():
    yield lambda v: ops.gemm_set_option("p8", v)
    ops.gemm_set_option("p8", 1)


@pytest.fixture(scope="module")
def device_operands(dev):
    """guarded device copies of the operands, one set per shape (Cell fields that pick among them do not enter the key)"""
    cache = {}

    def get(cell):
        key = (G._key(cell), cell.off, cell.act == ACT_SILU_MUL)
        if key not in cache:
            cache[key] = _place(cell, dev)
        return cache[key]

    return get


def _place(cell, dev):
    o, off = G.operands(cell), dict(cell.off)
    t = {}
    if cell.conv:
        B, H, W, Cin = o["A"].shape
        for name in ("A", "A_lo"):
            buf = torch.full((B + 2, H, W, Cin), float("nan"), dtype=cell.dt, device=dev)
            buf[1:1 + B] = o[name].to(cell.dt)
            t[name] = buf[1:1 + B]
    else:
        for name in ("A", "A_lo"):
            t[name] = G.guarded(o[name], cell.dt, dev)[1]
    rows = ops.swiglu_rows(cell.N // 2, "cpu") if cell.act == ACT_SILU_MUL else slice(None)
    for name in ("B", "B_lo"):
        t[name] = G.guarded(o[name][..., rows, :] if cell.act == ACT_SILU_MUL else o[name], cell.dt, dev)[1]
    t["bias_n"] = G.guarded_vec(o["bias_n"][rows], dev, off.get("bias_n", 0))
    t["bias_m"], t["scale_n"] = G.guarded_vec(o["bias_m"], dev), G.guarded_vec(o["scale_n"], dev)
    if not cell.conv:
        t["res"] = G.guarded(o["res"], torch.float32, dev, off=off.get("res", 0))[1]
        t["aux"] = G.guarded(o["aux"], cell.dt, dev)[1]
        hi = o["res"].to(cell.dt)
        t["res16"] = (G.guarded(hi.float(), cell.dt, dev)[1], G.guarded(o["res"] - hi.float(), cell.dt, dev)[1])
    return t


def _descriptor(cell, t, dev):
    """fresh sentinel-filled outputs and the descriptor that writes them -> (d, {name: (flat allocation, written view)})"""
    kw = {name: t[name] for name in ("bias_n", "bias_m", "scale_n", "res", "aux", "res16") if name in cell.has}
    bufs = {}
    if "stats" in cell.has:
        rows = ops.gemm_tiles_m(cell.M)
        flat = torch.full(((rows + 1) * 2 * cell.N,), G.SENTINEL, device=dev)
        bufs["stats"] = (flat, flat[:rows * 2 * cell.N].view(rows, 2, cell.N))
        kw["stats"] = bufs["stats"][1]
    if cell.conv:
        B, H, W, Cin, k, s, p, OH, OW = cell.geometry()
        if "A_lo" in cell.has:
            kw.update(x_lo=t["A_lo"], w_lo=t["B_lo"])
        if cell.ksplit > 1:
            d, parts, _ = ops._conv_desc(t["A"], t["B"], k, k, s, p, ksplit=cell.ksplit, **kw)
            parts.fill_(G.SENTINEL)
            bufs["parts"] = (parts.view(-1), parts.view(cell.ksplit, cell.M, cell.N))
            return d, bufs
        flat = torch.full(((B + 1) * OH * OW * cell.N,), G.SENTINEL, dtype=cell.out_dt, device=dev)
        out = flat[:cell.M * cell.N].view(B, OH, OW, cell.N)
        d, _, _ = ops._conv_desc(t["A"], t["B"], k, k, s, p, out=out, **kw)
        bufs["out"] = (flat, out.view(cell.M, cell.N))
        return d, bufs
    if "A_lo" in cell.has:
        kw["a_lo"] = t["A_lo"]
    if "B_lo" in cell.has:
        kw["b_lo"] = t["B_lo"]
    bufs["out"] = G.out_buffer(cell, dev)
    if "C_lo" in cell.has:
        bufs["out_lo"] = G.out_buffer(cell, dev)
        kw["out_lo"] = bufs["out_lo"][1]
    if "rowstats" in cell.has:
        flat = torch.full(((cell.M + 1) * (cell.N // 64) * 2,), G.SENTINEL, device=dev)
        bufs["rowstats"] = (flat, flat[:cell.M * (cell.N // 64) * 2].view(cell.M, cell.N // 64, 2))
        kw["rowstats"] = bufs["rowstats"][1]
    d, _, _, _ = ops._gemm_desc(t["A"], t["B"], out=bufs["out"][1], act=cell.act, **kw)
    assert (d.A_lo is not None) == ("A_lo" in cell.has) and (d.B_lo is not None) == ("B_lo" in cell.has)
    return d, bufs


def _launch(d):
    ops.check(ops.lib().asis_gemm(ops._stream(), C.byref(d)), "asis_gemm")


def run_cell(cell, get, dev, p8_option):
    p8_option(cell.p8)
    t = get(cell)
    runs = []
    for _ in range(2):
        d, bufs = _descriptor(cell, t, dev)
        assert ops.gemm_plan(d)[0] == cell.form, (cell.name, ops.gemm_plan(d))
        _launch(d)
        runs.append(bufs)
    torch.cuda.synchronize()
    first, second = runs
    for name in first:
        same = first[name][0] == second[name][0]
        assert bool(same.all()), "%s %s: %d elements differ between two launches" % (cell.name, name, int((~same).sum()))
    e = G.expectations(cell)
    worst = {}
    for name, (flat, view) in first.items():
        G.check_pad(cell, name, flat, view)
    if "parts" in first:      # K parts: three partial maps; their sum is the convolution, with the bias exactly once
        parts = first["parts"][1].cpu()
        out = ((parts[0] + parts[1]) + parts[2])[None]
    else:
        out = first["out"][1].cpu().reshape(e["out"].ref.shape)
    if "out_lo" in first:
        lo = first["out_lo"][1].cpu().reshape(out.shape)
        if cell.exact:
            worst["out_lo"] = G.check(cell, "out_lo", lo, e["out_lo"])
        else:
            out = out.double() + lo.double()
    worst["out"] = G.check(cell, "out", out, e["out"])
    for name in ("stats", "rowstats"):
        if name in first:
            worst[name] = G.check(cell, name, first[name][1], e[name])
    print(cell.name, " ".join("%s %.3e" % kv for kv in worst.items()))


def ids(c):
    return c.name


@pytest.mark.parametrize("cell", G.family("dense"), ids=ids)
def test_dense_forms(cell, device_operands, dev, p8_option):
    run_cell(cell, device_operands, dev, p8_option)


@pytest.mark.parametrize("cell", G.family("split"), ids=ids)
def test_split_forms(cell, device_operands, dev, p8_option):
    run_cell(cell, device_operands, dev, p8_option)


@pytest.mark.parametrize("cell", G.family("producer"), ids=ids)
def test_producer_form(cell, device_operands, dev, p8_option):
    run_cell(cell, device_operands, dev, p8_option)


@pytest.mark.parametrize("cell", G.family("p8"), ids=ids)
def test_persistent_form(cell, device_operands, dev, p8_option):
    run_cell(cell, device_operands, dev, p8_option)


@pytest.mark.parametrize("cell", G.family("conv"), ids=ids)
def test_conv_forms(cell, device_operands, dev, p8_option):
    run_cell(cell, device_operands, dev, p8_option)


@pytest.mark.parametrize("cell", G.family("conv_split"), ids=ids)
def test_conv_split_forms(cell, device_operands, dev, p8_option):
    run_cell(cell, device_operands, dev, p8_option)


@pytest.mark.parametrize("cell", G.MISALIGNED, ids=ids)
def test_scalar_epilogue_cells(cell, device_operands, dev, p8_option):
    """statistics, GELU' or K parts with an operand off its 16-byte boundary: refused, naming the operand, by the plan and by the
    launch; nothing is written"""
    t = device_operands(cell)
    d, bufs = _descriptor(cell, t, dev)
    assert dict(cell.off)[cell.refused] * 4 % 16 != 0 and getattr(d, cell.refused) % 16 != 0
    with pytest.raises(ValueError, match=cell.refused):
        ops.gemm_plan(d)
    with pytest.raises(ValueError, match="%s.*16-byte" % cell.refused):
        _launch(d)
    torch.cuda.synchronize()
    for name, (flat, view) in bufs.items():
        assert bool((flat == G.SENTINEL).all()), name
