"""CPU: the table, the generators and the checker of tests/gemm_ref.py, which test_gpu_gemm_forms.py runs on the device.
1. every cell plans to the form it names (asis_gemm_plan on a descriptor with placeholder pointers, laid out as the GPU test lays
   out its guarded tensors); 2. the forms of the table are all the forms there are, minus the explicit left-out list; 3. exact
   cells are exact in float32 on the CPU and exercise the 16-bit rounding, random cells stay inside their own bounds; 4. the
   checker fails on the mistakes a GEMM tile, epilogue or convolution gather realistically makes."""
import pytest
import torch

from adaptersis_amd import _lib, ops
from adaptersis_amd._lib import ACT_RELU
from tests import gemm_ref as G
from tests.test_gemm_plan import PTR, mk, plan

ALL = G.CELLS + G.MISALIGNED


def desc(cell: G.Cell):
    """the descriptor of the cell's launch as test_gpu_gemm_forms.py builds it (guard columns in every leading dimension)"""
    has = [h for h in cell.has] + (["res16_lo"] if "res16" in cell.has else [])
    M, N, K = cell.M, cell.N, cell.K
    kw = dict(dtype=_lib.ASIS_F16 if cell.dt == G.F16 else _lib.ASIS_BF16, out_f32=int(cell.out_f32), act=cell.act)
    if cell.conv:
        B, H, W, Cin, k, s, p, OH, OW = cell.geometry()
        kw.update(B_=B, H=H, W=W, OH=OH, OW=OW, stride=s, pad=p, ldb=K + 8, ldc=N, ldr=N)
        if cell.ksplit > 1:
            kw.update(ksplit=cell.ksplit, strideC=M * N)
        d = mk(M, N, K, has, conv=k, **kw)
    else:
        ld = cell.n_out + 8
        kw.update(lda=K + 8, ldb=K + 8, ldc=ld, ldr=N + 8, ldr16=N + 8, ld_aux=N + 8, batch=cell.batch)
        if cell.batch > 1:
            kw.update(strideB=(N + 1) * (K + 8), strideC=(M + 1) * ld + cell.stride_c_off)
        d = mk(M, N, K, has, **kw)
    for name, elements in cell.off:
        setattr(d, name, PTR + 4 * elements)
    return d


@pytest.fixture
def p8_option():
    yield lambda v: ops.gemm_set_option("p8", v)
    ops.gemm_set_option("p8", 1)


@pytest.mark.parametrize("cell", ALL, ids=lambda c: c.name)
def test_cell_plans_to_its_form(cell, p8_option):
    p8_option(cell.p8)
    got = plan(desc(cell))
    if cell.refused:
        assert isinstance(got, str) and cell.refused in got and "16-byte" in got, got
    else:
        assert not isinstance(got, str), got
        assert got[0] == cell.form, got
        assert got[2] == (cell.ksplit if cell.conv else cell.batch)


def test_table_covers_every_form():
    lib = _lib.lib()
    names = {lib.asis_gemm_form_name(i).decode() for i in range(64)} - {"?"}
    assert len(names) == 28
    assert {c.form for c in G.CELLS} == names - G.LEFT_OUT
    assert G.LEFT_OUT <= names and set(G.TILE) == names - G.LEFT_OUT
    for form in names - G.LEFT_OUT:      # each form has an exact and a random cell, in both operand types where it has both
        mine = [c for c in G.CELLS if c.form == form]
        assert {c.exact for c in mine} == {True, False}, form
        assert {c.dt for c in mine} == ({G.F16} if form == "p8" else {G.F16, G.BF16}), form
    assert all(c.p8 == 1 or c.form == "p8" for c in G.CELLS)


def test_approximation_allowances_are_the_measured_gaps():
    gelu, grad = G.approx_gap()
    print("gelu_fast gap %.3e, gelu_grad_fast gap %.3e" % (gelu, grad))
    assert gelu <= G.GELU_GAP <= 1.25 * gelu and grad <= G.GELU_GRAD_GAP <= 1.25 * grad


@pytest.mark.parametrize("cell", [c for c in ALL if c.exact], ids=lambda c: c.name)
def test_exact_cells_are_exact_in_float32(cell):
    o = G.operands(cell)
    r64, r32 = G.evaluate(cell, o), G.evaluate(cell, o, torch.float32)
    ref = r64["out"]
    assert torch.equal(r32["out"].double(), ref) and torch.equal(ref.float().double(), ref)
    assert torch.equal(ref * 2, (ref * 2).round()), "not a multiple of 0.5"
    for name in ("A", "B", "A_lo", "B_lo"):      # the operands are values of the 16-bit type
        assert torch.equal(o[name].to(cell.dt).float(), o[name])
    amax = float(ref.abs().max())
    assert amax < 60000, amax
    # every partial sum, in any order, is an integer below 2^24, and the epilogue's (acc + biases) * scale + res a multiple of
    # 0.5 below 2^23: even the sum of the |terms| is
    width = max(float(o[n].abs().max()) for n in ("A", "B", "A_lo", "B_lo"))
    parts = 1 + ("A_lo" in cell.has) + ("B_lo" in cell.has)
    assert 4 * (parts * cell.K * width * width + 40) + 100 < 2 ** 23
    e = G.expectations(cell)
    if not cell.out_f32:
        share = float((ref.abs() > G.UNREP[cell.dt]).double().mean())
        rounded = float((e["out"].exact.double() != ref).double().mean())
        print(cell.name, "max |ref| %.0f, above the exact range %.2f, changed by the rounding %.2f" % (amax, share, rounded))
        assert share >= 0.25 and rounded > 0.05
    if "out_lo" in e:      # the plane pair holds the value exactly
        assert torch.equal(e["out"].exact.double() + e["out_lo"].exact.double(), ref)
    if "rowstats" in e:
        G.check(cell, "rowstats", r32["rowstats"], e["rowstats"])


@pytest.mark.parametrize("cell", [c for c in ALL if not c.exact], ids=lambda c: c.name)
def test_random_cells_hold_their_own_bound_in_float32(cell):
    o = G.operands(cell)
    r32 = G.evaluate(cell, o, torch.float32)
    e = G.expectations(cell)
    out = r32["out"]
    if "C_lo" in cell.has:
        hi = out.to(cell.dt)
        out = hi.double() + (out - hi.float()).to(cell.dt).double()
    elif not cell.out_f32:
        out = out.to(cell.dt)
    G.check(cell, "out", out, e["out"])
    if "stats" in e:
        G.check(cell, "stats", G.stats_table(cell, r32["stats"]), e["stats"])
    if "rowstats" in e:
        G.check(cell, "rowstats", r32["rowstats"], e["rowstats"])
    if cell.act in (_lib.ACT_GELU, _lib.ACT_GELU_GRAD):      # ... and with the kernel's approximation in place of the function
        fast = G.evaluate(cell, o, torch.float32, mutate=dict(fast=True))["out"]
        assert not torch.equal(fast, r32["out"])
        G.check(cell, "out", fast if cell.out_f32 else fast.to(cell.dt), e["out"])


# ---- the checker against realistic mistakes -------------------------------------------------------------------------------
def _cell(name):
    return G.BY_NAME[name]


def _fails(cell, what, got, match):
    with pytest.raises(AssertionError, match=match) as info:
        G.check(cell, what, got, G.expectations(cell)[what])
    print(info.value)
    return str(info.value)


def _as_out(cell, v):
    return v.float() if cell.out_f32 else v.float().to(cell.dt)


DENSE_TARGETS = ["big_256x128_m16-300x136x96-full-f32-f16", "big_256x128_m16-300x136x96-full-16-bf16", "ph8_m16-300x264x2048-bias-16-f16",
                 "ph8_m16-300x264x2048-bias-gelu-16-bf16", "generic-300x136x72-full-gelu-16-f16", "big_256x128_split-300x136x64-a_lo-b_lo-bias-f32-f16",
                 "big_256x128_m16-300x136x96-plain-f32-random-f16", "p8-769x1032x128-plain-16-random-f16"]


@pytest.mark.parametrize("name", DENSE_TARGETS)
def test_checker_catches_dense_mistakes(name):
    cell = _cell(name)
    o = G.operands(cell)
    good = G.evaluate(cell, o)["out"]
    G.check(cell, "out", _as_out(cell, good), G.expectations(cell)["out"])
    tm, tn = G.TILE[cell.form]
    # one 8-wide K chunk dropped from one row (row 37 of the second row tile)
    row = min(tm + 37, cell.M - 1)
    a = dict(o, A=o["A"].clone())
    a["A"][row, 8:16] = 0
    msg = _fails(cell, "out", _as_out(cell, G.evaluate(cell, a)["out"]), r"\(row, col\) = \(%d, " % row)
    assert "row %d col" % (row % tm) in msg
    # two rows swapped inside one 32-row fragment
    sw = good.clone()
    sw[:, [tm + 3, tm + 20]] = sw[:, [tm + 20, tm + 3]]
    _fails(cell, "out", _as_out(cell, sw), r"tile \(1, ")
    if "bias_n" in cell.has:
        # bias_n shifted by one column inside the last 4-column group of the ragged last tile
        b = dict(o, bias_n=o["bias_n"].clone())
        b["bias_n"][-4:] = o["bias_n"][-4:].roll(1)
        _fails(cell, "out", _as_out(cell, G.evaluate(cell, b)["out"]), r"tile \(\d, %d\)" % ((cell.n_out - 1) // tn))
        # bias_n added three times (once per K part)
        _fails(cell, "out", _as_out(cell, G.evaluate(cell, o, mutate=dict(bias_times=3))["out"]), "elements wrong")


def test_checker_catches_a_written_pad_column_and_row():
    cell = _cell("big_256x128_m16-300x136x96-full-16-f16")
    flat, view = G.out_buffer(cell, "cpu")
    view.copy_(G.expectations(cell)["out"].exact[0])
    G.check_pad(cell, "out", flat, view)
    G.check(cell, "out", view[None], G.expectations(cell)["out"])
    flat2 = flat.clone()
    v2 = torch.as_strided(flat2, (cell.M, cell.N + 1), view.stride())
    v2[17, cell.N] = 1.0                                   # one pad column of one row
    with pytest.raises(AssertionError, match=r"1 pad elements written; first at flat offset \d+ \(row 17, column 136"):
        G.check_pad(cell, "out", flat2, torch.as_strided(flat2, view.shape, view.stride()))
    flat3 = flat.clone()
    flat3[cell.M * (cell.N + 8) + 5] = 0.0                 # the pad row
    with pytest.raises(AssertionError, match="row 300, column 5"):
        G.check_pad(cell, "out", flat3, torch.as_strided(flat3, view.shape, view.stride()))
    # batched, with a batch stride that is no multiple of the row: the mask follows the strides
    cell = _cell("ph8_m16-300x264x2048-batch3-bias_m-16-stride4-f16")
    flat, view = G.out_buffer(cell, "cpu")
    assert view.stride() == (301 * 272 + 4, 272, 1) and view.shape == (3, 300, 264)
    view.fill_(1.0)
    G.check_pad(cell, "out", flat, view)
    flat[301 * 272 + 2] = 1.0                              # between batch entries 0 and 1
    with pytest.raises(AssertionError, match="pad elements written"):
        G.check_pad(cell, "out", flat, view)


@pytest.mark.parametrize("name", ["conv_256x128-136-bias-stats-f16", "conv_512x64_split-40-cin64-b2-bias-stats-bf16", "generic-255x300x128-stats-f32-f16",
                                  "generic_conv-136-cin8-b2-bias-stats-f16"])
def test_checker_catches_stats_mistakes(name):
    cell = _cell(name)
    e = G.expectations(cell)["stats"]
    rb = G.TILE[cell.form][0] // 128
    assert e.ref.shape == (ops.gemm_tiles_m(cell.M), 2, cell.N)
    good = e.ref.float()
    G.check(cell, "stats", good, e)
    unwritten = good.clone()
    unwritten[rb if cell.M > G.TILE[cell.form][0] else 0] = G.SENTINEL              # a row of sums left unwritten
    _fails(cell, "stats", unwritten, "stats row %d" % (rb if cell.M > G.TILE[cell.form][0] else 0))
    if rb > 1:
        unzeroed = good.clone()
        unzeroed[1] = G.SENTINEL                                                    # a covered row not zeroed
        _fails(cell, "stats", unzeroed, "stats row 1")
        per128 = torch.zeros_like(good)                                             # sums per 128 rows instead of per tile
        v = G.evaluate(cell, G.operands(cell))["out"][0]
        for r in range(per128.shape[0]):
            per128[r, 0], per128[r, 1] = v[128 * r:128 * r + 128].sum(0), (v[128 * r:128 * r + 128] ** 2).sum(0)
        _fails(cell, "stats", per128, "stats row")
    # the column totals are right and one tile's share moved to the next: still caught
    if good.shape[0] > rb:
        moved = good.clone()
        moved[0, 0, 5] += 1.0
        moved[rb, 0, 5] -= 1.0
        _fails(cell, "stats", moved, "column 5")


@pytest.mark.parametrize("name", ["conv_256x128-136-bias-f16", "conv_ph8_split-256-bias-bf16", "conv_256x64-40-bias-stats-f16",
                                  "generic_conv-136-cin8-b2-bias-f16"])
def test_checker_catches_convolution_mistakes(name):
    cell = _cell(name)
    o = G.operands(cell)
    G.check(cell, "out", _as_out(cell, G.evaluate(cell, o)["out"]), G.expectations(cell)["out"])
    # a replicated border instead of a zero border: interior pixels agree, the worst element is on the border
    msg = _fails(cell, "out", _as_out(cell, G.evaluate(cell, o, mutate=dict(border="replicate"))["out"]), r"\(b, oh, ow, cout\)")
    b, oh, ow, _ = (int(s) for s in msg.split("(b, oh, ow, cout) = (")[1].split(")")[0].split(","))
    assert oh in (0, 12) or ow in (0, 11), msg
    bad = int(msg.split(": ")[1].split(" of ")[0])
    assert bad <= 2 * (13 * 12 - 11 * 10) * cell.N           # only border pixels
    # kh and kw exchanged
    _fails(cell, "out", _as_out(cell, G.evaluate(cell, o, mutate=dict(swap=True))["out"]), "elements wrong")
    # the bias of a K-split launch added by every part
    _fails(cell, "out", _as_out(cell, G.evaluate(cell, o, mutate=dict(bias_times=3))["out"]), "elements wrong")


def test_checker_catches_rowstats_and_plane_mistakes():
    cell = _cell("ph8_ln-300x320x2048-planes-rowstats-f16")
    e = G.expectations(cell)
    good = G.evaluate(cell, G.operands(cell), torch.float32)["rowstats"]
    G.check(cell, "rowstats", good, e["rowstats"])
    bad = good.clone()
    bad[299, 4] = bad[299, 3]                                # the last group of the last row holds its neighbour's sums
    _fails(cell, "rowstats", bad, "row 299, 64-column group 4")
    lo = e["out_lo"].exact.clone()
    lo[0, 100, 8:16] = 0                                     # one 8-column store vector of the lo plane missing
    msg = _fails(cell, "out_lo", lo, r"\(row, col\) = \(100, ")
    assert int(msg.split(": ")[1].split(" of ")[0]) <= 8


def test_guards_and_views():
    cell = _cell("ph8_m16-300x264x2048-batch3-bias_m-16-f16")
    o = G.operands(cell)
    flat, b = G.guarded(o["B"], cell.dt, "cpu")
    assert b.shape == (3, 264, 2048) and b.stride() == (265 * 2056, 2056, 1) and torch.equal(b.float(), o["B"])
    assert int(flat.isnan().sum()) == flat.numel() - b.numel()
    flat, r = G.guarded(o["res"], torch.float32, "cpu", off=2)
    assert r.storage_offset() == 2 and r.stride() == (272, 1) and torch.equal(r, o["res"])
    v = G.guarded_vec(o["bias_n"], "cpu", off=1)
    assert v.is_contiguous() and v.storage_offset() == 1 and torch.equal(v, o["bias_n"])
    relu = _cell("generic-300x136x72-full-relu-16-f16")      # ReLU sits before scale_n and res: only res goes below zero
    assert relu.act == ACT_RELU and float(G.expectations(relu)["out"].ref.min()) >= -50.0
