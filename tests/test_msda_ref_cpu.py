"""CPU: the float64 restatements of tests/msda_ref.py are right (they equal the oracle), their input generators keep their
guarantees on every case the GPU tests use, and the element-wise bounds of tests/test_gpu_msda_routes.py and
tests/test_gpu_dwconv_routes.py are neither vacuous nor too tight: the restatement evaluated in float32 — the reference alone, no
GPU code — stays inside every bound on every case, and three deliberately wrong restatements fall outside them on the cases
that target them."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_torch as O
from tests import msda_ref as R

F64, F32 = torch.float64, torch.float32


@functools.lru_cache(maxsize=None)
def _cases():
    return list(R.all_cases())


@functools.lru_cache(maxsize=None)
def _ref(i):
    return R.reference_of(_cases()[i])


def _oracle(case):
    B, Lq, M, Dh, P, shapes = case["B"], case["Lq"], case["M"], case["Dh"], case["P"], case["shapes"]
    L = len(shapes)
    Lin = sum(h * w for h, w in shapes)
    v = case["value"].to(F64).view(B, Lin, M, Dh).clone().requires_grad_(True)
    off = case["offaw"][:, :M * L * P * 2].to(F64).reshape(B, Lq, M, L, P, 2).clone().requires_grad_(True)
    lg = case["offaw"][:, M * L * P * 2:].to(F64).reshape(B, Lq, M, L * P).clone().requires_grad_(True)
    sp = torch.tensor(shapes)
    normalizer = torch.stack([sp[:, 1], sp[:, 0]], -1).to(F64)
    loc = case["ref"].to(F64)[None, :, None, None, None, :] + off / normalizer[None, None, None, :, None, :]
    out = O.ms_deform_attn_core(v, sp, loc, F.softmax(lg, -1).view(B, Lq, M, L, P))
    (out * case["dout"].to(F64).view(B, Lq, M * Dh)).sum().backward()
    return out.detach(), v.grad.reshape(B, Lin, M * Dh), off.grad.reshape(B * Lq, -1), lg.grad.reshape(B * Lq, -1)


@pytest.mark.parametrize("name", ["m8d32-pyr3-p4", "m4d16-1x1+2x3-p8", "sm-m2d128"])
def test_restatement_equals_the_oracle(name):
    i = next(k for k, c in enumerate(_cases()) if c["name"] == name)
    r = _ref(i)["ref"]
    out, dv, doff, dlg = _oracle(_cases()[i])
    assert float((r["out"] - out).abs().max()) <= 1e-12
    for got, want in ((r["dvalue"], dv), (r["doff"], doff), (r["dlogit"], dlg)):
        assert float((got - want).abs().max()) <= 1e-10


def test_generator_guarantees_hold_on_every_case():
    n_random = n_exact = 0
    for case in _cases() + [R.grid_stride_case()]:
        assert case["excluded"] == 0                       # (a) moves points, it never drops one
        lg = case["offaw"][:, case["M"] * len(case["shapes"]) * case["P"] * 2:]
        assert float(lg.max() - lg.min()) <= 4.0
        for k in ("value", "dout"):
            assert torch.equal(case[k].float().to(case["dtype"]).float(), case[k].float())   # 16-bit values exactly
        if case["mode"] == "random":
            assert all(w <= 128 for _, w in case["shapes"])
            assert R.boundary_distance(case) >= 2.0 ** -8, case["name"]
            n_random += 1
        else:
            assert R.fp32_positions_exact(case), case["name"]
            n_exact += 1
    assert n_random and n_exact


def test_exact_cases_reach_the_borders_the_centres_and_the_far_outside():
    for c in R.FWD_CASES:
        if c[-1] != "exact":
            continue
        case = R.fwd_case(c, torch.float16)
        B, Lq, M, P, shapes = case["B"], case["Lq"], case["M"], case["P"], case["shapes"]
        L = len(shapes)
        off = case["offaw"][:, :M * L * P * 2].reshape(B, Lq, M, L, P, 2)
        px, py = R._positions(case["ref"], off, shapes, F64)
        H, W = shapes[0]
        for p, S in ((px[:, :, :, 0], W), (py[:, :, :, 0], H)):
            have = set(p.reshape(-1).tolist())
            assert {-1.0, -0.5, 0.0, S - 1.0, S - 0.5, float(S)} <= have, (case["name"], S)
            assert any(abs(v) > 1e5 for v in have) and any(abs(v) > 2.0 ** 31 for v in have)
        centre = (px == px.round()) & (py == py.round()) & (px >= 0) & (py >= 0) & (px < 1e5) & (py < 1e5)
        assert bool(centre.any())
        # a point beyond the int range contributes exactly nothing, in the reference as in the kernel
        r = R.reference_of(case)
        wild = ((px.abs() > 1e5) | (py.abs() > 1e5)).all(-1).all(-1)          # every point of (b, q, m) far outside
        if bool(wild.any()):
            assert float(r["ref"]["out"].view(B, Lq, M, -1)[wild].abs().max()) == 0.0


def _bounds(case, r):
    dt, M, Dh, LP = case["dtype"], case["M"], case["Dh"], len(case["shapes"]) * case["P"]
    return {"out": R.tol_out(r, dt), "doff": R.tol_doff(r, Dh), "dlogit": R.tol_dlogit(r, Dh, LP),
            "dvalue": R.tol_dvalue(r, M, "scatter")}


def test_float32_restatement_stays_inside_every_bound():
    """not too tight: float32 on the CPU, out rounded to the 16-bit type, is inside the bounds on every case — and the
    split-output bound holds for the pair (hi, lo) made the way the kernel makes it"""
    top = {}
    for i, case in enumerate(_cases()):
        r, dt = _ref(i), case["dtype"]
        f = R.reference_of(case, work=F32, sums=False)["ref"]
        tol = _bounds(case, r)
        got = dict(f, out=f["out"].to(dt))
        for k in tol:
            ratio, idx = R.worst(got[k], r["ref"][k], tol[k])
            assert ratio <= 1.0, (case["name"], dt, k, ratio, idx)
            top[k] = max(top.get(k, 0.0), ratio)
        hi = f["out"].to(dt)
        lo = (f["out"] - hi.float()).to(dt)
        ratio, idx = R.worst(hi.double() + lo.double(), r["ref"]["out"], R.tol_split(r, dt))
        assert ratio <= 1.0, (case["name"], dt, "split", ratio, idx)
        top["split"] = max(top.get("split", 0.0), ratio)
    print("float32 restatement, worst |err|/bound:", {k: "%.3f" % v for k, v in top.items()})
    assert top["out"] > 0.5          # the output-rounding allowance is used: half of it would be missed


def test_bounds_without_the_position_term_are_missed_by_float32_itself():
    """why `S_pos` is in the bounds: without it the float32 restatement misses the d value and d off bounds"""
    i = next(k for k, c in enumerate(_cases()) if c["name"] == "lin-129x64" and c["dtype"] == torch.float16)
    case, r = _cases()[i], _ref(i)
    f = R.reference_of(case, work=F32, sums=False)["ref"]
    bare = dict(r, pos={k: torch.zeros_like(v) for k, v in r["pos"].items()})
    assert R.worst(f["dvalue"], r["ref"]["dvalue"], R.tol_dvalue(bare, case["M"], "scatter"))[0] > 10
    assert R.worst(f["doff"], r["ref"]["doff"], R.tol_doff(bare, case["Dh"]))[0] > 1
    assert R.worst(f["dvalue"], r["ref"]["dvalue"], R.tol_dvalue(r, case["M"], "scatter"))[0] <= 1


def _targets(wrong):
    names = {"swap": [c[0] for c in R.FWD_CASES if c[-1] == "random"] + ["sm-m4d16", "lin-65x64", "red-m8d64"],
             "clamp": [c[0] for c in R.FWD_CASES if c[0] != "x-m2d128-16x16-p1"] + ["sm-m4d16", "red-m8d64"],
             "wh": ["m1d8-1x7-p1", "m2d24-5x1-p1", "m4d16-1x1+2x3-p8", "x-m2d24-1x8+4x1-p8", "red-m8d64", "sm-m4d16",
                    "lin-65x64", "lin-129x64"]}[wrong]
    return [i for i, c in enumerate(_cases()) if c["name"] in names]


@pytest.mark.parametrize("wrong", ["swap", "clamp", "wh"])
def test_wrong_restatement_falls_outside_the_bounds(wrong):
    """not vacuous: a wrong corner weight, clamped instead of zeroed border taps, and a level's W taken for its H each break
    the bound of every output kind, on every case that targets them, in both 16-bit types"""
    idx = _targets(wrong)
    assert len(idx) >= 8
    for i in idx:
        case, r = _cases()[i], _ref(i)
        bad = R.reference_of(case, wrong=wrong, sums=False)["ref"]
        tol = _bounds(case, r)
        for k in ("out", "dvalue", "doff", "dlogit"):
            if k == "dlogit" and len(case["shapes"]) * case["P"] == 1:
                continue                                                    # a softmax over one point has no gradient
            got = bad[k].to(case["dtype"]) if k == "out" else bad[k]
            n_out = int(((got.double() - r["ref"][k]).abs() > tol[k]).sum())
            assert n_out > 0, (wrong, case["name"], case["dtype"], k)


# ---- DWConv + GELU ------------------------------------------------------------------------------------------------------
def _dw_all():
    return [(R.make_dwconv_case(n, B, C, g), bwd) for n, B, C, g, bwd in R.DW_CASES + [R.DW_BIG]]


def test_dwconv_restatement_equals_the_oracle():
    for name, B, C, grids, _ in (R.DW_CASES[0], R.DW_CASES[-1]):
        c = R.make_dwconv_case(name, B, C, grids)
        r = R.dwconv_reference(c["x"], c["w"], c["bias"], grids, c["dy"])["ref"]
        x, w, b = (c[k].to(F64).clone().requires_grad_(True) for k in ("x", "w", "bias"))
        y = F.gelu(O.dwconv(x, {"p.dwconv.weight": w, "p.dwconv.bias": b}, "p", grids))
        (y * c["dy"].to(F64)).sum().backward()
        assert float((r["out"] - y.detach()).abs().max()) <= 1e-12
        assert float((r["dx"] - x.grad).abs().max()) <= 1e-10
        assert float((r["dw9"] - w.grad.reshape(C, 9).t()).abs().max()) <= 1e-10
        assert float((r["dbias"] - b.grad).abs().max()) <= 1e-10


def test_dwconv_cases_cover_the_layouts():
    Cs = {c[2] for c in R.DW_CASES}
    assert Cs == {4, 12, 16, 64, 1024}
    assert any(c[2] == 1024 and c[1] * sum(a * b for a, b in c[3]) < 64 for c in R.DW_CASES)
    rows = R.DW_BIG[1] * sum(a * b for a, b in R.DW_BIG[3])
    nblk = R.dwconv_nblk(rows)
    assert rows == 65536 + 70 and nblk == 1024 and -(-rows // nblk) > 64 and -(-rows // nblk) * nblk > rows
    for name, B, C, g, _ in R.DW_CASES[:6]:
        c = R.make_dwconv_case(name, B, C, g)
        pre = R.dwconv_reference(c["x"], c["w"], c["bias"], g)["pre"]["out"]
        assert float((pre <= 3).double().mean()) > 0.9          # both sides of zero, mostly within +-3


def test_dwconv_float32_restatement_stays_inside_every_bound():
    top = {}
    for dt in R.DTYPES:
        for c, bwd in _dw_all():
            if c["C"] == 1024 and c["B"] == 3:
                continue                                       # the same arithmetic as B = 1, minutes less of CPU
            r = R.dwconv_reference(c["x"], c["w"], c["bias"], c["grids"], c["dy"])
            f = R.dwconv_reference(c["x"], c["w"], c["bias"], c["grids"], c["dy"], work=F32)["ref"]
            rows = c["B"] * c["x"].shape[1]
            checks = {"out": (f["out"].to(dt), R.tol_dw_out(r, dt)), "dx": (f["dx"].to(dt), R.tol_dw_out(r, dt, "dx")),
                      "dw9": (f["dw9"], R.tol_dw_param(r, "dw9", rows, R.dwconv_nblk(rows))),
                      "dbias": (f["dbias"], R.tol_dw_param(r, "dbias", rows, R.dwconv_nblk(rows)))}
            for k, (got, tol) in checks.items():
                ratio, idx = R.worst(got, r["ref"][k], tol)
                assert ratio <= 1.0, (c["name"], dt, k, ratio, idx)
                top[k] = max(top.get(k, 0.0), ratio)
    print("float32 DWConv restatement, worst |err|/bound:", {k: "%.3f" % v for k, v in top.items()})


def test_dwconv_wrong_tap_falls_outside_the_bounds():
    """a conv whose taps are mirrored (correlation taken for convolution) breaks the out and dx bounds"""
    for name, B, C, grids, _ in R.DW_CASES[:4]:
        c = R.make_dwconv_case(name, B, C, grids)
        r = R.dwconv_reference(c["x"], c["w"], c["bias"], grids, c["dy"])
        bad = R.dwconv_reference(c["x"], c["w"].flip(-1), c["bias"], grids, c["dy"])["ref"]
        for k in ("out", "dx"):
            tol = R.tol_dw_out(r, torch.float16, k)
            assert int(((bad[k] - r["ref"][k]).abs() > tol).sum()) > 0, (name, k)
