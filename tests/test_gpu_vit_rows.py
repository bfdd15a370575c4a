"""The HBM-bound row kernels of the trainable ViT (csrc/norm.hip, csrc/vit_bwd.hip, csrc/row_routines.h), each against the plain
float64 reference of tests/vit_rows_ref.py, at the shapes of its case tables: every shape is there for a branch of the host
dispatch or of a kernel loop, and tests/test_vit_rows_ref_cpu.py asserts on the CPU that it reaches it.

Row strides: wherever an entry point takes one, at least one case per kernel passes a column slice of a wider buffer; operand
padding is NaN, output padding a sentinel that must be unchanged.

Bounds (tests/bound_helpers.py; none is taken from what the kernels return):
  fp32 outputs   err <= max(4 Y, U ulp32 max|ref|), Y = the error of torch's own float32 evaluation of the operation on the CPU
                 against float64; U = 4 element-wise, 16 for sums over rows or over K (test_gpu_bn_bwd.py derives 16 for serial
                 chains up to 256 terms; the longest chain here is 33 rows a thread or wave).
  16-bit outputs |out - ref| <= h |ref| + s + (fp32 bound): h = half an ulp of the type, of the pair for hi + lo; s = half a
                 subnormal fp16 ulp.
  per binade     GELU and SwiGLU sweep many binades: Y and max|ref| are taken over the elements whose INPUT shares
                 floor(log2 |x|), so that a large value elsewhere does not loosen the bound on a small one.
  GELU forward   fp32 term 5.5e-7 absolute: the 5.1e-7 the comment in csrc/asis_common.h claims for |x| <= 12 and the fp16 values,
                 plus 4e-8 for a hardware exp2 one ulp off the evaluation used in the fit (one ulp32 of a q <= 0.17 is 2e-8, doubled).
  GELU backward  libm erff and __expf: the Y scheme per binade.
  SwiGLU         fp32 term max(4 Y, 2^-17 |ref|): __expf(x) = exp2(x log2e) with an fp32 product has a relative error
                 <= |x| 2^-24 + 2^-23 < 2^-19 at |x| <= 32, and enters sigma and sigma' at most four times.
  bit-exact      hi planes, packing, cls / pos add, dW and db of the finish (single fp32 products), determinism, the 2^-17
                 weight scaling of the LayerNorm backward: ``torch.equal``.
Not covered: the second grid-stride trip of asis_gelu16 / asis_gelu_split / asis_swiglu_bwd needs about 5e8 elements; GELU beyond
|x| = 65504 (bf16 / fp32 only; from |x| ~ 4e5 the clamp at 7 shows, see csrc/asis_common.h).

Measured on one MI355X, the case with the largest err / bound per output (all cases: run with ``-s``, every check prints a
MEASURE line before it asserts):

    output              worst case                                err        Y (float32)  bound      err / bound
    layernorm           1x2048 ld None f32                        6.425e-06  2.027e-06    8.107e-06  0.79
    layernorm16         4097x1024 ld None bf16                    1.562e-02  1.294e-05    1.574e-02  0.99
    split_stats.hi+lo   130x64 ld 72 bf16                         6.104e-05  0.000e+00    2.447e-04  0.25
    split_stats.mean    130x260 ld 268 f16                        1.506e-06  1.337e-06    5.348e-06  0.28
    split_stats.rstd    130x64 ld 72 f16                          6.670e-07  4.713e-07    2.529e-06  0.26
    ln_bwd.dx           4x1536 maxc 6 res 0 strided 0             5.891e-07  3.465e-07    1.606e-06  0.37
    ln_bwd.dweight      31x4 maxc 4 res 1 strided 0               9.500e-07  4.806e-07    1.221e-05  0.08
    ln_bwd.dbias        130x2048 maxc 8 res 1 strided 0           4.214e-06  8.028e-06    7.228e-05  0.06
    gelu16.fwd          63488 values f16                          6.039e-05  0.000e+00    6.170e-05  0.98
    gelu16.bwd.ones     63488 values f16                          4.874e-04  2.654e-07    4.890e-04  1.00
    gelu16.bwd.random   36608 values bf16                         3.894e-03  8.302e-07    3.923e-03  0.99
    gelu_split.hi+lo    1112064 points f16                        7.573e-07  0.000e+00    2.505e-06  0.30
    swiglu_bwd          257x4096 bf16                             1.562e-02  8.703e-06    1.572e-02  0.99
    colsum              33x2056 ld 2056 f32                       3.979e-06  3.964e-06    5.808e-05  0.07
    ls_finish.dgamma    3x1024 nocs                               1.381e-07  4.803e-08    1.277e-06  0.11

For a 16-bit output err and bound are those of the element with the largest err / bound: there the rounding of the type is nearly
the whole of both, so a ratio just under 1 is what a correct kernel gives (Y column: the float32 yardstick of the case; 0 where the
fp32 term is the fixed GELU figure or absent).  GELU: |hi + lo - gelu| over the 2^20-point grid and the fp16 values is at most
9.54e-07 (fp16 pair; it exceeds the pair's own rounding by 5.2e-08 at the most, 8.5e-08 for bf16), against the 5.1e-7 of the
header and the 5.5e-7 allowed here: no 16-bit pair resolves the claim near x = 4, where the pair itself rounds by up to 9.5e-7;
on x <= 0, where |gelu| <= 0.17 and the fp16 pair rounds by 8e-8 at the most, the maximum is 1.08e-07.  Decoded MX planes: at most 2.73e-2 (hi8) and 2.89e-2
(lo8) rel-L2 from the 16-bit planes.
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from adaptersis_amd import ops
from tests import vit_rows_ref as R
from tests.bound_helpers import DT, HALF, PAIR, SUBN, ULP32, U_ELEM, U_SUM, _bound, _err, _gen
from tests.conftest import rel_l2
from tests.mx_helpers import decode

gpu = pytest.mark.gpu
EPS = R.EPS
F32 = torch.float32
SENT = 768.0            # exact in fp16, bf16 and fp32
NAN = float("nan")
GELU_F32_TERM = 5.5e-7
NAME = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32"}


def _report(name, case, err, bound, yard):
    print(f"MEASURE {name} {case}: err {err:.3e} yard {yard:.3e} bound {bound:.3e} ratio {err / bound:.3f}")


def _wide(t, ld, dev, fill=NAN):
    """t [rows, D] on the device; with ``ld`` as a column slice of a [rows, ld] buffer whose padding holds ``fill``"""
    if not ld:
        return t.to(dev)
    big = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=dev)
    big[:, :t.shape[1]] = t.to(dev)
    return big[:, :t.shape[1]]


def _sentinel_out(rows, D, ld, dtype, dev):
    big = torch.full((rows, ld), SENT, dtype=dtype, device=dev)
    return big, big[:, :D]


def _pad_untouched(big, D):
    return bool((big[:, D:] == SENT).all())


def _check32(name, case, got, ref, f32, ulps):
    bound, yard = _bound(f32, ref, ulps)
    err = _err(got, ref)
    _report(name, case, err, bound, yard)
    assert err <= bound, (name, case, err, bound, yard)


def _check16(name, case, got, ref, fb, yard, dt, pair=False):
    """element by element: |got - ref| <= h |ref| + s + fb; fb a number or a tensor like ref"""
    lim = (PAIR if pair else HALF)[dt] * ref.abs() + SUBN[dt] + fb
    d = (got.detach().double().cpu() - ref).abs()
    assert bool(torch.isfinite(d).all()), (name, case)
    ratio = (d / lim).reshape(-1)
    k = int(ratio.argmax())
    print(f"MEASURE {name} {case}: err {float(d.reshape(-1)[k]):.3e} yard {float(yard):.3e} bound {float(lim.reshape(-1)[k]):.3e} "
          f"ratio {float(ratio[k]):.3f}")
    assert float(ratio[k]) <= 1.0, (name, case, float(d.reshape(-1)[k]), float(lim.reshape(-1)[k]))


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---- 1. LayerNorm forward -----------------------------------------------------------------------------------------------------
def _ln_forward_case(dev, rows, D, ld, dt):
    x, w, b, y64, y32, *_ = R.ln_fwd_case(rows, D)
    xd, wd, bd = _wide(x, ld, dev), w.to(dev), b.to(dev)
    if ld:
        big, out = _sentinel_out(rows, D, ld, dt, dev)
        ops.layernorm(xd, wd, bd, EPS, out=out)
        assert _pad_untouched(big, D), (rows, D, ld)
    else:
        out = ops.layernorm(xd, wd, bd, EPS, dt)
    assert out.dtype == dt
    case = f"{rows}x{D} ld {ld} {NAME[dt]}"
    if dt == F32:
        _check32("layernorm", case, out, y64, y32, U_ELEM)
    else:
        fb, yard = _bound(y32, y64, U_ELEM)
        _check16("layernorm16", case, out, y64, fb, yard, dt)
    return out


@gpu
@pytest.mark.parametrize("dt", [F32] + DT, ids=lambda d: NAME[d])
def test_layernorm_generic(dev, dt):
    """layernorm_kernel: 63 / 64 / 65 float4 chunks against 64 lanes, the widest D, partial and full blocks of four rows"""
    for rows, D, ld in R.LN_GENERIC:
        _ln_forward_case(dev, rows, D, ld, dt)


def _ln_fixed_cases(dev):
    for rows, D, ld, *_ in R.LN_FIXED:
        for dt in DT:
            _ln_forward_case(dev, rows, D, ld, dt)


@gpu
@pytest.mark.parametrize("case", R.LN_FIXED, ids=lambda c: f"{c[0]}x{c[1]}")
def test_layernorm_fixed(dev, case):
    """layernorm_fixed_kernel (default form: two rows a wave): even, odd (the clamped second row of the last wave is not stored)
    and partial-last-block row counts; 4095 rows take the generic kernel on the same input.  The float32 output of the same
    shape stays on the generic kernel."""
    rows, D, ld = case[:3]
    for dt in DT:
        _ln_forward_case(dev, rows, D, ld, dt)
    if rows == 4097:
        _ln_forward_case(dev, rows, D, ld, F32)


@gpu
@pytest.mark.parametrize("form", ["0", "1"])
def test_layernorm_fixed_forms(dev, form):
    """ASIS_LN_FAST = 0 (always the generic kernel) and 1 (fixed kernel, one row a wave) on the same cases, one child process
    each: the switch is read once"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_vit_rows"], cwd=root, env={**os.environ, "ASIS_LN_FAST": form},
                       capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-1000:]
    assert f"fixed cases ok form {form}" in r.stdout and r.stdout.count("MEASURE layernorm16") == 2 * len(R.LN_FIXED)


# ---- 2. split_stats, layernorm_mx ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", R.STATS_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_split_stats_and_layernorm_mx(dev, case):
    rows, D, ld = case
    x, w, b, y64, y32, mean64, rstd64, mean32, rstd32 = R.ln_fwd_case(rows, D)
    xd, wd, bd = _wide(x, ld, dev), w.to(dev), b.to(dev)
    for dt in DT:
        tag = f"{rows}x{D} ld {ld} {NAME[dt]}"
        hi, lo, mr = ops.split_stats(xd, dt, EPS)
        assert torch.equal(_bits(hi), _bits(x.to(dt)))
        _check16("split_stats.hi+lo", tag, hi.double() + lo.double(), x.double(), 0.0, 0.0, dt, pair=True)
        _check32("split_stats.mean", tag, mr[:, 0], mean64, mean32, U_ELEM)
        _check32("split_stats.rstd", tag, mr[:, 1], rstd64, rstd32, U_ELEM)
        amax = ((D - 1) ** 0.5 * w.abs().max() + b.abs().max()).reshape(1).to(dev)        # a loose bound of |y|
        assert float(amax) > float(y64.abs().max())
        y16, mx = ops.layernorm_mx(xd, wd, bd, EPS, dt, amax)
        assert torch.equal(_bits(y16), _bits(ops.layernorm(xd, wd, bd, EPS, dt)))
        dh, dl = decode(mx.cpu(), float(amax), dt, False)
        e_hi, e_lo = rel_l2(dh, y16.float()), rel_l2(dl, y64 - y16.double().cpu())
        print(f"MEASURE layernorm_mx {tag}: rel-L2 hi8 {e_hi:.3e} (0.04) lo8 {e_lo:.3e} (0.06)")
        assert e_hi < 0.04 and e_lo < 0.06


# ---- 3. LayerNorm backward ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", R.LN_BWD, ids=lambda c: f"{c[0]}x{c[1]}")
def test_layernorm_bwd(dev, case):
    """dx element by element, dweight / dbias from reduce_rows(partial), with and without the residual; the run is
    deterministic, and with res = None scaling w by 2^-17 scales dx exactly and leaves the partial sums alone (_nw_pow2)"""
    rows, D, strided, maxc, nblk, rpb, waves, empty = case
    dy, x, w, res, refs = R.ln_bwd_case(rows, D)
    lds = (D + 4, D + 8, D + 12, D + 4) if strided else (0, 0, 0, 0)
    dyd, xd, resd, wd = _wide(dy, lds[0], dev), _wide(x, lds[1], dev), _wide(res, lds[2], dev), w.to(dev)
    for with_res in (True, False):
        tag = f"{rows}x{D} maxc {maxc} res {int(with_res)} strided {int(strided)}"

        def run(wv):
            big, out = _sentinel_out(rows, D, lds[3], F32, dev) if strided else (None, None)
            dx, partial = ops.layernorm_bwd(dyd, xd, wv, EPS, res=resd if with_res else None, out=out)
            assert big is None or (_pad_untouched(big, D) and dx.data_ptr() == big.data_ptr())
            return dx, partial

        dx, partial = run(wd)
        assert partial.shape == (nblk, 2, D)
        if empty is not None:
            assert not bool(partial[empty:].any())
        red = ops.reduce_rows(partial.view(nblk, -1)).view(2, D)
        (dx64, dw64, db64), (dx32, dw32, db32) = refs[with_res]
        _check32("ln_bwd.dx", tag, dx, dx64, dx32, U_ELEM)
        _check32("ln_bwd.dweight", tag, red[0], dw64, dw32, U_SUM)
        _check32("ln_bwd.dbias", tag, red[1], db64, db32, U_SUM)
        dx2, partial2 = run(wd)
        assert torch.equal(dx, dx2) and torch.equal(partial, partial2)
        if not with_res:
            dxs, partials = run(wd * 2.0 ** -17)
            assert torch.equal(dxs, dx * 2.0 ** -17) and torch.equal(partials, partial)


# ---- 4. GELU ------------------------------------------------------------------------------------------------------------------
def _gelu_grad_f32(pre, dpost):
    xx = pre.float().clone().requires_grad_()
    F.gelu(xx).backward(dpost.float())
    return xx.grad


@gpu
@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_gelu16_every_value(dev, dt):
    """asis_gelu16 on every finite value of the type up to 65504: forward against the claimed polynomial error, backward
    (dpost = 1 and random) by the Y scheme per binade; n = 8 and n = 8 * 256 + 8 (a second block of one thread)"""
    pre = R.all_values(dt)
    pred = pre.to(dev)
    out = ops.gelu16(pred)
    ref = R.gelu(pre)
    _check16("gelu16.fwd", f"{len(pre)} values {NAME[dt]}", out, ref, GELU_F32_TERM, 0.0, dt)
    gen = _gen(41, len(pre))
    for kind, dpost in (("ones", torch.ones(len(pre)).to(dt)), ("random", (torch.randn(len(pre), generator=gen) * 1.5).to(dt))):
        gref = R.gelu_grad(pre) * dpost.double()
        g32 = _gelu_grad_f32(pre, dpost)
        yb = R.per_binade_max(pre, (g32.double() - gref).abs())
        fb = torch.maximum(4 * yb, U_ELEM * ULP32 * R.per_binade_max(pre, gref.abs()))
        got = ops.gelu16(pred, dpost.to(dev))
        _check16(f"gelu16.bwd.{kind}", f"{len(pre)} values {NAME[dt]}", got, gref, fb, float(yb.max()), dt)
        for n in (8, 8 * 256 + 8):
            idx = torch.arange(n) * (len(pre) // n)
            sub = ops.gelu16(pred[idx.to(dev)].contiguous(), dpost[idx].contiguous().to(dev))
            assert torch.equal(_bits(sub), _bits(got.cpu()[idx])), n
    for n in (8, 8 * 256 + 8):
        idx = torch.arange(n) * (len(pre) // n)
        assert torch.equal(_bits(ops.gelu16(pred[idx.to(dev)].contiguous())), _bits(out.cpu()[idx])), n


@gpu
@pytest.mark.parametrize("dt", DT, ids=lambda d: NAME[d])
def test_gelu_split_grid(dev, dt):
    """asis_gelu_split on 2^20 fp32 points of [-12, 12] and the fp16 values: hi + lo by the pair bound around the claimed
    polynomial error, hi the rounding of hi + lo; split=False gives the same hi and no lo"""
    x = R.gelu_grid()
    xd = x.to(dev)
    ref = R.gelu(x)
    hi, lo = ops.gelu_split(xd, dt, True)
    s = hi.double().cpu() + lo.double().cpu()
    _check16("gelu_split.hi+lo", f"{len(x)} points {NAME[dt]}", s, ref, GELU_F32_TERM, 0.0, dt, pair=True)
    # hi is the 16-bit rounding of the value hi + lo.  Where lo itself was rounded up to exactly half an ulp of hi (a subnormal
    # lo, thousands of grid points) hi + lo is a tie between hi and its neighbour: there hi is one of the two nearest values
    near = R.round_to(s, dt)
    assert bool(((hi.double().cpu() - s).abs() <= (near - s).abs()).all())
    assert float((near == hi.double().cpu()).double().mean()) > 0.99
    d = (s - ref).abs()
    low = float((d - PAIR[dt] * ref.abs() - SUBN[dt]).max())
    neg = float(d[x <= 0].max())         # |gelu| <= 0.17 there: the pair rounds by at most 8e-8 (fp16), and the fit's own error shows
    print(f"MEASURE gelu.fp32side {NAME[dt]}: max |hi + lo - gelu| {float(d.max()):.3e}, on x <= 0 {neg:.3e}, less the pair "
          f"rounding {low:.3e} (claimed 5.1e-7, allowed {GELU_F32_TERM:.1e})")
    hi1, lo1 = ops.gelu_split(xd, dt, False)
    assert lo1 is None and torch.equal(_bits(hi1), _bits(hi))
    for n in (8, 8 * 256 + 8):
        idx = torch.arange(n) * (len(x) // n)
        h, l = ops.gelu_split(xd[idx.to(dev)].contiguous(), dt, True)
        assert torch.equal(_bits(h), _bits(hi.cpu()[idx])) and torch.equal(_bits(l), _bits(lo.cpu()[idx])), n


# ---- 5. SwiGLU backward -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", R.SWIGLU_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_swiglu_bwd(dev, case):
    rows, Hd = case
    x12, dhs = R.swiglu_case(rows, Hd)
    x12d = x12.to(dev)
    key = torch.cat([x12[:, :Hd], x12[:, :Hd]], 1)          # both halves depend on x1 through the exponential
    for dt in DT:
        dh = dhs[dt]
        out = ops.swiglu_bwd(x12d, dh.to(dev))
        assert out.shape == (rows, 2 * Hd) and out.dtype == dt
        ref = R.swiglu_bwd(x12, dh)
        yb = R.per_binade_max(key, (R.swiglu_f32(x12, dh).double() - ref).abs())
        fb = torch.maximum(4 * yb, 2.0 ** -17 * ref.abs())
        _check16("swiglu_bwd", f"{rows}x{Hd} {NAME[dt]}", out, ref, fb, float(yb.max()), dt)
        ext = [0, Hd - 1, Hd, 2 * Hd - 1]                   # x1 = -100 | +100: 0 | dh x2, and 0 | dh x1
        got = out.cpu()[:, ext].float()
        assert bool(torch.isfinite(got).all()) and bool((got == ref[:, ext].to(dt).float()).all())
        assert bool((got[:, [0, 2]] == 0).all())


# ---- 6. column sums -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dt", DT + [F32], ids=lambda d: NAME[d])
@pytest.mark.parametrize("case", R.COLSUM_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_colsum(dev, case, dt):
    rows, C16, C32, pad, nblk, rpb, unrolled, tail, gy16, gy32, trips = case
    C = C32 if dt == F32 else C16
    x = R.colsum_input(rows, C, dt)
    xd = _wide(x, C + pad if pad else 0, dev)
    partial = ops.colsum(xd)
    assert partial.shape == (nblk, C)
    first_empty = R.rowblock(rows)[2]
    if first_empty is not None:
        assert not bool(partial[first_empty:].any())
    _check32("colsum", f"{rows}x{C} ld {C + pad} {NAME[dt]}", ops.reduce_rows(partial), R.colsum(x), x.float().sum(0), U_SUM)
    assert torch.equal(partial, ops.colsum(xd))


# ---- 7. LayerScale o Linear finish --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", R.LS_CASES, ids=lambda c: f"{c[0]}x{c[1]}-{c[3]}")
def test_ls_linear_finish(dev, case):
    N, K, trips, what = case
    t = R.ls_case(N, K, what)
    G, W, bias, gamma, cs, gs = (t[k] for k in ("G", "W", "bias", "gamma", "cs", "gs"))
    on = lambda v: None if v is None else v.to(dev)
    dW = torch.full((N, K), SENT, device=dev)
    db = None if what == "nodb" else torch.full((N,), SENT, device=dev)
    dgamma = None if what == "nodgamma" else torch.full((N,), SENT, device=dev)
    plain = gamma is None
    ops.ls_linear_finish(on(G), None if plain else on(W), None if plain else on(bias), on(gamma), on(cs), gs, dW, db, dgamma)
    sc = torch.tensor(gs, dtype=F32) * (gamma if not plain else torch.ones(N))          # one fp32 product
    assert torch.equal(dW.cpu(), G * sc[:, None])
    if db is not None:
        assert torch.equal(db.cpu(), sc * (cs if cs is not None else torch.zeros(N)))
    if plain:
        assert bool((dgamma == SENT).all())                  # untouched
    elif dgamma is not None:
        ref = R.ls_linear_finish(G, W, bias, gamma, cs, gs)[2]
        _check32("ls_finish.dgamma", f"{N}x{K} {what}", dgamma, ref, R.ls_f32(t), U_SUM)


# ---- 8. packing ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case", R.CAST_PAD_CASES, ids=lambda c: f"{c[0]}x{c[1]}-ld{c[2]}-part{c[5]}")
def test_cast_pad(dev, case):
    rows, cols, ld_dst, ld_src, scale, part, over = case
    src = torch.randn(rows, cols, generator=_gen(51, rows, cols)) * 3
    srcd = _wide(src, ld_src if ld_src > cols else 0, dev)
    v = src * torch.tensor(scale, dtype=F32)
    for dt in DT:
        out = ops.cast_pad(srcd, ld_dst, dt, scale, part)
        assert out.shape == (rows, ld_dst) and out.dtype == dt
        assert torch.equal(_bits(out[:, :cols]), _bits(R.split(v, dt)[part]))
        assert not bool(_bits(out[:, cols:]).any())
    if ld_dst == -(-cols // 8) * 8:
        assert torch.equal(_bits(ops.cast_pad(srcd, None, DT[0], scale, part)), _bits(ops.cast_pad(srcd, ld_dst, DT[0], scale, part)))


@gpu
@pytest.mark.parametrize("case", R.IM2COL_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}-P{c[3]}-ld{c[4]}")
def test_im2col_patch(dev, case):
    B, H, W, P, ldk, over = case
    img = torch.randn(B, 3, H, W, generator=_gen(52, B, H, W, P))
    imgd = img.to(dev)
    ref = R.im2col(img, P)
    K = 3 * P * P
    for dt in DT:
        want_hi, want_lo = R.split(ref, dt)
        hi, lo = ops.im2col_patch(imgd, P, ldk, dt, split=True)
        assert hi.shape == (B * (H // P) * (W // P), ldk)
        assert torch.equal(_bits(hi[:, :K]), _bits(want_hi)) and torch.equal(_bits(lo[:, :K]), _bits(want_lo))
        assert not bool(_bits(hi[:, K:]).any()) and not bool(_bits(lo[:, K:]).any())
        assert torch.equal(_bits(ops.im2col_patch(imgd, P, ldk, dt)), _bits(hi))


@gpu
@pytest.mark.parametrize("case", R.CLS_POS_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_add_cls_pos(dev, case):
    B, N, D, over = case
    gen = _gen(53, B, N, D)
    x, cls, pos = torch.randn(B, N, D, generator=gen), torch.randn(D, generator=gen), torch.randn(N + 1, D, generator=gen)
    ref = R.add_cls_pos(x, cls, pos)
    out = ops.add_cls_pos(x.to(dev), cls.to(dev), pos.to(dev))
    assert torch.equal(out.cpu(), ref)
    buf = torch.full((B, N + 1, D), SENT, device=dev)
    assert ops.add_cls_pos(x.to(dev), cls.to(dev), pos.to(dev), out=buf) is buf and torch.equal(buf.cpu(), ref)


if __name__ == "__main__":          # the child of test_layernorm_fixed_forms: ASIS_LN_FAST is set by the parent
    _ln_fixed_cases(torch.device("cuda:0"))
    print(f"fixed cases ok form {os.environ.get('ASIS_LN_FAST')}")
