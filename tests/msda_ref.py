"""float64 restatements, on the CPU, of the adapter kernels: the multi-scale deformable-attention sampling core
(`csrc/msda.hip`, the MSDA half of `csrc/adapter_bwd.hip`) and the ConvFFN depthwise 3x3 conv + erf GELU, with the input
generators, the case lists and the element-wise bounds that `test_msda_ref_cpu.py` (no GPU) and `test_gpu_msda_routes.py` /
`test_gpu_dwconv_routes.py` share.

The MSDA restatement is explicit indexing (floor, four taps, zero padding by masking, softmax over L*P), no `grid_sample`.  It
takes what the kernel takes — `value` and `dout` already rounded to the 16-bit operand type, fp32 `offaw` rows, `ref`, `shapes` —
and returns, for `out`, `d value`, `d off`, `d logit`:

  ref    the float64 result (the gradients through `torch.autograd`)
  abs    `S_abs`: the same expression on |value|, |dout|, |d bilinear weight| and the softmax weights — the sum of the absolute
         values of the terms of every element, no cancellation.  d logit: A_j (T_j + sum_k A_k T_k), T_j = <|dout|, |S_j|>.
  pos    `S_pos`: the first-order effect on that element of the kernel's fp32 sampling position.  The kernel forms
         px = (rx + ox / W) * W - 0.5 in four fp32 roundings, each <= u x the magnitude it rounds, so
         |px_fp32 - px| <= dpx = 4 u (|rx| W + |ox| + 0.5), far above the u-relative error of everything else: a weight
         bx*by moves by <= dpx*by + dpy*bx, a derivative weight dbx*by by <= dpy.  `S_pos` is `S_abs` with every bilinear weight
         replaced by that move.  (The n u S_abs terms count roundings of the weight CHAIN; this is the rounding of its INPUT:
         without the term the float32 restatement itself — no GPU code — misses the d value bound by up to 360x (a single tap of weight
         2^-7 on a 129-pixel level) and the d off bound by up to 1.9x: tests/test_msda_ref_cpu.py asserts both facts.)
  count  d value only: the number of in-range taps that land on each (b, pixel, m)
"""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24          # fp32 unit roundoff
WRONG = (None, "swap", "clamp", "wh")


def eps16(dtype):
    """unit roundoff of the 16-bit type: round-to-nearest is off by at most half an ulp, which is up to 2^-11 |x| for fp16 (11
    significant bits) and 2^-8 |x| for bf16 (8) — reached just above a power of two.  This is the whole output-rounding
    allowance; half of it is a bound that a correctly rounded result misses by up to 2x."""
    return 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8


def tiny16(dtype):
    """half the spacing of fp16's subnormals (below 2^-14 its rounding error is absolute); bf16 has fp32's exponent range"""
    return 2.0 ** -25 if dtype == torch.float16 else 0.0


def starts_of(shapes):
    st, acc = [], 0
    for h, w in shapes:
        st.append(acc)
        acc += h * w
    return st


# ------------------------------------------------------------------------------------------------------------------------
# MSDA restatement
# ------------------------------------------------------------------------------------------------------------------------
def msda_reference(value, offaw, ref, shapes, M, P, dout=None, work=torch.float64, wrong=None, sums=True):
    """value [B, Lin, D]; offaw [B*Lq, >= M*L*P*3] (offsets (x, y) per (m, l, p), then logits per (m, l*p)); ref [Lq, 2];
    dout [B*Lq, D] or None.  ``work``: the dtype everything is evaluated in (float64: the reference; float32: the
    bounds' sanity check).  ``wrong``: a deliberately wrong variant — "swap": ax and ay swapped on corner (x0+1, y0);
    "clamp": out-of-range taps read the clamped pixel instead of zero; "wh": the level's W used for its H.
    Returns {"ref": {...}, "abs": {...}, "pos": {...}, "count": ...} keyed by out / dvalue / doff / dlogit."""
    assert wrong in WRONG
    B, Lin, D = value.shape
    Dh, L, LP, Lq = D // M, len(shapes), len(shapes) * P, ref.shape[0]
    assert Lin == sum(h * w for h, w in shapes) and offaw.shape[0] == B * Lq
    st = starts_of(shapes)
    grad = dout is not None
    v = value.to(work).view(B, Lin, M, Dh).clone().requires_grad_(grad)
    ow = offaw[:, :M * LP * 3].to(work)
    off = ow[:, :M * LP * 2].reshape(B, Lq, M, L, P, 2).clone().requires_grad_(grad)
    logit = ow[:, M * LP * 2:].reshape(B, Lq, M, LP).clone().requires_grad_(grad)
    A = torch.softmax(logit, -1).view(B, Lq, M, L, P)
    r = ref.to(work)
    rx, ry = r[:, 0].view(1, Lq, 1, 1), r[:, 1].view(1, Lq, 1, 1)
    bi, mi = torch.arange(B).view(B, 1, 1, 1), torch.arange(M).view(1, 1, M, 1)
    out = torch.zeros(B, Lq, M, Dh, dtype=work)
    if sums:
        d64 = torch.float64
        g = dout.to(d64).abs().view(B, Lq, M, 1, Dh) if grad else None
        s_out, p_out = torch.zeros(B, Lq, M, Dh, dtype=d64), torch.zeros(B, Lq, M, Dh, dtype=d64)
        T, Tp = torch.zeros(B, Lq, M, L, P, dtype=d64), torch.zeros(B, Lq, M, L, P, dtype=d64)
        s_off, p_off = torch.zeros(B, Lq, M, L, P, 2, dtype=d64), torch.zeros(B, Lq, M, L, P, 2, dtype=d64)
        s_dv, p_dv = torch.zeros(B * Lin * M, Dh, dtype=d64), torch.zeros(B * Lin * M, Dh, dtype=d64)
        count = torch.zeros(B * Lin * M, dtype=torch.int64)
    for l, (H, W) in enumerate(shapes):
        Hy = W if wrong == "wh" else H
        ox, oy = off[:, :, :, l, :, 0], off[:, :, :, l, :, 1]
        px = (rx + ox / W) * W - 0.5
        py = (ry + oy / Hy) * Hy - 0.5
        fx, fy = torch.floor(px.detach()), torch.floor(py.detach())
        ax, ay = px - fx, py - fy
        if sums:
            dpx = 4 * U * (rx.abs() * W + ox.detach().abs() + 0.5).to(d64)
            dpy = 4 * U * (ry.abs() * Hy + oy.detach().abs() + 0.5).to(d64)
            Al = A[:, :, :, l].detach().to(d64)
        for t in range(4):
            tx, ty = t & 1, t >> 1
            xx, yy = fx + tx, fy + ty
            inb = (xx >= 0) & (xx <= W - 1) & (yy >= 0) & (yy <= Hy - 1)
            bx, by = (ax if tx else 1 - ax), (ay if ty else 1 - ay)
            if wrong == "swap" and t == 1:
                bx, by = ay, 1 - ax
            idx = st[l] + yy.clamp(0, H - 1).long() * W + xx.clamp(0, W - 1).long()
            vt = v[bi, idx, mi]                                             # [B, Lq, M, P, Dh]
            keep = torch.ones_like(inb) if wrong == "clamp" else inb
            out = out + ((A[:, :, :, l] * bx * by * keep.to(work)).unsqueeze(-1) * vt).sum(3)
            if not sums:
                continue
            k = inb.to(d64)
            bxd, byd = bx.detach().to(d64), by.detach().to(d64)
            posw = (dpx * byd + dpy * bxd) * k
            va = vt.detach().to(d64).abs()
            s_out += ((Al * bxd * byd * k).unsqueeze(-1) * va).sum(3)
            p_out += ((Al * posw).unsqueeze(-1) * va).sum(3)
            if grad:
                gv = (g * va).sum(-1)                                      # [B, Lq, M, P]
                T[:, :, :, l] += bxd * byd * k * gv
                Tp[:, :, :, l] += posw * gv
                s_off[:, :, :, l, :, 0] += Al * byd * k * gv
                s_off[:, :, :, l, :, 1] += Al * bxd * k * gv
                p_off[:, :, :, l, :, 0] += Al * dpy * k * gv
                p_off[:, :, :, l, :, 1] += Al * dpx * k * gv
                rows = ((bi * Lin + idx) * M + mi).reshape(-1)
                s_dv.index_add_(0, rows, ((Al * bxd * byd * k).unsqueeze(-1) * g).reshape(-1, Dh))
                p_dv.index_add_(0, rows, ((Al * posw).unsqueeze(-1) * g).reshape(-1, Dh))
                count.index_add_(0, rows, inb.reshape(-1).long())
    res = {"ref": {"out": out.detach().reshape(B, Lq, D)}}
    if grad:
        (out * dout.to(work).view(B, Lq, M, Dh)).sum().backward()
        res["ref"].update(dvalue=v.grad.reshape(B, Lin, D), doff=off.grad.reshape(B * Lq, M * LP * 2),
                          dlogit=logit.grad.reshape(B * Lq, M * LP))
    if sums:
        res["abs"], res["pos"] = {"out": s_out.reshape(B, Lq, D)}, {"out": p_out.reshape(B, Lq, D)}
        if grad:
            Ad = A.detach().to(d64)
            res["abs"].update(dvalue=s_dv.view(B, Lin, D), doff=s_off.reshape(B * Lq, -1),
                              dlogit=(Ad * (T + (Ad * T).sum((3, 4), keepdim=True))).reshape(B * Lq, -1))
            res["pos"].update(dvalue=p_dv.view(B, Lin, D), doff=p_off.reshape(B * Lq, -1),
                              dlogit=(Ad * (Tp + (Ad * Tp).sum((3, 4), keepdim=True))).reshape(B * Lq, -1))
            res["count"] = count.view(B, Lin, M)
    return res


# ------------------------------------------------------------------------------------------------------------------------
# bounds (derivations: the docstring of tests/test_gpu_msda_routes.py)
# ------------------------------------------------------------------------------------------------------------------------
def tol_out(r, dtype):
    return eps16(dtype) * r["ref"]["out"].abs() + tiny16(dtype) + 2.0 ** -16 * r["abs"]["out"] + r["pos"]["out"]


def tol_split(r, dtype):
    return eps16(dtype) ** 2 * r["ref"]["out"].abs() + 2.0 ** -16 * r["abs"]["out"] + 2.0 ** -24 + r["pos"]["out"]


def tol_doff(r, Dh):
    return (4 * Dh + 16) * 2 * U * r["abs"]["doff"] + r["pos"]["doff"]


def tol_dlogit(r, Dh, LP):
    return (4 * Dh + LP + 16) * 2 * U * r["abs"]["dlogit"] + r["pos"]["dlogit"]


def tol_dvalue(r, M, route, dtype=None, amax=0.0):
    """route: "scatter" (the LDS-tile and global-atomics kernels), "sorted" (+ the fixed-point grid: half a step per record,
    doubled; the step is 2^(e - 29) <= amax 2^-29 with e = amax's exponent, which the kernel keeps >= -97, a step of 2^-126),
    "matrix" (+ the merged weights' 16-bit storage)."""
    B, Lin, D = r["ref"]["dvalue"].shape
    n = r["count"].to(torch.float64).unsqueeze(-1).expand(B, Lin, M, D // M).reshape(B, Lin, D)
    tol = (n + 16) * 2 * U * r["abs"]["dvalue"] + r["pos"]["dvalue"]
    if route == "sorted":
        tol = tol + n * max(amax * 2.0 ** -29, 2.0 ** -126)
    elif route == "matrix":
        tol = tol + eps16(dtype) * r["abs"]["dvalue"]
    else:
        assert route == "scatter"
    return tol


def worst(got, ref, tol):
    """-> (largest |got - ref| / tol, its index tuple); a non-finite element, or any error where tol == 0, counts as inf"""
    got, ref = got.detach().to(torch.float64).cpu(), ref.to(torch.float64)
    assert got.shape == ref.shape == tol.shape, (got.shape, ref.shape, tol.shape)
    err = (got - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, math.inf))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / tol)
    i = int(ratio.reshape(-1).argmax())
    return float(ratio.reshape(-1)[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), err.shape))


def assert_within(what, got, ref, tol, axes):
    """every element within its bound; a failure names the worst element by ``axes`` (e.g. "b q m*Dh+c")"""
    ratio, idx = worst(got, ref, tol)
    print(f"{what}: worst |err|/bound {ratio:.3f} at ({axes}) = {idx}")
    if not ratio <= 1.0:
        g, rr = float(got.detach().to(torch.float64).cpu()[idx]), float(ref[idx])
        raise AssertionError(f"{what}: element ({axes}) = {idx}: got {g!r}, reference {rr!r}, |err| {abs(g - rr):.3e}, "
                             f"bound {float(tol[idx]):.3e} (x{ratio:.2f})")
    return ratio


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def _positions(ref, off, shapes, dtype):
    """px, py [B, Lq, M, L, P] of every point by the kernel's own sequence of operations in ``dtype``"""
    r, o = ref.to(dtype), off.to(dtype)
    px, py = [], []
    for l, (H, W) in enumerate(shapes):
        px.append((r[:, 0].view(1, -1, 1, 1) + o[:, :, :, l, :, 0] / W) * W - 0.5)
        py.append((r[:, 1].view(1, -1, 1, 1) + o[:, :, :, l, :, 1] / H) * H - 0.5)
    return torch.stack(px, 3), torch.stack(py, 3)


def boundary_distance(case):
    """smallest distance of any sampling coordinate of ``case`` to an integer (a cell boundary), in pixels, float64"""
    B, Lq, M, P, shapes = case["B"], case["Lq"], case["M"], case["P"], case["shapes"]
    L = len(shapes)
    off = case["offaw"][:, :M * L * P * 2].reshape(B, Lq, M, L, P, 2)
    px, py = _positions(case["ref"], off, shapes, torch.float64)
    p = torch.stack([px, py])
    return float((p - p.round()).abs().min())


def fp32_positions_exact(case):
    """"exact" cases: the kernel's fp32 px, py equal the float64 ones bit for bit wherever the point is within 4 pixels of its
    level (the wild offsets round, and land outside either way)"""
    B, Lq, M, P, shapes = case["B"], case["Lq"], case["M"], case["P"], case["shapes"]
    L = len(shapes)
    off = case["offaw"][:, :M * L * P * 2].reshape(B, Lq, M, L, P, 2)
    p32, p64 = _positions(case["ref"], off, shapes, torch.float32), _positions(case["ref"], off, shapes, torch.float64)
    ok = True
    for a, b in zip(p32, p64):
        near = b.abs() < 256
        ok = ok and bool((a.double()[near] == b[near]).all()) and bool((a.double()[~near].abs() > 1e5).all())
    return ok


WILD = (1e6, -1e6, 3e9, -3e9)


def make_case(name, B, Lq, M, Dh, shapes, P, dtype, mode="random", dout_scale=1.0, shared_ref=False):
    """Inputs of one MSDA case, made on the CPU before either side sees them.  ``value`` and ``dout`` hold values of the 16-bit
    ``dtype`` exactly; logits have spread <= 4.
    mode "random": uniform ref, offsets up to +-2.5 px (some points leave the level).  Guarantee (a): wherever px or py (float64)
        is within 2^-8 of an integer its offset is moved by 2^-6 px, so the kernel's fp32 position (error < 2^-14 px for levels
        up to 128 wide) falls in the same cell; ``case["moved"]`` counts them, none is excluded.
    mode "exact": guarantee (b): power-of-two levels, ref = (k + 0.5) / (Wmax, Hmax), and offsets that put the points on a fixed
        list of targets — pixel centres, px in {-1, -0.5, W-1, W-0.5, W} (same in y), mid-cell points — or +-1e6 / +-3e9 px away;
        every fp32 intermediate is a short dyadic number, so the kernel's px is exact.
    shared_ref: every query has the same ref and (before (a)) zero offsets: one cell collects all the records."""
    L, LP, D = len(shapes), len(shapes) * P, M * Dh
    Lin = sum(h * w for h, w in shapes)
    gen = torch.Generator().manual_seed(abs(hash_name(name)) % (2 ** 31))
    rnd = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
    value = ((rnd(B, Lin, D) * 2 - 1) * 1.5).float().to(dtype)
    dout = (((rnd(B * Lq, D) * 2 - 1) * 1.5).float().to(dtype).float() * dout_scale).to(dtype).float()
    logit = ((rnd(B * Lq, M * LP) * 4 - 2)).float()
    moved = 0
    if mode == "random":
        ref = rnd(Lq, 2).float()
        off = ((rnd(B, Lq, M, L, P, 2) * 2 - 1) * 2.5).float()
        if shared_ref:
            ref = torch.tensor([0.37, 0.61]).repeat(Lq, 1)
            off = torch.zeros_like(off)
        for _ in range(2):
            px, py = _positions(ref, off, shapes, torch.float64)
            p = torch.stack([px, py], -1)                                  # [B, Lq, M, L, P, 2]
            close = (p - p.round()).abs() < 2.0 ** -8
            moved += int(close.sum())
            off = torch.where(close, off + 2.0 ** -6, off)
    else:
        assert mode == "exact" and all(h & (h - 1) == 0 and w & (w - 1) == 0 for h, w in shapes)
        Hm, Wm = max(h for h, _ in shapes), max(w for _, w in shapes)
        q = torch.arange(Lq)
        # k sweeps the first and the last cells first, so px = k + offset reaches both borders on the full-size level
        kx = torch.tensor([(0, Wm - 1, 1, Wm // 2)[i % 4] if i < 8 else (5 * i) % Wm for i in range(Lq)])
        ky = torch.tensor([(0, Hm - 1, Hm // 2, 1)[(i // 2) % 4] if i < 8 else (3 * i) % Hm for i in range(Lq)])
        ref = torch.stack([(kx + 0.5) / Wm, (ky + 0.5) / Hm], -1).float()
        off64 = torch.zeros(B, Lq, M, L, P, 2, dtype=torch.float64)
        n = torch.arange(B * Lq * M * P).view(B, Lq, M, P)
        for l, (H, W) in enumerate(shapes):
            for a, (S, rr) in enumerate(((W, ref[:, 0]), (H, ref[:, 1]))):
                targets = torch.tensor([-1.0, -0.5, 0.0, 0.5, 1.0, S - 2.0, S - 1.5, S - 1.0, S - 0.5, float(S), S / 2.0,
                                        S / 2.0 + 0.25, -1.5, S + 0.5], dtype=torch.float64)
                pick = (n * (3 if a else 1) + (n // 14 if a else 0) + 5 * l + a) % len(targets)
                base = rr.double().view(1, Lq, 1, 1) * S - 0.5
                off64[:, :, :, l, :, a] = targets[pick] - base
        wild = (n % 23) == 7                                                 # some points far outside, in x, y or both
        wv = torch.tensor(WILD, dtype=torch.float64)[(n // 23) % 4]
        for l in range(L):
            off64[:, :, :, l, :, 0] = torch.where(wild & (n % 2 == 1), wv, off64[:, :, :, l, :, 0])
            off64[:, :, :, l, :, 1] = torch.where(wild & (n % 3 != 1), wv, off64[:, :, :, l, :, 1])
        off = off64.float()
        assert bool((off.double() == off64).all())
    offaw = torch.cat([off.reshape(B * Lq, -1), logit], 1).contiguous()
    return dict(name=name, B=B, Lq=Lq, M=M, Dh=Dh, shapes=list(shapes), P=P, dtype=dtype, mode=mode, value=value, dout=dout,
                offaw=offaw, ref=ref.contiguous(), moved=moved, excluded=0)


def hash_name(name):
    h = 0
    for ch in str(name):
        h = (h * 131 + ord(ch)) % 1000000007
    return h


def reference_of(case, **kw):
    return msda_reference(case["value"], case["offaw"], case["ref"], case["shapes"], case["M"], case["P"], dout=case["dout"], **kw)


# ---- the case lists of tests/test_gpu_msda_routes.py: (name, B, Lq, M, Dh, shapes, P, mode) ------------------------------
PYR3, PYR4 = [(16, 16), (8, 8), (4, 4)], [(16, 16), (8, 8), (4, 4), (2, 2)]
FWD_CASES = [
    ("m1d8-1x7-p1", 2, 37, 1, 8, [(1, 7)], 1, "random"),                   # NC=1, L*P = 1, H == 1
    ("m2d24-5x1-p1", 1, 50, 2, 24, [(5, 1)], 1, "random"),                 # NC=1, W == 1
    ("m4d16-1x1+2x3-p8", 2, 19, 4, 16, [(1, 1), (2, 3)], 8, "random"),     # NC=2, L*P = 16 as (2, 8), a 1x1 level
    ("m8d32-pyr3-p4", 2, 50, 8, 32, PYR3, 4, "random"),                    # NC=2, (3, 4)
    ("m2d128-pyr4-p4", 1, 33, 2, 128, PYR4, 4, "random"),                  # NC=2, L*P = 16 as (4, 4)
    ("m2d24-pyr3-p4", 2, 21, 2, 24, PYR3, 4, "random"),                    # NC=1 on the pyramid
    ("x-m4d16-pyr3-p4", 2, 48, 4, 16, PYR3, 4, "exact"),                   # NC=2, borders / centres / wild offsets
    ("x-m1d8-pyr4-p4", 1, 32, 1, 8, PYR4, 4, "exact"),                     # NC=1, the same
    ("x-m2d24-1x8+4x1-p8", 1, 16, 2, 24, [(1, 8), (4, 1)], 8, "exact"),    # H == 1 and W == 1 levels, exact
    ("x-m2d128-16x16-p1", 2, 24, 2, 128, [(16, 16)], 1, "exact"),
]
# d offsets / d logits: the per-head reduction of msda_bwd_kernel.  shuffle: Dh/8 a power of two <= 64 and D % 512 == 0
RED_SHAPES, RED_P, RED_B, RED_LQ = [(6, 7), (3, 4)], 2, 2, 11
RED_CASES = [(4, 128, "shuffle"), (8, 64, "shuffle"), (32, 16, "shuffle"), (2, 256, "shuffle"), (16, 128, "shuffle"),
             (16, 96, "atomics"), (1, 1024, "atomics"), (32, 8, "atomics"), (2, 24, "atomics")]
# d value scatter: the level whose Lin selects the kernel (M = 1, Dh = 8, Lq = 64, P = 4)
LIN_CASES = [((64, 64), "tile<8>"), ((65, 64), "tile<4>"), ((129, 64), "tile<2>"), ((129, 128), "global atomics")]
# d value sorted / matrix: (name, B, Lq, M, Dh, shapes, P, shared_ref)
SM_SHAPES = [(6, 7), (3, 4), (2, 2)]
SM_CASES = [("sm-m4d16", 2, 50, 4, 16, SM_SHAPES, 4, False), ("sm-m2d128", 2, 50, 2, 128, SM_SHAPES, 4, False),
            ("sm-m2d256", 2, 23, 2, 256, SM_SHAPES, 4, False), ("sm-m1d1024", 1, 23, 1, 1024, SM_SHAPES, 4, False),
            ("sm-shared-m4d16", 2, 50, 4, 16, SM_SHAPES, 4, True), ("sm-lq1-m4d16", 2, 1, 4, 16, SM_SHAPES, 4, False)]
# |dout| reaches 1.5 before scaling: amax's exponent is the scale's down to 2^-97, then -98 (2^-98.5), -99 (2^-99), -100 (2^-100)
AMAX_SCALES = [1.0, 2.0 ** -20, 2.0 ** -60, 2.0 ** -97, 2.0 ** -98.5, 2.0 ** -99, 2.0 ** -100, 0.0]
DTYPES = [torch.float16, torch.bfloat16]


def fwd_case(c, dtype):
    name, B, Lq, M, Dh, shapes, P, mode = c
    return make_case(name, B, Lq, M, Dh, shapes, P, dtype, mode)


def red_case(c, dtype):
    M, Dh, _ = c
    return make_case(f"red-m{M}d{Dh}", RED_B, RED_LQ, M, Dh, RED_SHAPES, RED_P, dtype)


def lin_case(c, dtype):
    (H, W), _ = c
    return make_case(f"lin-{H}x{W}", 2, 64, 1, 8, [(H, W)], 4, dtype)


def sm_case(c, dtype, dout_scale=1.0):
    name, B, Lq, M, Dh, shapes, P, shared = c
    return make_case(name, B, Lq, M, Dh, shapes, P, dtype, dout_scale=dout_scale, shared_ref=shared)


def all_cases():
    """every (case, dtype) the GPU tests generate with `make_case` (the grid-stride case is built by `grid_stride_case`)"""
    for dt in DTYPES:
        for c in FWD_CASES:
            yield fwd_case(c, dt)
        for c in RED_CASES:
            yield red_case(c, dt)
        for c in LIN_CASES:
            yield lin_case(c, dt)
        for c in SM_CASES:
            yield sm_case(c, dt)


GS_ROWS = 65535 * 8 + 300


def grid_stride_case():
    """B*Lq = 65535*8 + 300 queries on one 4x4 level, M = 1, Dh = 8, L = P = 1, fp16: more rows than msda_bwd_kernel's grid"""
    return make_case("grid-stride", 1, GS_ROWS, 1, 8, [(4, 4)], 1, torch.float16)


# ------------------------------------------------------------------------------------------------------------------------
# DWConv 3x3 + erf GELU
# ------------------------------------------------------------------------------------------------------------------------
def _per_level(x, grids, fn):
    B, N, C = x.shape
    outs, s = [], 0
    for gh, gw in grids:
        xi = x[:, s:s + gh * gw].transpose(1, 2).reshape(B, C, gh, gw)
        outs.append(fn(xi).flatten(2).transpose(1, 2))
        s += gh * gw
    assert s == N
    return torch.cat(outs, 1)


def dwconv_reference(x, w, bias, grids, dy=None, work=torch.float64):
    """x [B, Ntok, C] fp32 values, w [C, 1, 3, 3], bias [C], dy [B, Ntok, C] -> ref / abs / pre dicts.
    out = gelu(pre), pre = bias + conv(x, w) per level (F.conv2d, groups = C, as oracle.ref_torch.dwconv).
    abs:  out: S_pre = |bias| + conv(|x|, |w|).
          g = dy gelu'(pre) is first made without cancellation: G = |dy| (|gelu'(pre)| + |gelu''(pre)| S_pre), the second term being
          what an error of S_pre-relative size in the recomputed pre does to it; then dx: conv^T(G, |w|);
          d w9[t]: sum_rows (G + |dy|) |x shifted by t|;  d bias: sum_rows (G + |dy|)  (the + |dy| carries the 2^-20 absolute allotment
          of the GELU-gradient intrinsics, which the (rows + nblk + 16) 2u >= 2^-19 in front of it covers).
    pre:  out: |pre|;  dx: conv^T(|dy| (1 + |pre|), |w|): the same 2^-20 allotment through the transposed conv."""
    B, N, C = x.shape
    grad = dy is not None
    xr = x.to(work).clone().requires_grad_(grad)
    wr, br = w.to(work).clone().requires_grad_(grad), bias.to(work).clone().requires_grad_(grad)
    conv = lambda t, ww, bb: _per_level(t, grids, lambda xi: F.conv2d(xi, ww, bb, padding=1, groups=C))
    pre = conv(xr, wr, br)
    out = F.gelu(pre)
    res = {"ref": {"out": out.detach()}, "abs": {}, "pre": {"out": pre.detach().abs().double()}}
    d64 = torch.float64
    xa, wa, ba = x.to(d64).abs(), w.to(d64).abs(), bias.to(d64).abs()
    s_pre = conv(xa, wa, ba)
    res["abs"]["out"] = s_pre
    if grad:
        (out * dy.to(work)).sum().backward()
        res["ref"].update(dx=xr.grad, dw9=wr.grad.reshape(C, 9).t().contiguous(), dbias=br.grad)
        p = pre.detach().to(d64)
        pdf = torch.exp(-0.5 * p * p) / math.sqrt(2 * math.pi)
        g1 = 0.5 * (1 + torch.erf(p / math.sqrt(2))) + p * pdf
        g2 = pdf * (2 - p * p)
        dya = dy.to(d64).abs()
        G = dya * (g1.abs() + g2.abs() * s_pre)
        convT = lambda t: _per_level(t, grids, lambda ti: F.conv_transpose2d(ti, wa, None, padding=1, groups=C))
        res["abs"]["dx"] = convT(G)
        res["pre"]["dx"] = convT(dya * (1 + p.abs()))
        Gw = (G + dya).clone().requires_grad_(False)
        # sum_rows Gw * |x shifted|: the weight gradient of the conv on |x| against Gw
        wz = torch.zeros_like(wa).requires_grad_(True)
        bz = torch.zeros_like(ba).requires_grad_(True)
        (conv(xa, wz, bz) * Gw).sum().backward()
        res["abs"]["dw9"], res["abs"]["dbias"] = wz.grad.reshape(C, 9).t().contiguous(), bz.grad
    return res


def tol_dw_out(r, dtype, key="out"):
    return eps16(dtype) * r["ref"][key].abs() + tiny16(dtype) + 2.0 ** -18 * r["abs"][key] + 2.0 ** -20 * r["pre"][key]


def tol_dw_param(r, key, rows, nblk):
    return (rows + nblk + 16) * 2 * U * r["abs"][key]


def dwconv_nblk(rows):
    """blocks of dwconv_gelu_bwd_kernel (asis_dwconv_bwd_nblk): 64 rows each, at most 1024"""
    return max(1, min(1024, (rows + 63) // 64))


def make_dwconv_case(name, B, C, grids):
    """|pre| mostly within +-3: x uniform +-1.5, w +-0.6, bias +-0.5"""
    Ntok = sum(a * b for a, b in grids)
    gen = torch.Generator().manual_seed(hash_name(name) % (2 ** 31))
    rnd = lambda *s: (torch.rand(*s, generator=gen, dtype=torch.float64) * 2 - 1)
    return dict(name=name, B=B, C=C, grids=list(grids), x=(rnd(B, Ntok, C) * 1.5).float(), w=(rnd(C, 1, 3, 3) * 0.6).float(),
                bias=(rnd(C) * 0.5).float(), dy=rnd(B, Ntok, C).float())


DW_PYRS = [[(7, 9), (4, 5), (2, 3)], [(1, 6), (5, 1), (1, 1)], [(3, 3)]]
# (name, B, C, grids, backward runs)
DW_CASES = [(f"dw-c{C}-b{B}-p{i}", B, C, g, C != 12) for C in (4, 12, 16, 64, 1024) for i, g in enumerate(DW_PYRS)
            for B in (1, 3) if not (C == 1024 and B == 3 and i == 0) and not (C == 12 and B == 3)]
DW_BIG = ("dw-c4-big", 1, 4, [(256, 256), (7, 10)], True)       # 65536 + 70 rows: 65 rows per block, the last block ends early
