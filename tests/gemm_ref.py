"""The cells of the GEMM / implicit-GEMM convolution form tests (test_gemm_ref_cpu.py, test_gpu_gemm_forms.py): which kernel form a
launch must plan to (csrc/gemm.hip: gemm_plan), its operands, a float64 restatement of ``asis_gemm``'s arithmetic
(include/asis_hip.h) and a checker that looks at EVERY element and names the worst one.  Nothing here needs a GPU.

Two operand kinds.
  exact   small integers (A, B, A_lo, B_lo in -r .. r; bias_n, bias_m, res integers; scale_n a power of two in {0.5, 1, 2, 4}):
          every partial sum of every summation order is a multiple of 0.5 below 2^23, so an fp32 output must be BIT-EQUAL to the
          float64 reference and a 16-bit output equal to ``ref.float().to(dt)`` (to_t16 is round-to-nearest-even); r is widened
          for 16-bit outputs until at least a quarter of the elements need that rounding (|ref| > 2048 fp16, > 256 bf16).
  random  normal operands rounded to the 16-bit type, for what cannot be exact (GELU, GELU', SiLU, column / row sums).  Per
          element |got - ref| <= max(4 Y, U ulp32 max|ref|) (tests/bound_helpers.py; Y = error of torch's float32 CPU evaluation
          of the same formula, U = U_ELEM for outputs, U_SUM for sums), + HALF[dt] |ref| + SUBN[dt] for a 16-bit output, + the
          allowance of the two approximated functions below.

``gelu_fast`` / ``gelu_grad_fast`` restate csrc/asis_common.h: gelu_erf / gelu_erf_grad_fast in float64.  Their allowances are the
worst gap to the exact erf forms on a dense grid (``approx_gap``), measured on the FORMULA, never on a kernel:
GELU_GAP = 5.2e-8 absolute on [-12, 12]; GELU_GRAD_GAP = 7.0e-8 absolute on [-8, 8] (measured 5.17e-8 and 6.97e-8;
test_gemm_ref_cpu.py pins both).  The float32 ROUNDING of the two formulas is part of Y: Y is the larger of the float32 errors of
the exact and of the restated formula, each against its own float64 evaluation."""
import dataclasses
import functools
import math

import torch
import torch.nn.functional as F

from adaptersis_amd._lib import ACT_GELU, ACT_GELU_GRAD, ACT_NONE, ACT_RELU, ACT_SILU_MUL
from tests.bound_helpers import HALF, SUBN, U_ELEM, U_SUM, ULP32, _gen

F16, BF16 = torch.float16, torch.bfloat16
SENTINEL = -123.0          # representable in both 16-bit types
UNREP = {F16: 2048.0, BF16: 256.0}      # above this an integer may need rounding
# (rows, columns) of one workgroup tile of each form: the checker's (tile_m, tile_n, row-in-tile, col-in-tile)
TILE = {"generic": (128, 128), "generic_conv": (128, 128), "big_256x128_m16": (256, 128), "ph8_m16": (256, 256), "ph8_ln": (256, 256),
        "p8": (256, 256), "big_256x128_split": (256, 128), "big_256x64_split": (256, 64), "conv_256x64": (256, 64),
        "conv_256x128": (256, 128), "conv_ph8": (256, 256), "conv_256x64_split": (256, 64), "conv_512x64_split": (512, 64),
        "conv_256x128_split": (256, 128), "conv_ph8_split": (256, 256)}
# forms the table leaves out on purpose (test_gpu_gemm_forms.py says why)
LEFT_OUT = {"ph8_mx", "conv_ph8_mx", "conv_512x64_mx", "conv_256x128_mx", "conv_256x64_mx",            # MX: test_gpu_mx.py
            "p8_ln",                                                                                    # LayerNorm-fold consumer
            "ph8_m32", "big_256x128", "big_256x128_k64", "big_256x256", "conv_512x64_split_m16",      # environment switches
            "conv_256x128_split_m16", "conv_256x128_split_bk32"}
GELU_GAP, GELU_GRAD_GAP = 5.2e-8, 7.0e-8
FULL = ("bias_n", "bias_m", "scale_n", "res")


@dataclasses.dataclass(frozen=True)
class Cell:
    name: str
    form: str
    family: str                 # dense | split | producer | p8 | conv | conv_split
    dt: torch.dtype
    M: int
    N: int
    K: int
    batch: int = 1              # > 1: B is [batch, N, K], A is shared
    out_f32: bool = False
    has: tuple = ()             # bias_n bias_m scale_n res stats aux A_lo B_lo res16 C_lo rowstats
    act: int = ACT_NONE
    exact: bool = True
    p8: int = 1                 # the "p8" option the cell runs under
    stride_c_off: int = 0       # elements added to the batch stride of the output
    conv: tuple = ()            # (B, H, W, Cin, k, stride, pad)
    ksplit: int = 1
    off: tuple = ()             # ((operand, elements into its allocation), ...): misaligned views
    refused: str = ""           # a launch asis_gemm must refuse: what its message names

    @property
    def n_out(self):
        return self.N // 2 if self.act == ACT_SILU_MUL else self.N

    @property
    def out_dt(self):
        return torch.float32 if self.out_f32 else self.dt

    def geometry(self):
        """conv: (B, H, W, Cin, k, stride, pad, OH, OW)"""
        B, H, W, Cin, k, s, p = self.conv
        return B, H, W, Cin, k, s, p, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1


def _dtn(dt):
    return "f16" if dt == F16 else "bf16"


def _cells():
    out = []

    def add(form, family, shape, tag, dts=(F16, BF16), **kw):
        for dt in dts:
            M, N, K = shape
            out.append(Cell(f"{form}-{M}x{N}x{K}-{tag}-{_dtn(dt)}", form, family, dt, M, N, K, **kw))

    def dense_set(form, shape):
        add(form, "dense", shape, "full-f32", out_f32=True, has=FULL)
        add(form, "dense", shape, "full-16", has=FULL)
        add(form, "dense", shape, "full-relu-16", has=FULL, act=ACT_RELU)
        add(form, "dense", shape, "full-gelu-16", has=FULL, act=ACT_GELU, exact=False)
        add(form, "dense", shape, "plain-f32-random", out_f32=True, exact=False)

    dense_set("generic", (300, 136, 72))
    dense_set("generic", (255, 300, 128))
    add("generic", "dense", (255, 300, 128), "stats-f32", out_f32=True, has=("bias_n", "stats"), exact=False)
    add("generic", "dense", (300, 2, 128), "batch3-bias_m-16", batch=3, has=("bias_m",))
    dense_set("big_256x128_m16", (300, 136, 96))
    add("big_256x128_m16", "dense", (300, 132, 96), "full-f32", out_f32=True, has=FULL)
    add("big_256x128_m16", "dense", (300, 132, 96), "full-16", has=FULL)
    add("big_256x128_m16", "dense", (300, 130, 96), "scalar-full-f32", out_f32=True, has=FULL)
    add("big_256x128_m16", "dense", (300, 130, 96), "scalar-full-16", has=FULL)
    add("big_256x128_m16", "dense", (300, 136, 96), "gelu_grad-16", has=("aux",), act=ACT_GELU_GRAD, exact=False)
    add("big_256x128_m16", "dense", (300, 136, 96), "gelu_grad-scale-res-f32", out_f32=True, has=("aux", "scale_n", "res"),
        act=ACT_GELU_GRAD, exact=False)
    big = (300, 264, 2048)
    add("ph8_m16", "dense", big, "bias-16", has=("bias_n",))
    add("ph8_m16", "dense", big, "bias-gelu-16", has=("bias_n",), act=ACT_GELU, exact=False)
    add("ph8_m16", "dense", big, "bias-relu-16", has=("bias_n",), act=ACT_RELU)
    add("ph8_m16", "dense", big, "plain-16-random", exact=False)
    add("ph8_m16", "dense", (300, 260, 2048), "slab-full-16", has=FULL)
    add("ph8_m16", "dense", (300, 260, 2048), "slab-full-f32", out_f32=True, has=FULL)
    add("ph8_m16", "dense", (300, 262, 2048), "scalar-full-16", has=FULL)
    add("ph8_m16", "dense", (300, 262, 2048), "scalar-full-f32", out_f32=True, has=FULL)
    add("ph8_m16", "dense", big, "gelu_grad-16", has=("aux",), act=ACT_GELU_GRAD, exact=False)
    add("ph8_m16", "dense", big, "batch3-bias_m-16", batch=3, has=("bias_m",))
    add("ph8_m16", "dense", big, "batch3-bias_m-16-stride4", batch=3, has=("bias_m",), stride_c_off=4)
    for K in (64, 128):
        add("ph8_m16", "dense", (300, 288, K), "swiglu", has=("bias_n",), act=ACT_SILU_MUL, exact=False)
    for form, shape in (("big_256x128_split", (300, 136, 64)), ("big_256x128_split", (300, 136, 128)), ("big_256x64_split", (300, 36, 64))):
        add(form, "split", shape, "a_lo-f32", out_f32=True, has=("A_lo",))
        add(form, "split", shape, "a_lo-b_lo-f32", out_f32=True, has=("A_lo", "B_lo"))
        add(form, "split", shape, "a_lo-b_lo-bias-f32", out_f32=True, has=("A_lo", "B_lo", "bias_n"))
        add(form, "split", shape, "a_lo-b_lo-f32-random", out_f32=True, has=("A_lo", "B_lo"), exact=False)
    prod = (300, 320, 2048)
    add("ph8_ln", "producer", prod, "planes-rowstats", has=("bias_n", "scale_n", "res16", "C_lo", "rowstats"))
    add("ph8_ln", "producer", prod, "res-f32-rowstats", out_f32=True, has=("bias_n", "scale_n", "res", "rowstats"))
    add("ph8_ln", "producer", prod, "planes-f32out", out_f32=True, has=("bias_n", "scale_n", "res16"))
    add("ph8_ln", "producer", (300, 328, 2048), "planes-overhang", has=("bias_n", "scale_n", "res16", "C_lo"))
    add("ph8_ln", "producer", prod, "planes-rowstats-random", has=("bias_n", "scale_n", "res16", "C_lo", "rowstats"), exact=False)
    p8 = (769, 1032, 128)
    add("p8", "p8", p8, "bias-16", dts=(F16,), p8=2, has=("bias_n",))
    add("p8", "p8", p8, "scale-res-f32", dts=(F16,), p8=2, out_f32=True, has=("scale_n", "res"))
    add("p8", "p8", p8, "a_lo-b_lo-f32", dts=(F16,), p8=2, out_f32=True, has=("A_lo", "B_lo"))
    add("p8", "p8", p8, "plain-16-random", dts=(F16,), p8=2, exact=False)

    def conv(form, Cout, tag, geo=(2, 13, 12, 64, 3, 1, 1), split=False, dts=(F16, BF16), **kw):
        B, H, W, Cin, k, s, p = geo
        P = B * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
        kw["has"] = tuple(kw.get("has", ())) + (("A_lo", "B_lo") if split else ())
        kw.setdefault("out_f32", True)
        for dt in dts:
            out.append(Cell(f"{form}-{Cout}-{tag}-{_dtn(dt)}", form, "conv_split" if split else "conv", dt, P, Cout, k * k * Cin, conv=geo, **kw))

    S2 = (2, 27, 25, 64, 3, 2, 0)
    for form, Cout, split, geo, ks, s2 in (("conv_256x64", 40, False, None, False, True), ("conv_256x128", 136, False, None, True, True),
                                           ("conv_ph8", 256, False, None, True, True), ("conv_ph8", 1032, False, None, False, False),
                                           ("conv_256x64_split", 40, True, None, True, False),
                                           ("conv_512x64_split", 40, True, (2, 17, 16, 64, 3, 1, 1), False, False),
                                           ("conv_256x128_split", 136, True, None, False, False),
                                           ("conv_ph8_split", 256, True, None, True, False),
                                           ("generic_conv", 136, False, (2, 13, 12, 8, 3, 1, 1), False, False),
                                           ("generic_conv", 136, False, (1, 13, 12, 64, 3, 1, 1), False, False)):
        g = dict(geo=geo) if geo else {}
        tag = "" if geo is None else "cin%d-b%d-" % (geo[3], geo[0])
        conv(form, Cout, tag + "bias", split=split, has=("bias_n",), **g)
        conv(form, Cout, tag + "bias-stats", split=split, has=("bias_n", "stats"), exact=False, **g)
        if ks:
            conv(form, Cout, tag + "bias-ksplit3", split=split, has=("bias_n",), ksplit=3, **g)
        if s2:
            conv(form, Cout, "stride2-bias", split=split, has=("bias_n",), geo=S2)
    conv("conv_512x64_split", 40, "stride2-bias", split=True, has=("bias_n",), geo=(2, 35, 33, 64, 3, 2, 0))
    conv("generic_conv", 136, "1x1-16bit", has=("bias_n",), geo=(2, 13, 12, 64, 1, 1, 0), out_f32=False)
    return out


CELLS = _cells()
BY_NAME = {c.name: c for c in CELLS}
assert len(BY_NAME) == len(CELLS)


def _misaligned():
    """the launches whose run-time epilogue choice the plan did not see (csrc/gemm_big.h: vector epilogue or scalar fallback): an
    operand a few bytes into its allocation.  The scalar fallback has no statistics, no GELU' and no K parts: asis_gemm refuses
    them, naming the operand."""
    conv = BY_NAME["conv_256x128-136-bias-stats-f16"]
    ksp = BY_NAME["conv_256x128-136-bias-ksplit3-f16"]
    gg = BY_NAME["big_256x128_m16-300x136x96-gelu_grad-16-f16"]
    ggr = BY_NAME["big_256x128_m16-300x136x96-gelu_grad-scale-res-f32-f16"]
    return [dataclasses.replace(conv, name="misaligned-bias_n-conv-stats", off=(("bias_n", 1),), refused="bias_n"),
            dataclasses.replace(ksp, name="misaligned-bias_n-conv-ksplit3", off=(("bias_n", 1),), refused="bias_n"),
            dataclasses.replace(gg, name="misaligned-bias_n-gelu_grad", has=("aux", "bias_n"), off=(("bias_n", 1),), refused="bias_n"),
            dataclasses.replace(ggr, name="misaligned-res-gelu_grad", off=(("res", 2),), refused="res")]


MISALIGNED = _misaligned()


def family(name, *more):
    return [c for c in CELLS if c.family in (name,) + more]


# ---- operands ---------------------------------------------------------------------------------------------------------------
def _r(cell: Cell) -> int:
    """half-width of the integer operand range of an exact cell: 7, widened for a 16-bit output until the standard deviation of
    the sums is ``m`` UNREP / 1.15 (P(|z| > 1.15) = 0.25 for a normal sum).  m leaves a ReLU cell its quarter and keeps
    4.7 sigma times the largest scale below 60000: 3 for bf16 (UNREP = 256), 2 for fp16, 1.45 for fp16 under scale_n <= 4"""
    r = 7
    if not cell.out_f32:
        m = 3.0 if cell.dt == BF16 else 1.45 if "scale_n" in cell.has else 2.0
        parts = 1 + ("A_lo" in cell.has) + ("B_lo" in cell.has)
        while math.sqrt(cell.K * parts) * r * (r + 1) / 3 < m * UNREP[cell.dt] / 1.15:
            r += 1
    return r


def _key(cell):
    return (cell.M, cell.N, cell.K, cell.batch, cell.dt, cell.exact, cell.conv, _r(cell) if cell.exact else 0)


@functools.lru_cache(maxsize=None)
def _operands(key):
    M, N, K, batch, dt, exact, conv, r = key
    g = _gen(M, N, K, batch, int(dt == F16), int(exact), len(conv) and sum(conv))

    def mat(*shape, width=r, std=1.0):
        if exact:
            return torch.randint(-width, width + 1, shape, generator=g).float()
        return (std * torch.randn(shape, generator=g)).to(dt).float()      # 16-bit operands: rounded here, once

    def vec(*shape, width=20, std=1.0):
        if exact:
            return torch.randint(-width, width + 1, shape, generator=g).float()
        return std * torch.randn(shape, generator=g)

    o = {}
    if conv:
        B, H, W, Cin, k, s, p = conv
        o["A"], o["A_lo"] = mat(B, H, W, Cin), mat(B, H, W, Cin, std=2.0 ** -9)
    else:
        o["A"], o["A_lo"] = mat(M, K), mat(M, K, std=2.0 ** -9)
    bshape = (batch, N, K) if batch > 1 else (N, K)
    o["B"], o["B_lo"] = mat(*bshape), mat(*bshape, std=2.0 ** -9)
    o["bias_n"], o["bias_m"] = vec(N), vec(M)
    o["scale_n"] = (2.0 ** torch.randint(-1, 3, (N,), generator=g).float()) if exact else 1 + 0.3 * torch.randn(N, generator=g)
    o["res"] = vec(M, N, width=50, std=3.0)
    o["aux"] = (1.5 * torch.randn((M, N), generator=g)).to(dt).float()
    return o


def operands(cell: Cell) -> dict:
    """the logical (unpadded) operands as float32 CPU tensors, shared by every cell of one shape; 16-bit operands hold values
    of the 16-bit type.  ``res16``: the (hi, lo) planes of ``res``."""
    o = dict(_operands(_key(cell)))
    if "res16" in cell.has:
        hi = o["res"].to(cell.dt)
        o["res16"] = (hi.float(), (o["res"] - hi.float()).to(cell.dt).float())
    return o


# ---- the arithmetic of asis_gemm, in the dtype it is given -----------------------------------------------------------------
def gelu_fast(x):
    """csrc/asis_common.h: gelu_erf, restated in the dtype of x: max(x, 0) - |x| 2^P(min(|x|, 7))"""
    ax = x.abs()
    a = ax.clamp(max=7.0)
    p = torch.full_like(x, 3.30870223e-05)
    for c in (-7.69167002e-04, 8.08053612e-03, -5.34118121e-02, -4.58771202e-01, -1.15120162e+00, 6.93082119e-06 - 1.0):
        p = p * a + c
    return x.clamp(min=0) - ax * torch.exp2(p)


def gelu_grad_fast(x):
    """csrc/asis_common.h: gelu_erf_grad_fast, restated in the dtype of x: Phi(x) + x phi(x) with Abramowitz-Stegun 7.1.26 for Phi"""
    ax = x.abs()
    t = 1.0 / (0.3275911 * 0.70710678118654752440 * ax + 1.0)
    poly = ((((0.5 * 1.061405429 * t - 0.5 * 1.453152027) * t + 0.5 * 1.421413741) * t - 0.5 * 0.284496736) * t + 0.5 * 0.254829592) * t
    e = torch.exp2(-0.5 * 1.4426950408889634 * (x * x))
    q = poly * e
    return torch.where(x >= 0, 1.0 - q, q) + x * e * 0.39894228040143267794


def gelu_grad(x):
    return 0.5 * (1 + torch.erf(x * 0.70710678118654752440)) + x * torch.exp(-0.5 * x * x) * 0.39894228040143267794


def approx_gap():
    """(|gelu_fast - gelu|, |gelu_grad_fast - gelu'|) at their worst on a dense float64 grid: [-12, 12] for the activation (its
    argument is an accumulator; past 7 both are x or 0 to 1e-11), [-8, 8] for the derivative (aux ~ 1.5 N(0, 1) in the cells)"""
    x = torch.linspace(-12, 12, 2_400_001, dtype=torch.float64)
    g = float((gelu_fast(x) - F.gelu(x)).abs().max())
    x = torch.linspace(-8, 8, 1_600_001, dtype=torch.float64)
    return g, float((gelu_grad_fast(x) - gelu_grad(x)).abs().max())


def conv_acc(x, w, cell, border="zero", swap=False):
    """x [B, H, W, Cin], w [Cout, k * k * Cin] (tap-major: kh, kw, ci) -> [B * OH * OW, Cout].  ``border`` / ``swap``: the two
    mistakes the checker must catch (a replicated border; kh and kw exchanged)"""
    B, H, W, Cin, k, s, p, OH, OW = cell.geometry()
    w4 = w.reshape(-1, k, k, Cin).permute(0, 3, 1, 2)
    if swap:
        w4 = w4.transpose(2, 3)
    xn = x.permute(0, 3, 1, 2)
    if border == "replicate" and p:
        xn, p = F.pad(xn, (p, p, p, p), mode="replicate"), 0
    y = F.conv2d(xn, w4.contiguous(), stride=s, padding=p)
    return y.permute(0, 2, 3, 1).reshape(B * OH * OW, -1)


def evaluate(cell: Cell, o: dict, dt=torch.float64, mutate=None) -> dict:
    """asis_gemm's arithmetic on ``o`` in ``dt`` (float64: the reference; float32: the yardstick Y) ->
    ``out`` [batch, M, n_out] before the output rounding, ``acc``, and where the cell has them ``stats`` [2, tiles, N] (sum and
    sum of squares per tile of TILE[form] rows) and ``rowstats`` [M, N / 64, 2].  ``mutate``: dict of deliberate mistakes
    (test_gemm_ref_cpu.py): bias_times, border, swap; fast: the kernels' approximations of GELU / GELU'."""
    mutate = mutate or {}
    c = {k: (tuple(t.to(dt) for t in v) if isinstance(v, tuple) else v.to(dt)) for k, v in o.items()}
    A, B = c["A"], c["B"]

    def prod(a, b):
        if cell.conv:
            return conv_acc(a, b, cell, mutate.get("border", "zero"), mutate.get("swap", False))[None]
        return (a @ b.transpose(-1, -2)).reshape(cell.batch, cell.M, cell.N)

    acc = prod(A, B)
    if "A_lo" in cell.has:
        acc = acc + prod(c["A_lo"], B)
    if "B_lo" in cell.has:
        acc = acc + prod(A, c["B_lo"])
    v = acc
    if "bias_n" in cell.has:
        v = v + mutate.get("bias_times", 1) * c["bias_n"]
    if "bias_m" in cell.has:
        v = v + c["bias_m"][:, None]
    if cell.act == ACT_GELU:
        v = gelu_fast(v) if mutate.get("fast") else F.gelu(v)
    elif cell.act == ACT_RELU:
        v = v.clamp(min=0)
    elif cell.act == ACT_GELU_GRAD:
        v = v * (gelu_grad_fast(c["aux"]) if mutate.get("fast") else gelu_grad(c["aux"]))
    elif cell.act == ACT_SILU_MUL:      # logical column order here: [x1 | x2]; the device rows go through ops.swiglu_rows
        x1, x2 = v[..., :cell.N // 2], v[..., cell.N // 2:]
        v = x1 * torch.sigmoid(x1) * x2
    if "scale_n" in cell.has:
        v = v * c["scale_n"]
    if "res" in cell.has:
        v = v + c["res"]
    if "res16" in cell.has:
        v = v + (c["res16"][0] + c["res16"][1])
    r = {"out": v, "acc": acc}
    if "stats" in cell.has:
        r["stats"] = tile_sums(cell, v[0])
    if "rowstats" in cell.has:
        g = v[0].reshape(cell.M, cell.N // 64, 64)
        r["rowstats"] = torch.stack((g.sum(2), (g * g).sum(2)), 2)
    return r


def tile_sums(cell, v):
    """[2, row tiles of the form, N]: column sums and sums of squares of each tile's rows"""
    tm = TILE[cell.form][0]
    nt = -(-cell.M // tm)
    vp = F.pad(v, (0, 0, 0, nt * tm - cell.M)).reshape(nt, tm, -1)
    return torch.stack((vp.sum(1), (vp * vp).sum(1)))


def stats_table(cell, sums):
    """the contract of the stats table (csrc/gemm_big.h): [ceil(M / 128), 2, N]; a tile's first row carries its sums, the other
    rows it covers are zero"""
    rb = TILE[cell.form][0] // 128
    t = torch.zeros((-(-cell.M // 128), 2, cell.N), dtype=sums.dtype)
    t[::rb] = sums.permute(1, 0, 2)
    return t


# ---- what a launch must produce --------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Expect:
    ref: torch.Tensor                 # float64
    exact: torch.Tensor = None        # bit pattern to meet, in the output dtype (exact cells)
    bound: torch.Tensor = None        # per-element float64 bound (random cells)
    yard: float = 0.0


def _bound(f32, ref, ulps):
    yard = float((f32.double() - ref).abs().max())
    return max(4 * yard, ulps * ULP32 * float(ref.abs().max())), yard


@functools.lru_cache(maxsize=None)
def expectations(cell: Cell) -> dict:
    """name -> Expect for ``out`` (+ ``out_lo``, ``stats``, ``rowstats``); computed once per cell and never modified"""
    o = operands(cell)
    r64 = evaluate(cell, o)
    r32 = evaluate(cell, o, torch.float32)
    ref = r64["out"]
    e = {}
    if cell.exact:
        q = ref.float()
        hi = q.to(cell.out_dt)
        e["out"] = Expect(ref, exact=hi)
        if "C_lo" in cell.has:
            e["out_lo"] = Expect(ref - hi.double(), exact=(q - hi.float()).to(cell.dt))
    else:
        b, yard = _bound(r32["out"], ref, U_ELEM)
        if cell.act in (ACT_GELU, ACT_GELU_GRAD):
            fast = dict(fast=True)
            yard = max(yard, float((evaluate(cell, o, torch.float32, fast)["out"].double() - evaluate(cell, o, mutate=fast)["out"]).abs().max()))
            b = max(b, 4 * yard)
        bound = torch.full_like(ref, b)
        if cell.act == ACT_GELU:
            bound += GELU_GAP * (o["scale_n"].double().abs() if "scale_n" in cell.has else 1.0)
        if cell.act == ACT_GELU_GRAD:
            bound += GELU_GRAD_GAP * r64["acc"].abs() * (o["scale_n"].double().abs() if "scale_n" in cell.has else 1.0)
        if "C_lo" in cell.has:       # the pair hi + lo is compared: PAIR[dt] |ref| is the pair's own rounding
            from tests.bound_helpers import PAIR
            bound += PAIR[cell.dt] * ref.abs() + SUBN[cell.dt]
        elif not cell.out_f32:
            bound += HALF[cell.dt] * ref.abs() + SUBN[cell.dt]
        e["out"] = Expect(ref, bound=bound, yard=yard)
    if "stats" in cell.has:
        t64, t32 = r64["stats"], r32["stats"]
        bound = torch.empty_like(t64)
        for k in (0, 1):
            bound[k] = _bound(t32[k], t64[k], U_SUM)[0]
        e["stats"] = Expect(stats_table(cell, t64), bound=stats_table(cell, bound))
    if "rowstats" in cell.has:
        t64, t32 = r64["rowstats"], r32["rowstats"]
        bound = torch.empty_like(t64)
        for k in (0, 1):
            bound[..., k] = _bound(t32[..., k], t64[..., k], U_SUM)[0]
        e["rowstats"] = Expect(t64, bound=bound)
    return e


# ---- the checker ------------------------------------------------------------------------------------------------------------
def where(cell: Cell, what: str, idx) -> str:
    """an element's place in words: dense (row, col) and its tile coordinates; conv (b, oh, ow, cout)"""
    idx = [int(i) for i in idx]
    if what == "stats":
        return "stats row %d (output rows %d..), kind %d, column %d" % (idx[0], idx[0] * 128, idx[1], idx[2])
    if what == "rowstats":
        return "row %d, 64-column group %d, kind %d" % tuple(idx)
    b, row, col = idx
    if cell.conv:
        _, _, _, _, _, _, _, OH, OW = cell.geometry()
        return "(b, oh, ow, cout) = (%d, %d, %d, %d)" % (row // (OH * OW), row % (OH * OW) // OW, row % OW, col)
    tm, tn = TILE[cell.form]
    return "batch %d (row, col) = (%d, %d): tile (%d, %d), row %d col %d in the %dx%d tile" % (b, row, col, row // tm, col // tn, row % tm,
                                                                                               col % tn, tm, tn)


def check(cell: Cell, what: str, got: torch.Tensor, exp: Expect) -> float:
    """every element of ``got`` (any device; the shape of exp.ref) against ``exp``; AssertionError naming the worst element and
    the number of bad ones.  -> the largest error"""
    got = got.detach().cpu()
    assert got.shape == exp.ref.shape, (cell.name, what, tuple(got.shape), tuple(exp.ref.shape))
    err = (got.double() - exp.ref).abs()
    if exp.exact is not None:
        assert got.dtype == exp.exact.dtype, (cell.name, what, got.dtype)
        bad = (got != exp.exact) | got.isnan()
        err = (got.double() - exp.exact.double()).abs()
        rule = "must equal the float64 reference%s bit for bit" % ("" if got.dtype == torch.float32 else " rounded to %s" % _dtn(cell.dt))
    else:
        bad = ~(err <= exp.bound)           # NaN is bad
        rule = "bound max(4 Y, U ulp32 max|ref|) + output rounding, Y = %.3e" % exp.yard
    err = torch.where(got.double().isfinite(), err, torch.full_like(err, float("inf")))
    n = int(bad.sum())
    if n:
        score = torch.where(bad, err if exp.exact is not None else err / exp.bound.clamp(min=1e-300), torch.zeros_like(err))
        i = torch.unravel_index(torch.argmax(score), score.shape)
        raise AssertionError("%s %s: %d of %d elements wrong (%s); worst at %s: got %r, reference %r%s" % (
            cell.name, what, n, bad.numel(), rule, where(cell, what, i), float(got[i]), float(exp.ref[i]),
            "" if exp.exact is not None else ", bound %.3e" % float(exp.bound[i])))
    return float(err.max())


def check_pad(cell: Cell, what: str, flat: torch.Tensor, body: torch.Tensor):
    """``body`` is a strided view into the 1-D allocation ``flat`` that was filled with SENTINEL: nothing outside it was written"""
    mask = torch.zeros(flat.numel(), dtype=torch.bool)
    first = body.storage_offset() - flat.storage_offset()
    torch.as_strided(mask, body.shape, body.stride(), first).fill_(True)
    f = flat.detach().cpu()
    bad = (~mask) & (f != SENTINEL)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        ld = body.stride(-2)
        raise AssertionError("%s %s: %d pad elements written; first at flat offset %d (row %d, column %d of the padded rows), value %r"
                             % (cell.name, what, int(bad.sum()), i, (i - first) // ld, (i - first) % ld, float(f[i])))


# ---- guarded device tensors -------------------------------------------------------------------------------------------------
def guarded(t: torch.Tensor, dt, device, row_pad=1, col_pad=8, fill=float("nan"), off=0):
    """-> (flat allocation, view of t's shape): the last two dims sit in rows of ``cols + col_pad`` with ``row_pad`` extra rows,
    ``off`` elements into the allocation; everything else holds ``fill``"""
    *lead, R, Ccols = t.shape
    nl = math.prod(lead)
    ld, sb = Ccols + col_pad, (R + row_pad) * (Ccols + col_pad)
    flat = torch.full((off + nl * sb + 8,), fill, dtype=dt, device=device)
    shape, stride = (*lead, R, Ccols), (*[sb * math.prod(lead[i + 1:]) for i in range(len(lead))], ld, 1)
    view = torch.as_strided(flat, shape, stride, off)
    view.copy_(t.to(dt))
    return flat, view


def guarded_vec(t, device, off=0):
    """fp32 vector ``off`` elements into an allocation with NaN on both sides (contiguous, so ops takes it)"""
    buf = torch.full((off + t.numel() + 4,), float("nan"), dtype=torch.float32, device=device)
    buf[off:off + t.numel()] = t
    return buf[off:off + t.numel()]


def out_buffer(cell: Cell, device, dt=None):
    """-> (flat, view [batch, M, n_out] or [M, n_out]): SENTINEL everywhere, 8 pad columns and one pad row per batch entry"""
    M, n = cell.M, cell.n_out
    ld = n + 8
    sb = (M + 1) * ld + cell.stride_c_off
    flat = torch.full((cell.batch * sb + 8,), SENTINEL, dtype=dt or cell.out_dt, device=device)
    if cell.batch > 1:
        return flat, torch.as_strided(flat, (cell.batch, M, n), (sb, ld, 1))
    return flat, torch.as_strided(flat, (M, n), (ld, 1))
