"""Float64 references, dispatch rules, case tables and inputs of the ViT row kernels (csrc/norm.hip, csrc/vit_bwd.hip,
csrc/row_routines.h), shared by tests/test_vit_rows_ref_cpu.py (no GPU: the references against autograd, every table entry
against the dispatch rules, every input rule) and tests/test_gpu_vit_rows.py (the kernels against the references).

The references are written from the formulas, not from the kernels.  Each table entry is a shape plus the branch it is meant to
reach; the claim is a literal, and the CPU test recomputes it from the rules below, so that a later change of a rule cannot
silently uncover a branch."""
import functools
import math

import torch
import torch.nn.functional as F

from tests.bound_helpers import DT, _gen

EPS = 1e-6
F32 = torch.float32


# ---- references (float64) ---------------------------------------------------------------------------------------------------
def layernorm(x, w, b, eps=EPS):
    """-> (y, mean, rstd)"""
    x, w, b = x.double(), w.double(), b.double()
    mean = x.sum(-1, keepdim=True) / x.shape[-1]
    var = ((x - mean) ** 2).sum(-1, keepdim=True) / x.shape[-1]
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean) * rstd * w + b, mean.squeeze(-1), rstd.squeeze(-1)


def layernorm_bwd(dy, x, w, eps=EPS, res=None):
    """-> (dx [+ res], dweight, dbias)"""
    dy, x, w = dy.double(), x.double(), w.double()
    D = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / D
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).sum(-1, keepdim=True) / D + eps)
    xhat = (x - mean) * rstd
    g = dy * w
    dx = rstd * (g - g.sum(-1, keepdim=True) / D - xhat * (g * xhat).sum(-1, keepdim=True) / D)
    if res is not None:
        dx = dx + res.double()
    return dx, (dy * xhat).sum(0), dy.sum(0)


def gelu(x):
    """x Phi(x), Phi by erfc: no cancellation on the negative side"""
    x = x.double()
    return 0.5 * x * torch.special.erfc(-x / math.sqrt(2.0))


def gelu_grad(x):
    """Phi(x) + x phi(x)"""
    x = x.double()
    return 0.5 * torch.special.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def swiglu_bwd(x12, dh):
    """h = silu(x1) x2 -> [d x1 | d x2] = [dh x2 s (1 + x1 (1 - s)) | dh x1 s], s = sigmoid(x1), 1 - s = sigmoid(-x1)"""
    x12, dh = x12.double(), dh.double()
    Hd = x12.shape[-1] // 2
    x1, x2 = x12[..., :Hd], x12[..., Hd:]
    s, ns = 1.0 / (1.0 + torch.exp(-x1)), 1.0 / (1.0 + torch.exp(x1))
    return torch.cat([dh * x2 * s * (1.0 + x1 * ns), dh * x1 * s], -1)


def colsum(x):
    return x.double().sum(0)


def ls_linear_finish(G, W, bias, gamma, cs, gs):
    """out = x + gamma (A W^T + b), G = dout^T A, cs = colsum(dout) -> (dW, db, dgamma); gamma None: plain Linear"""
    G = G.double()
    c = cs.double() if cs is not None else torch.zeros(G.shape[0], dtype=torch.float64)
    if gamma is None:
        return gs * G, gs * c, None
    ga = gamma.double()
    bb = bias.double() if bias is not None else torch.zeros_like(c)
    return gs * ga[:, None] * G, gs * ga * c, gs * ((W.double() * G).sum(1) + bb * c)


def im2col(img, P):
    """[B, 3, H, W] -> [B (H/P) (W/P), 3 P P], k = c P^2 + i P + j, patches row-major over the grid"""
    B, C, H, W = img.shape
    gh, gw = H // P, W // P
    return img.view(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * P * P)


def add_cls_pos(x, cls, pos):
    B, N, D = x.shape
    return torch.cat([cls.view(1, 1, D).expand(B, 1, D), x], 1) + pos.view(1, N + 1, D)


def split(x, dt):
    """fp32 -> (hi, lo): hi the 16-bit rounding, lo the 16-bit rounding of the (exact) fp32 residual"""
    hi = x.to(dt)
    return hi, (x - hi.float()).to(dt)


def round_to(v, dt):
    """float64 -> the nearest value of the 16-bit type (ties to even), as float64: ONE rounding, where a conversion by way of
    float32 would round twice"""
    bits, emin = (11, -13) if dt == torch.float16 else (8, -125)
    e = torch.frexp(v)[1].clamp(min=emin)            # v = m 2^e, 0.5 <= |m| < 1
    q = torch.exp2((e - bits).double())
    return torch.round(v / q) * q


def all_values(dt, limit=65504.0):
    """every finite value of the 16-bit type with |x| <= limit, zero-padded to a multiple of 8"""
    v = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(dt)
    v = v[torch.isfinite(v.float()) & (v.float().abs() <= limit)]
    return torch.cat([v, torch.zeros(-len(v) % 8, dtype=dt)])


# ---- dispatch rules of the host code ----------------------------------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def rowblock(R):
    """asis_rowblock_nblk: 32 rows a block, 2048 blocks at the most -> (nblk, rows per block, first empty block or None)"""
    nblk = min(cdiv(R, 32), 2048)
    rpb = cdiv(R, nblk)
    used = cdiv(R, rpb)
    return nblk, rpb, (used if used < nblk else None)


def wave_rows(R):
    """the distinct numbers of rows one wave of a 4-wave block walks (rows r0 + wave, r0 + wave + 4, ...)"""
    nblk, rpb, _ = rowblock(R)
    out = set()
    for blk in range(nblk):
        n = max(0, min(R, (blk + 1) * rpb) - blk * rpb)
        out |= {max(0, cdiv(n - w, 4)) for w in range(4)}
    return out


def ln_bwd_maxc(D):
    return 4 if D <= 1024 else (6 if D <= 1536 else 8)


def lane_trips(D):
    return cdiv(D // 4, 64)


def ln_fixed(rows, D, out_f32, form=2):
    """asis_layernorm takes layernorm_fixed_kernel"""
    return bool(form) and not out_f32 and D in (768, 1024, 1536) and rows >= 4096


def colsum_gy(C, per):
    return min(cdiv(C // per, 256), 4096)


PACK_GRID = 4096 * 256          # threads of a capped grid-stride launch of the packing kernels


# ---- case tables ------------------------------------------------------------------------------------------------------------
# LayerNorm forward, generic kernel: D = 63, 64, 65 float4 chunks against 64 lanes, the LN_MAXC limit; four rows a block.
# (rows, D, ld or None): ld = row stride of x and of the output where it is a column slice of a wider buffer
LN_D = (4, 64, 252, 256, 260, 1000, 2048)
LN_ROWS = (1, 3, 4, 5, 130)
LN_GENERIC = [(rows, D, (D + 4 if rows in (3, 130) else None)) for D in LN_D for rows in LN_ROWS]
# fixed kernel: (rows, D, ld, fixed, second row of the last wave clamped, rows in the last block of 8)
LN_FIXED = [(4096, 768, None, True, False, 8), (4097, 768, 776, True, True, 1), (4103, 768, None, True, True, 7),
            (4096, 1024, None, True, False, 8), (4097, 1024, None, True, True, 1), (4103, 1024, 1028, True, True, 7),
            (4096, 1536, 1544, True, False, 8), (4097, 1536, None, True, True, 1), (4103, 1536, None, True, True, 7),
            (4095, 1024, None, False, False, 0)]          # one row short: the generic kernel on the same input
# split_stats / layernorm_mx: all below 4096 rows; x strided for rows 5 and 130
STATS_CASES = [(rows, D, (D + 8 if rows != 1 else None)) for D in (64, 260, 2048) for rows in (1, 5, 130)]

# LayerNorm backward: (R, D, strided, MAXC, nblk, rows per block, rows a wave walks, first empty block)
LN_BWD = [
    (1, 4, False, 4, 1, 1, {0, 1}, None),            # waves 1..3 idle
    (31, 4, False, 4, 1, 31, {7, 8}, None),
    (4, 252, False, 4, 1, 4, {1}, None),             # one row a wave: a prefetch that never has a successor
    (5, 260, False, 4, 1, 5, {1, 2}, None),          # wave 0 has one prefetched successor; two lane trips
    (31, 1024, False, 4, 1, 31, {7, 8}, None),       # the last width of MAXC 4, every chunk live
    (33, 1024, False, 4, 2, 17, {4, 5}, None),       # two blocks, 17 and 16 rows
    (130, 1024, True, 4, 5, 26, {6, 7}, None),
    (1, 1028, False, 6, 1, 1, {0, 1}, None),         # the first width of MAXC 6
    (5, 1028, False, 6, 1, 5, {1, 2}, None),
    (33, 1028, True, 6, 2, 17, {4, 5}, None),
    (4, 1536, False, 6, 1, 4, {1}, None),            # MAXC 6 with every chunk live
    (130, 1536, False, 6, 5, 26, {6, 7}, None),
    (1, 1540, False, 8, 1, 1, {0, 1}, None),         # the first width of MAXC 8: no prefetch
    (5, 1540, False, 8, 1, 5, {1, 2}, None),
    (33, 2048, True, 8, 2, 17, {4, 5}, None),
    (130, 2048, False, 8, 5, 26, {6, 7}, None),
    (65537, 64, False, 4, 2048, 33, {0, 8, 9}, 1986),  # the block cap: 33-row blocks, the blocks from 1986 on empty
]

SWIGLU_CASES = [(R, Hd) for R in (1, 3, 257) for Hd in (4, 132, 4096)]

# column sums: (R, C16, C32, ld - C, nblk, rows per block, unrolled trips, tail rows, gy 16-bit, gy fp32, column trips)
_BIG16, _BIG32 = 8 * 256 * 4096 + 8, 4 * 256 * 4096 + 8
COLSUM_CASES = [
    (1, 8, 8, 0, 1, 1, 0, 1, 1, 1, 1),               # smallest shape
    (3, 8, 8, 8, 1, 3, 0, 3, 1, 1, 1),               # tail loop only
    (4, 8, 8, 0, 1, 4, 1, 0, 1, 1, 1),               # one unrolled trip, no tail
    (7, 136, 136, 8, 1, 7, 1, 3, 1, 1, 1),           # unrolled trip plus tail, ld > C
    (33, 2056, 2056, 0, 2, 17, 4, 1, 2, 3, 1),       # a partial last column block
    (65537, 64, 64, 8, 2048, 33, 8, 1, 1, 1, 1),     # cap, empty blocks, 33-row blocks = 8 unrolled + 1 tail
    (2, _BIG16, _BIG32, 0, 1, 2, 0, 2, 4096, 4096, 2),  # second trip of the column loop under the 4096 cap
]

# LayerScale o Linear finish: (N, K, lane trips, what is given)
LS_CASES = [
    (1, 4, 1, "all"), (3, 40, 1, "all"), (24, 40, 1, "all"), (5, 256, 1, "all"), (5, 260, 2, "all"), (3, 1024, 4, "all"),
    (24, 4096, 16, "all"), (1, 4096, 16, "all"),
    (5, 260, 2, "plain"), (24, 4096, 16, "plain"), (3, 40, 1, "plain"),      # gamma None: dW = gs G, db = gs cs
    (5, 260, 2, "nobias"), (3, 1024, 4, "nocs"), (5, 256, 1, "nodb"), (3, 40, 1, "nodgamma"), (1, 4, 1, "plain-nocs"),
]

# cast_pad: (rows, cols, ld_dst, ld_src, scale, part, chunks above the grid)
CAST_PAD_CASES = [
    (5, 1, 8, 1, 1.0, 0, False), (5, 7, 8, 7, 0.37, 0, False), (3, 8, 8, 12, 1.0, 0, False), (3, 8, 16, 8, 0.37, 1, False),
    (6, 9, 16, 9, 0.37, 0, False), (6, 9, 24, 13, 1.0, 1, False), (37, 588, 592, 588, 1.0, 0, False),
    (37, 588, 600, 592, 0.37, 1, False), (37, 588, 592, 588, 0.37, 0, False), (4, 7, 16, 9, 0.37, 1, False),
    (2049, 4104, 4104, 4104, 0.37, 0, True),
]
# im2col: (B, H, W, P, ldk, chunks above the grid)
IM2COL_CASES = [(2, 28, 42, 14, 592, False), (1, 42, 28, 14, 600, False), (2, 32, 48, 16, 768, False), (1, 48, 32, 16, 776, False),
                (12, 518, 518, 14, 592, True)]
# add_cls_pos: (B, N, D, float4 above the grid)
CLS_POS_CASES = [(1, 1, 4, False), (3, 16, 128, False), (2, 1369, 1536, True)]


# ---- inputs and references per case -----------------------------------------------------------------------------------------
def ln_params(D, tag):
    gen = _gen(31, D, tag)
    return 1 + 0.3 * torch.randn(D, generator=gen), 0.2 * torch.randn(D, generator=gen)


@functools.lru_cache(maxsize=2)
def ln_fwd_case(rows, D):
    """rows with a mean about 30 sigma from zero -> (x, w, b, y64, y32, mean64, rstd64, mean32, rstd32)"""
    n = 4096 if rows == 4095 else rows        # 4095 rows: the first 4095 of the 4096-row case, "the same input"
    gen = _gen(32, n, D)
    x = (0.25 * torch.randn(n, D, generator=gen) + 8 + 0.5 * torch.randn(n, 1, generator=gen))[:rows].contiguous()
    w, b = ln_params(D, 1)
    y64, mean64, rstd64 = layernorm(x, w, b)
    y32 = F.layer_norm(x, (D,), w, b, EPS)
    mean32 = x.mean(-1)
    rstd32 = (x.var(-1, unbiased=False) + EPS).rsqrt()
    return x, w, b, y64, y32, mean64, rstd64, mean32, rstd32


def _ln_autograd(dy, x, w, res, dtype):
    xx, ww = x.to(dtype).clone().requires_grad_(), w.to(dtype).clone().requires_grad_()
    bb = torch.zeros_like(ww).requires_grad_()
    F.layer_norm(xx, (x.shape[-1],), ww, bb, EPS).backward(dy.to(dtype))
    dx = xx.grad if res is None else xx.grad + res.to(dtype)
    return dx, ww.grad, bb.grad


@functools.lru_cache(maxsize=2)
def ln_bwd_case(R, D):
    """-> (dy, x, w, res, {with_res: (ref triple, float32 triple)}); the references are autograd in float32, the formula in float64"""
    gen = _gen(33, R, D)
    x = 1.5 * torch.randn(R, D, generator=gen) + 0.5 + 0.5 * torch.randn(R, 1, generator=gen)
    dy = torch.randn(R, D, generator=gen)
    res = torch.randn(R, D, generator=gen)
    w, _ = ln_params(D, 2)
    out = {}
    for with_res in (True, False):
        r = res if with_res else None
        out[with_res] = (layernorm_bwd(dy, x, w, EPS, r), _ln_autograd(dy, x, w, r, F32))
    return dy, x, w, res, out


@functools.lru_cache(maxsize=2)
def swiglu_case(R, Hd):
    """x1 over [-32, 32], its first column -100 and its last +100 (__expf overflows there); x2 and dh O(1), x2 of those two
    columns with 8 significant bits so that dh x2 is exact in fp32 and rounds to 16 bits once.  -> (x12, dh per dtype)"""
    gen = _gen(34, R, Hd)
    x1 = 64 * torch.rand(R, Hd, generator=gen) - 32
    x2 = torch.randn(R, Hd, generator=gen) + 0.25
    x1[:, 0], x1[:, -1] = -100.0, 100.0
    for c in (0, -1):
        x2[:, c] = x2[:, c].bfloat16().float()
    dh = torch.randn(R, Hd, generator=gen) + 0.25
    return torch.cat([x1, x2], 1).contiguous(), {dt: dh.to(dt) for dt in DT}


def swiglu_f32(x12, dh):
    """torch's float32 evaluation: autograd of F.silu(x1) * x2"""
    Hd = x12.shape[1] // 2
    xx = x12.clone().requires_grad_()
    (F.silu(xx[:, :Hd]) * xx[:, Hd:]).backward(dh.float())
    return xx.grad


def colsum_input(R, C, dt):
    gen = _gen(35, R, C % 100003)
    return (torch.randn(R, C, generator=gen) + 0.3).to(dt)


def ls_case(N, K, what):
    """-> dict of the operands (None where ``what`` leaves one out) and gs"""
    gen = _gen(36, N, K, len(what))
    t = dict(G=torch.randn(N, K, generator=gen), W=0.05 * torch.randn(N, K, generator=gen), bias=0.1 * torch.randn(N, generator=gen),
             gamma=0.5 + torch.rand(N, generator=gen), cs=torch.randn(N, generator=gen) * 3, gs=0.37 if N % 2 else 1.0 / 1024)
    if what.startswith("plain"):
        t["gamma"] = None
    if what == "nobias":
        t["bias"] = None
    if what.endswith("nocs"):
        t["cs"] = None
    return t


def ls_f32(t):
    """torch's float32 evaluation of dgamma"""
    c = t["cs"] if t["cs"] is not None else torch.zeros(t["G"].shape[0])
    b = t["bias"] if t["bias"] is not None else torch.zeros_like(c)
    return t["gs"] * ((t["W"] * t["G"]).sum(1) + b * c)


def gelu_grid():
    """2^20 fp32 points on [-12, 12] and the fp16 values as fp32"""
    grid = torch.linspace(-12.0, 12.0, 1 << 20, dtype=torch.float64).float()
    return torch.cat([grid, all_values(torch.float16).float()]).contiguous()


def binade(x):
    """group index of every element: floor(log2 |x|) + 1 (frexp's exponent), zeros in a group of their own"""
    e = torch.frexp(x.double().abs())[1].long()
    return torch.where(x == 0, torch.full_like(e, -5000), e)


def per_binade_max(x, v):
    """max of v >= 0 over the binade of x every element lies in, spread back to the elements"""
    uniq, inv = torch.unique(binade(x).reshape(-1), return_inverse=True)
    m = torch.zeros(len(uniq), dtype=torch.float64).scatter_reduce(0, inv, v.double().reshape(-1), "amax")
    return m[inv].view(x.shape)
