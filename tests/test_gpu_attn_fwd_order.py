"""attn_fwd_pipe_kernel: the speculative tile order (exponentials against the running maximum as it stands, the row sums decide
whether the maximum is formed at all) against the max-first order (ASIS_ATTN_MAXFIRST=1) -- bit for bit -- and both against a
float64 softmax attention, on scores built to reach every branch; the decision itself is emulated on the CPU
(scripts/attn_fwd_ab.py: emulate_decision)."""
import importlib.util
import os

import pytest
import torch

from adaptersis_amd import ops
from tests.conftest import rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("attn_fwd_ab", os.path.join(ROOT, "scripts", "attn_fwd_ab.py"))
ab = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ab)

H = 2
C_FOLD = 0.125 * 1.4426950408889634
KINDS = ["small", "rescale_each", "slow_no_rescale", "threshold", "overflow"]
# (name, folded, V row-major, dtype); "mx": the MX form of the second output plane
FORMS = [("fold_vt", True, False, torch.float16), ("plain_vt", False, False, torch.float16),
         ("fold_rows", True, True, torch.float16), ("plain_rows", False, True, torch.float16),
         ("fold_rows_mx", True, True, torch.float16), ("fold_vt", True, False, torch.bfloat16)]
SHAPES = [(2, 64), (2, 65), (1, 129), (2, 200)]  # 65: a tail tile with one valid key; 129, 200: one / two tiles in between


def next_up(x: float, dt) -> float:
    t = torch.tensor([x], dtype=dt)
    return float((t.view(torch.int16) + 1).view(dt))


def scores(kind: str, B: int, N: int, dt, seed: int):
    """-> q', k, v float [B, N, H, 64], already rounded to ``dt``; q' . k = the score in log2 units.  Apart from "small", q' is
    (1, 0, ..) for even and (0.5, 0, ..) for odd queries, so that k[.., 0] IS the score row of the even queries (exactly: a
    sum with one non-zero term) and the odd ones see half of it: lanes of one wave on both sides of every decision."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, N, H, 64, generator=g)
    if kind == "small":  # deviation 0.4: no tile after the first one leaves the fast path
        q = torch.randn(B, N, H, 64, generator=g) * 0.224
        k = torch.randn(B, N, H, 64, generator=g) * 0.224
    else:
        q = torch.zeros(B, N, H, 64)
        q[:, 0::2, :, 0], q[:, 1::2, :, 0] = 1.0, 0.5
        tile = (torch.arange(N) // 64).float()
        if kind == "rescale_each":      # the row maximum rises by 8 (4 for the odd queries) at every tile
            s = 8.0 * tile[None, :, None] - torch.rand(B, N, H, generator=g)
        elif kind == "slow_no_rescale":  # first tile: maximum 0; later tiles 1 .. 5 above it, sums far above 48, never above 6
            s = torch.where(tile[None, :, None] == 0, -torch.rand(B, N, H, generator=g), 1.0 + 4.0 * torch.rand(B, N, H, generator=g))
            s[:, 7] = 0.0
        elif kind == "threshold":       # exactly 6 above in tile 1 (no rescale: the comparison is strict), the next float in tile 2
            s = -1.0 - torch.rand(B, N, H, generator=g)
            s[:, 7] = 0.0
            if N > 64 + 9:
                s[:, 64 + 9] = 6.0
            if N > 128 + 30:
                s[:, 128 + 30] = next_up(6.0, dt)
        else:                           # overflow: exp2(200) is inf in the speculative pass
            s = -torch.rand(B, N, H, generator=g)
            if N > 64:
                s[:, min(64 + 40, N - 1)] = 200.0
        k = torch.zeros(B, N, H, 64)
        k[..., 0] = s
        k[..., 1:] = torch.randn(B, N, H, 63, generator=g)  # q' is zero there
    return q.to(dt).float(), k.to(dt).float(), v.to(dt).float()


def reference(q, k, v, c):
    """float64 softmax attention on the 16-bit operands; c: what multiplies q . k to give log2 units"""
    qd, kd, vd = (t.double().permute(0, 2, 1, 3) for t in (q, k, v))
    s2 = (qd @ kd.transpose(-1, -2)) * c
    ref = (torch.softmax(s2 * 0.6931471805599453, -1) @ vd).permute(0, 2, 1, 3).reshape(-1, H * 64)
    return ref, torch.logsumexp(s2 * 0.6931471805599453, -1) * 1.4426950408889634


_cases = {}


def case(kind, B, N, dt, folded):
    """operands and float64 reference, built once per (kind, shape, dtype, folded)"""
    key = (kind, B, N, dt, folded)
    if key not in _cases:
        q, k, v = scores(kind, B, N, dt, 100 + KINDS.index(kind))
        if not folded:  # the kernel multiplies by scale * log2(e) itself
            q = (q / C_FOLD).to(dt).float()
        _cases[key] = (q, k, v) + reference(q, k, v, 1.0 if folded else C_FOLD)
    return _cases[key]


def run(dev, form, dt, segs, q, k, v, maxfirst):
    """one launch over the stacked segments -> (out, second plane or None, lse or None)"""
    _, folded, rows, _ = form
    D = H * 64
    os.environ["ASIS_ATTN_MAXFIRST"] = "1" if maxfirst else "0"
    try:
        R = q.shape[0]
        q, k, v = (t.to(dev).to(dt) for t in (q, k, v))
        o = torch.empty((R, D), device=dev, dtype=dt)
        o_lo = torch.empty_like(o)
        one = len(segs) == 1
        lse = torch.empty((segs[0][0], H, segs[0][1]), device=dev, dtype=torch.float32) if one else None
        scale = None if folded else 0.125
        if rows:
            qkv = torch.cat([q, k, v], dim=1).contiguous()
            amax = v.float().abs().max().reshape(1) if form[0].endswith("_mx") else None
            ops.attention_fwd_qkv(qkv, list(segs), H, scale, o, out_lo=o_lo, lse=lse, mx_amax=amax)
        else:
            qk = torch.cat([q, k], dim=1).contiguous()
            ld = (max(n for _, n in segs) + 63) // 64 * 64
            vt = torch.full((sum(b for b, _ in segs), D, ld), float("nan"), device=dev, dtype=dt)  # pad columns: anything
            r0 = b0 = 0
            for B, N in segs:
                vt[b0:b0 + B, :, :N] = v[r0:r0 + B * N].view(B, N, D).transpose(1, 2)
                r0, b0 = r0 + B * N, b0 + B
            if one:
                ops.attention_fwd(qk[:, :D], qk[:, D:], vt, segs[0][0], H, segs[0][1], scale, out=o, lse=lse, out_lo=o_lo)
            else:
                (B1, N1), (B2, N2) = segs
                ops.attention_fwd_seg(qk[:, :D], qk[:, D:], vt, B1, N1, B2, N2, H, scale, out=o, out_lo=o_lo)
        torch.cuda.synchronize()
        return o, o_lo, lse
    finally:
        os.environ.pop("ASIS_ATTN_MAXFIRST", None)


def check(dev, form, kind, segs, q, k, v, ref, lse_ref):
    name, folded, rows, dt = form
    new, old = (run(dev, form, dt, segs, q, k, v, mf) for mf in (False, True))
    tag = f"{name} {dt} {kind} {segs}"
    # identity: output, second plane, log-sum-exp
    assert torch.equal(new[0], old[0]), f"{tag}: outputs differ between the two orders"
    assert torch.equal(new[1], old[1]), f"{tag}: second output planes differ between the two orders"
    assert new[2] is None or torch.equal(new[2], old[2]), f"{tag}: log-sum-exp differs between the two orders"
    # correctness, the bounds of tests/test_gpu_kernels.py (test_attention_fwd_prescaled / _qkv_row_major_v)
    o, o_lo, lse = new
    assert torch.isfinite(o.float()).all(), tag
    err = rel_l2(o, ref)
    msg = f"{tag}: rel-L2 {err:.2e}"
    if not name.endswith("_mx"):
        err_split = rel_l2(o.double() + o_lo.double(), ref)
        msg += f" split {err_split:.2e}"
    if lse is not None:
        err_lse = float((lse.cpu().double() - lse_ref).abs().max())
        msg += f" lse {err_lse:.2e}"
    print(msg)
    assert err < (1e-3 if dt == torch.float16 else 1e-2), msg
    if not name.endswith("_mx"):
        assert err_split < (4e-4 if dt == torch.float16 else 4e-3), msg
    if lse is not None:
        assert err_lse < 2e-3, msg


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"{f[0]}-{str(f[3])[6:]}")
def test_orders_agree_and_match_float64(dev, form):
    for kind in KINDS:
        for B, N in SHAPES:
            q, k, v, ref, lse_ref = case(kind, B, N, form[3], form[1])
            check(dev, form, kind, [(B, N)], *(t.reshape(B * N, H * 64) for t in (q, k, v)), ref, lse_ref)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"{f[0]}-{str(f[3])[6:]}")
def test_orders_agree_two_segments(dev, form):
    """both stacked token batches in one launch: (1, 129) and (1, 128)"""
    for kind in KINDS:
        parts = [case(kind, 1, N, form[3], form[1]) for N in (129, 128)]
        q, k, v = (torch.cat([p[i].reshape(-1, H * 64) for p in parts]) for i in range(3))
        check(dev, form, kind, [(1, 129), (1, 128)], q, k, v, torch.cat([p[3] for p in parts]), None)


@pytest.mark.parametrize("kind", KINDS + ["gaussian5"])
def test_sum_test_never_passes_where_max_first_rescales(kind):
    """host side: the emulated wave-level decision on the inputs above and on Gaussian scores of deviation 5 (log2 units)"""
    if kind == "gaussian5":
        g = torch.Generator().manual_seed(5)
        a = (5.0 / 8.0) ** 0.5
        q, k = ((torch.randn(2, 1765, H, 64, generator=g) * a).half().float() for _ in range(2))
    else:
        q, k, _ = scores(kind, 2, 200, torch.float16, 100 + KINDS.index(kind))
    c = ab.emulate_decision(q.permute(0, 2, 1, 3), k.permute(0, 2, 1, 3))
    print(kind, ab.shares(c))
    assert c["tiles"] > 0 and c["fast"] + c["slow"] + c["rescale"] + c["unsound"] == c["tiles"]
    assert c["unsound"] == 0
    # the inputs reach the branch they are named after
    want = {"small": "fast", "rescale_each": "rescale", "slow_no_rescale": "slow", "threshold": "rescale", "overflow": "rescale",
            "gaussian5": "rescale"}[kind]
    assert c[want] > 0
    if kind in ("small", "slow_no_rescale"):
        assert c[want] == c["tiles"]
    if kind == "threshold":
        assert c["slow"] > 0  # tile 1: exactly 6 above, not more
