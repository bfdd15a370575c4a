"""Reference restatement of LoRA on the q and v projections of one DINOv2 block for the tests: torch on the CPU in whatever dtype
the inputs have (the tests pass float64, under autograd), composed from ``oracle.ref_torch``.

    u = xn A^T  (A [2r, D]: rows 0..r = A_q, r..2r = A_v);   q += s u_q B_q^T;   v += s u_v B_v^T;   s = alpha / r
"""
import torch
import torch.nn.functional as F

from oracle import ref_torch as O


def attention(x, sd, p: str, heads: int, A, Bq, Bv, s: float):
    """``O.attention`` (`dinov2/layers/attention.py:56-69`) with the low-rank terms added to q and v before the heads split"""
    B, N, C = x.shape
    hd = C // heads
    r = Bq.shape[1]
    qkv = F.linear(x, sd[p + ".qkv.weight"], sd.get(p + ".qkv.bias"))
    u = x @ A.t()
    q = qkv[..., :C] + s * (u[..., :r] @ Bq.t())
    k = qkv[..., C:2 * C]
    v = qkv[..., 2 * C:] + s * (u[..., r:] @ Bv.t())
    split = lambda t: t.reshape(B, N, heads, hd).permute(0, 2, 1, 3)
    q, k, v = split(q) * hd ** -0.5, split(k), split(v)
    attn = (q @ k.transpose(-2, -1)).softmax(dim=-1)
    o = (attn @ v).transpose(1, 2).reshape(B, N, C)
    return F.linear(o, sd[p + ".proj.weight"], sd.get(p + ".proj.bias"))


def block(xs, sd, p: str, heads: int, A, Bq, Bv, s: float):
    """One block on the stacked token batches ``xs`` = [x (b_i, N_i, D), ...] -> the list of outputs"""
    ls = lambda t, name: t * sd[name] if name in sd else t
    out = []
    for x in xs:
        x = x + ls(attention(O.layer_norm(x, sd, p + ".norm1"), sd, p + ".attn", heads, A, Bq, Bv, s), p + ".ls1.gamma")
        x = x + ls(O.mlp(O.layer_norm(x, sd, p + ".norm2"), sd, p + ".mlp"), p + ".ls2.gamma")
        out.append(x)
    return out


def run(sd, p: str, x2, dy2, segs, heads: int, A, Bq, Bv, s: float):
    """float64 autograd of sum(y * dy) -> (y, dx, dA, dB_q, dB_v) for the stacked [R, D] input ``x2``"""
    osd = {k: v.double() for k, v in sd.items() if k.startswith(p + ".")}
    xr = x2.double().clone().requires_grad_(True)
    Ar, Bqr, Bvr = (t.double().clone().requires_grad_(True) for t in (A, Bq, Bv))
    D = x2.shape[1]
    xs, r0 = [], 0
    for b, n in segs:
        xs.append(xr[r0:r0 + b * n].view(b, n, D))
        r0 += b * n
    y = torch.cat([o.reshape(-1, D) for o in block(xs, osd, p, heads, Ar, Bqr, Bvr, s)])
    (y * dy2.double()).sum().backward()
    return y.detach(), xr.grad, Ar.grad, Bqr.grad, Bvr.grad
