"""Reference restatement of stochastic depth in DINOv2's subset form (`dinov2/layers/block.py:89-138`) for the tests: torch on
the CPU in whatever dtype the inputs have (the tests pass float64), composed from ``oracle.ref_torch``.

A branch specification is one ``(indices, alpha)`` per stacked token batch (segment), as ``adaptersis_amd.droppath`` produces:
``out = x`` and, on the kept samples in their drawn order, ``out += alpha * branch(x_kept)`` through ``index_add``.
"""
import torch

from oracle import ref_torch as O


def kept_rows(segs, spec) -> torch.Tensor:
    """rows of the stacked [R, D] matrix that the kept samples occupy, in the order of the compact matrix"""
    rows, r0 = [], 0
    for (b, n), (idx, _) in zip(segs, spec):
        for i in idx:
            rows.extend(range(r0 + i * n, r0 + (i + 1) * n))
        r0 += b * n
    return torch.tensor(rows, dtype=torch.long)


def row_alphas(segs, spec) -> torch.Tensor:
    """alpha of every row of the compact matrix (float64)"""
    out = []
    for (b, n), (idx, alpha) in zip(segs, spec):
        out.extend([float(alpha)] * (len(idx) * n))
    return torch.tensor(out, dtype=torch.float64)


def segment_chunks(segs, spec):
    """[(first compact row, end, alpha)] per segment that kept something"""
    out, c0 = [], 0
    for (b, n), (idx, alpha) in zip(segs, spec):
        if idx:
            out.append((c0, c0 + len(idx) * n, float(alpha)))
            c0 += len(idx) * n
    return out


def drop_add_residual(x: torch.Tensor, branch, keep) -> torch.Tensor:
    """x (b, N, D); ``keep`` = (indices, alpha) or None (nothing dropped) -> x + alpha * branch(x[indices]) scattered back"""
    if keep is None:
        return x + branch(x)
    idx, alpha = keep
    if len(idx) == 0:
        return x
    idx = torch.as_tensor(list(idx), dtype=torch.long)
    res = branch(x[idx])
    return torch.index_add(x.flatten(1), 0, idx, res.flatten(1), alpha=float(alpha)).view_as(x)


def block(xs, sd, p: str, heads: int, keep):
    """One block on the stacked token batches ``xs`` = [x (b_i, N_i, D), ...]; ``keep`` = (keep_attn, keep_ffn), each a list
    with one (indices, alpha) per batch, or None for a branch that drops nothing.  -> the list of outputs."""
    ka, kf = keep
    ls = lambda t, name: t * sd[name] if name in sd else t
    attn = lambda t: ls(O.attention(O.layer_norm(t, sd, p + ".norm1"), sd, p + ".attn", heads), p + ".ls1.gamma")
    ffn = lambda t: ls(O.mlp(O.layer_norm(t, sd, p + ".norm2"), sd, p + ".mlp"), p + ".ls2.gamma")
    out = []
    for i, x in enumerate(xs):
        x = drop_add_residual(x, attn, None if ka is None else ka[i])
        x = drop_add_residual(x, ffn, None if kf is None else kf[i])
        out.append(x)
    return out
