"""HIP-backed Lovasz-Softmax loss — API mirror of `segloss/lovasz_loss.py:7-67`.

``LovaszSoftmax`` keeps the reference's constructor and call convention: ``inputs`` are NCHW class probabilities, used as they
are, ``targets`` a label map (B,H,W) or (B,1,H,W).  The loss is taken over the whole flattened batch and over all classes.
Forward and gradient are one ``ops.lovasz_softmax`` call (a device radix sort of the per-pixel errors of every class, a scan and
a gradient pass, csrc/lovasz.hip); the module is differentiable through torch autograd.  The order of the sort is defined:
descending error, ties by ascending pixel index, so the gradient is reproducible where errors tie.

``lovasz_grad`` is the host helper under the reference's name, in closed form (float64): the reference's differences of
``1 - I/U`` cancel in float32 once the pixel count reaches millions.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from .dice import _labels


def lovasz_grad(gt_sorted: torch.Tensor) -> torch.Tensor:
    """Gradient of the Lovasz extension w.r.t. the sorted errors (Alg. 1 of the paper), float64, from integer counts:
    with G = #class pixels, f_k / b_k = #class / #other among positions 0..k, I = G - f_k, U = G + b_k:
    class pixel 1/U, other I/(U (U - 1)); G == 0: g_0 = 1 and 0 elsewhere."""
    gt = gt_sorted.reshape(-1).to(torch.int64)
    n = gt.numel()
    if n == 0:
        return torch.zeros(0, dtype=torch.float64, device=gt.device)
    G = gt.sum()
    f = gt.cumsum(0)
    b = (1 - gt).cumsum(0)
    I, U = (G - f).double(), (G + b).double()
    other = I / torch.clamp(U * (U - 1.0), min=1.0)  # U == 1 on an "other" pixel only when G == 0, k == 0 (set below)
    g = torch.where(gt > 0, 1.0 / U, other)
    if int(G) == 0:
        g = torch.zeros_like(g)
        g[0] = 1.0
    return g


class _LovaszFn(torch.autograd.Function):
    """loss(probabilities NCHW, labels [B,H,W]) through ``asis_lovasz_softmax`` (+ the resize transpose when H,W differ)."""

    @staticmethod
    def forward(ctx, prob_nchw, labels, reduction):
        q = prob_nchw.detach().permute(0, 2, 3, 1).contiguous().float()  # no copy when it is an NHWC buffer view
        loss, per_class, dz = ops.lovasz_softmax(q, labels, 0, reduction, 1.0)
        ctx.dz, ctx.hw = dz, q.shape[1:3]
        return per_class if reduction == "none" else loss.view(())

    @staticmethod
    def backward(ctx, gout):
        dz = ctx.dz * gout  # "none": one factor per class, on the last (channel) axis of NHWC
        h, w = ctx.hw
        if tuple(dz.shape[1:3]) != (h, w):
            dz, _ = ops.resize_bilinear_bwd(dz.contiguous(), h, w, torch.float32)
        return dz.permute(0, 3, 1, 2), None, None


class LovaszSoftmax(nn.Module):
    def __init__(self, reduction='mean'):
        super().__init__()
        self.reduction = reduction

    def forward(self, inputs, targets):
        if inputs.dim() == 5:
            raise NotImplementedError("5-D (volumetric) input is not built (never used by the training scripts)")
        if inputs.dim() != 4:
            raise ValueError("LovaszSoftmax: inputs must be (B,C,H,W) probabilities")
        reduction = self.reduction if self.reduction in ("none", "sum") else "mean"  # the reference's else branch
        return _LovaszFn.apply(inputs, _labels(targets, inputs.shape), reduction)
