"""HIP-backed mirror of `segloss/ND_Crossentropy.py:11-47`."""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from .dice import seg_loss


class CrossentropyND(nn.Module):
    """Mean (optionally class-weighted) cross entropy over all pixels of NCHW logits ("network has to have NO
    NONLINEARITY")."""

    def __init__(self, weight=None):
        super().__init__()
        self.weight = weight

    def forward(self, inp, target):
        return seg_loss(inp, target, 0, ops.LOSS_NONE, 0.0, n_ce=1, ce_weight=self.weight)


class _HardPixelFn(torch.autograd.Function):
    """loss(NCHW logits or probabilities, labels [B,H,W]) through ``asis_hardpixel_loss`` (+ the resize transpose when H,W
    differ): the mean or sum of the K largest per-pixel losses of the whole batch."""

    @staticmethod
    def forward(ctx, x_nchw, labels, kind, K, n_softmax, gamma, smooth, weight, size_average):
        x = x_nchw.detach().permute(0, 2, 3, 1).contiguous().float()  # no copy when it is an NHWC buffer view
        loss, dz = ops.hardpixel_loss(x, labels, kind, K, n_softmax=n_softmax, gamma=gamma, smooth=smooth, class_weight=weight,
                                      size_average=size_average)
        ctx.dz, ctx.hw = dz, x.shape[1:3]
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        dz = ctx.dz
        h, w = ctx.hw
        if tuple(dz.shape[1:3]) != (h, w):
            dz, _ = ops.resize_bilinear_bwd(dz, h, w, torch.float32)
        return (dz.permute(0, 3, 1, 2) * gout,) + (None,) * 8


def _weight_on(weight, device):
    return None if weight is None else torch.as_tensor(weight).detach().float().contiguous().to(device)


class TopKLoss(CrossentropyND):
    """`ND_Crossentropy.py:34-47`: the per-pixel cross entropy of NCHW logits ("network has to have NO NONLINEARITY"), of which
    the largest ``k`` percent of the whole batch are averaged; ``target`` is (B,1,H,W) and read as ``target[:, 0]``.  A radix
    select on the device, no sort (csrc/hardpixel.hip); ties at the threshold go to the lower pixel index.  Pixels labelled
    ``ignore_index`` (any label outside 0..C-1) cost 0 and still count in the number of pixels, as in the reference."""

    def __init__(self, weight=None, ignore_index=-100, k=10):
        super().__init__(weight)
        self.k, self.ignore_index = k, ignore_index

    def forward(self, inp, target):
        if inp.dim() != 4:
            raise NotImplementedError("only (B,C,H,W) input is built (5-D volumetric input is never used by the training scripts)")
        C = inp.shape[1]
        if 0 <= self.ignore_index < C:
            raise NotImplementedError("an ignore_index inside 0..C-1 is not built (the kernel ignores labels outside that range)")
        target = target[:, 0].long().contiguous()
        num_voxels = target.numel()
        K = int(num_voxels * self.k / 100)
        if K == 0:
            raise ValueError(f"TopKLoss: k={self.k} selects none of the {num_voxels} pixels (the reference returns NaN)")
        return _HardPixelFn.apply(inp, target, ops.HARDPIXEL_CE, K, 0, 0.0, 0.0, _weight_on(self.weight, inp.device), True)
