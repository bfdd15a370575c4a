"""HIP-backed knowledge-distillation loss (no counterpart in the reference's `segloss/`).

``DistillationLoss(temperature, flips)`` is the soft-target term of Hinton et al. (2015) for dense prediction, evaluated at the
size the hard loss is evaluated at: with p = softmax(resize(student) / T) and q = the mean over the teacher's views of
softmax(resize(view) / T), loss = T^2 mean over the pixels of KL(q || p).  ``logit`` is (B,C,h,w) like the input of every other loss
here; ``teacher`` one (B,C,h_k,w_k) map or a list of up to 8, each of its own size (a teacher with another head, views at other
scales); ``flips[k]`` tells that view k was predicted from the mirrored frame.  ``size``: (H, W), an int or a tensor whose last two
dimensions are H, W (the target); None = the student's own h, w.  Forward and gradient are one ``ops.distill_loss`` call
(csrc/distill.hip); the backward goes through the resize transpose (``ops.resize_bilinear_bwd``) when H, W differ from h, w.  No
gradient reaches the teacher.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops


def _nhwc(x: torch.Tensor) -> torch.Tensor:
    return x.detach().permute(0, 2, 3, 1).contiguous().float()  # no copy when it is an NHWC buffer view


class _SoftTargetFn(torch.autograd.Function):
    """loss(NCHW student logits) against NCHW teacher maps through ``op(student, teachers, size) -> (loss, dz)``, both NHWC:
    ``ops.distill_loss`` here, ``ops.consistency_loss`` in consistency.py (+ the resize transpose when H,W differ)"""

    @staticmethod
    def forward(ctx, x_nchw, teachers, size, op):
        x = _nhwc(x_nchw)
        loss, dz = op(x, [_nhwc(t) for t in teachers], tuple(x.shape[1:3]) if size is None else size)
        ctx.dz, ctx.hw = dz, x.shape[1:3]
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        dz = ctx.dz
        h, w = ctx.hw
        if tuple(dz.shape[1:3]) != (h, w):
            dz, _ = ops.resize_bilinear_bwd(dz, h, w, torch.float32)
        return (dz.permute(0, 3, 1, 2) * gout,) + (None,) * 3


class DistillationLoss(nn.Module):
    def __init__(self, temperature=1.0, flips=None):
        super().__init__()
        if not float(temperature) > 0.0:
            raise ValueError("temperature must be > 0")
        self.temperature = float(temperature)
        self.flips = None if flips is None else [bool(f) for f in flips]

    def forward(self, logit, teacher, size=None):
        if logit.dim() != 4:
            raise NotImplementedError("only (B,C,H,W) input is built")
        teachers = [teacher] if torch.is_tensor(teacher) else list(teacher)
        return _SoftTargetFn.apply(logit, teachers, size,
                                   lambda x, ts, sz: ops.distill_loss(x, ts, sz, flips=self.flips, temperature=self.temperature))
