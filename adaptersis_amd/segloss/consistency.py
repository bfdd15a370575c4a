"""HIP-backed consistency loss of teacher-student (mean-teacher) training (no counterpart in the reference's `segloss/`).

``ConsistencyLoss(temperature, threshold, flips)`` is ``DistillationLoss`` with the confidence gate of the UA-MT / FixMatch family
and a per-sample weight: with p = softmax(resize(student) / T), q = the mean over the teacher's views of softmax(resize(view) / T)
and m = [max_c q_c >= threshold], loss = T^2 sum over the pixels of w_b m KL(q || p) / N — normalised by the number of pixels N,
not by the number the gate keeps.  The gate looks at q at the temperature of the loss: gate on the T = 1 distribution by training at
T = 1, the default.  ``logit`` is (B,C,h,w); ``teacher`` one (B,C,h_k,w_k) map or a list of up to 8, each of its own size;
``flips[k]`` tells that view k was predicted from the mirrored frame.  ``size``: (H, W), an int or a tensor whose last two
dimensions are H, W (the target); None = the student's own h, w.  ``sample_weight``: fp32 [B] on the device, finite and >= 0.
Forward and gradient are one ``ops.consistency_loss`` call (csrc/consist.hip); the backward goes through the resize transpose
(``ops.resize_bilinear_bwd``) when H, W differ from h, w.  ``last_kept`` holds the device count (int32 [1]) of the pixels the gate let
through in the last forward.  No gradient reaches the teacher.  ``mix`` = (sel, donor): the loss over a batch mixed by
``ops.mix_batch`` — the teacher's maps are read from sample donor[b] where sel is set (``ops.consistency_loss``); sel has the
size the loss is evaluated at.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from .distill import _SoftTargetFn


class ConsistencyLoss(nn.Module):
    def __init__(self, temperature=1.0, threshold=None, flips=None):
        super().__init__()
        if not float(temperature) > 0.0:
            raise ValueError("temperature must be > 0")
        if threshold is not None and not float(threshold) <= 1.0:
            raise ValueError("threshold must be at most 1 (None or <= 0 keeps every pixel)")
        self.temperature = float(temperature)
        self.threshold = None if threshold is None else float(threshold)
        self.flips = None if flips is None else [bool(f) for f in flips]
        self.last_kept = None

    def forward(self, logit, teacher, size=None, sample_weight=None, mix=None):
        if logit.dim() != 4:
            raise NotImplementedError("only (B,C,H,W) input is built")
        teachers = [teacher] if torch.is_tensor(teacher) else list(teacher)

        def op(x, ts, sz):
            loss, self.last_kept, dz = ops.consistency_loss(x, ts, sz, flips=self.flips, temperature=self.temperature,
                                                            threshold=self.threshold, sample_weight=sample_weight, mix=mix)
            return loss, dz

        return _SoftTargetFn.apply(logit, teachers, size, op)
