"""HIP-backed focal loss — API mirror of `segloss/focal_loss.py:7-91`.

``FocalLoss`` keeps the reference's constructor and call convention: ``logit`` is (B,C,H,W), class probabilities unless
``apply_nonlin`` makes them (None, ``softmax_helper`` or ``nn.Softmax(1)``: the kernel applies the softmax itself), ``target`` a
label map (B,1,H,W) or (B,H,W).  loss = mean (``size_average``) or sum over all pixels of ``-alpha[t] (1 - pt)^gamma log(pt)``,
pt = sum_c onehot_c q_c + smooth with the one-hot row clamped to [smooth/(C-1), 1-smooth] when ``smooth`` is set.  Forward and
gradient are one ``ops.hardpixel_loss`` call with K = all pixels (csrc/hardpixel.hip).  The reference moves the labels to the
host every step (`focal_loss.py:68`); nothing here leaves the device.  1 - pt is clamped at 0: the reference returns NaN where
pt lies an ulp above 1 and gamma is not an integer.  A label outside 0..C-1 costs 0 (the reference's scatter fails on it).
"""
from __future__ import annotations

import numpy as np
import torch
from torch import nn

from .. import ops
from .ND_Crossentropy import _HardPixelFn
from .dice import _labels
from .dice_loss import _nonlin_count


class FocalLoss(nn.Module):
    def __init__(self, apply_nonlin=None, alpha=None, gamma=2, balance_index=0, smooth=1e-5, size_average=True):
        super().__init__()
        self.apply_nonlin = apply_nonlin
        self.alpha = alpha
        self.gamma = gamma
        self.balance_index = balance_index
        self.smooth = smooth
        self.size_average = size_average
        self._n = _nonlin_count(apply_nonlin)
        if self.smooth is not None:
            if self.smooth < 0 or self.smooth > 1.0:
                raise ValueError('smooth value should be in [0,1]')

    def alpha_vector(self, num_class: int):
        """the [C] class factors of `focal_loss.py:51-63`, float32 on the host; None = ones"""
        alpha = self.alpha
        if alpha is None:
            return None
        if isinstance(alpha, (list, np.ndarray)):
            assert len(alpha) == num_class
            a = torch.as_tensor(np.asarray(alpha), dtype=torch.float32).reshape(num_class)
            return a / a.sum()
        if isinstance(alpha, float):
            a = torch.ones(num_class) * (1 - alpha)
            a[self.balance_index] = alpha
            return a
        raise TypeError('Not support alpha type')

    def forward(self, logit, target):
        if logit.dim() != 4:
            raise NotImplementedError("only (B,C,H,W) input is built (never called otherwise by the training scripts)")
        alpha = self.alpha_vector(logit.shape[1])
        if alpha is not None:
            alpha = alpha.to(logit.device)
        labels = _labels(target, (logit.shape[0], 1) + tuple(logit.shape[2:]))
        return _HardPixelFn.apply(logit, labels, ops.HARDPIXEL_FOCAL, labels.numel(), self._n, float(self.gamma),
                                  float(self.smooth or 0.0), alpha, bool(self.size_average))
