"""Self-adaptive confidence thresholds for the consistency term (FreeMatch, Wang et al. 2023), kept on the device with no host
synchronisation: a global threshold tau that follows the teacher's mean confidence, scaled per class by a moving average ptilde of
the teacher's class distribution,

    tau <- m tau + (1 - m) S_conf / cnt,   ptilde_c <- m ptilde_c + (1 - m) S_c / cnt,   thr_c = fp32(tau ptilde_c / max ptilde)

with S_c, S_conf, cnt the sums of ``ops.confidence_stats`` over the batch (all ranks' batches: the sums are all-reduced), and
tau = ptilde_c = 1 / C to start with.  Kernels: csrc/adapt.hip (libasis_adapt.so, opened by the first ``update``)."""
from __future__ import annotations

from typing import Optional

import torch

from . import ops, parallel


class AdaptiveThreshold:
    """``thresholds``: fp32 [C] on ``device``, what ``ops.consistency_loss(class_threshold=)`` reads; ``state``: float64 [C + 2] =
    tau, n_updates, ptilde[C]; ``sums``: float64 [C + 2], the statistics of the last ``update`` (after the all-reduce)."""

    def __init__(self, num_classes: int, momentum: float = 0.999, device=None, process_group=None):
        if isinstance(num_classes, bool) or not isinstance(num_classes, int) or not 1 <= num_classes <= ops.ADAPT_MAX_CLASSES:
            raise ValueError(f"AdaptiveThreshold: num_classes={num_classes!r} must be an int in 1..{ops.ADAPT_MAX_CLASSES}")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"AdaptiveThreshold: momentum={momentum} must be in [0, 1)")
        self.num_classes, self.momentum, self.process_group = num_classes, float(momentum), process_group
        C = num_classes
        self.state = torch.tensor([1.0 / C, 0.0] + [1.0 / C] * C, dtype=torch.float64).to(device)
        self.thresholds = torch.full((C,), 1.0 / C, dtype=torch.float64).float().to(device)   # tau ptilde_c / max ptilde = 1 / C
        self.sums = torch.zeros((C + 2,), dtype=torch.float64).to(device)
        self._scratch = None

    def update(self, maps, flips, size, temperature: float = 1.0, sample_weight: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The statistics of the teacher's ``maps`` (``ops.confidence_stats``), their sum over the ranks, one step of the
        recursion -> ``thresholds`` (the same tensor every time, updated in place).  No host sync."""
        maps = [maps] if torch.is_tensor(maps) else list(maps)
        size = tuple(size.shape[-2:]) if torch.is_tensor(size) else ((size, size) if isinstance(size, int) else tuple(size))
        need = ops.confidence_stats_scratch_bytes(maps[0].shape[0] * int(size[0]) * int(size[1]))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty((need,), device=self.state.device, dtype=torch.uint8)
        ops.confidence_stats(maps, size, flips=flips, temperature=temperature, sample_weight=sample_weight, out=self.sums,
                             scratch=self._scratch)
        if parallel.collectives_on(self.process_group):
            torch.distributed.all_reduce(self.sums, group=self.process_group)
        return ops.adaptive_threshold_update(self.sums, self.state, self.thresholds, self.momentum)

    def state_dict(self) -> dict:
        """host copies: what a checkpoint keeps"""
        return {"state": self.state.detach().cpu().clone(), "thresholds": self.thresholds.detach().cpu().clone(),
                "momentum": self.momentum}

    def load_state_dict(self, sd: dict) -> None:
        state, thr = sd["state"], sd["thresholds"]
        if tuple(state.shape) != tuple(self.state.shape) or tuple(thr.shape) != tuple(self.thresholds.shape):
            raise ValueError(f"AdaptiveThreshold: the saved state is for {state.numel() - 2} classes, this one for {self.num_classes}")
        self.state.copy_(state.to(torch.float64))
        self.thresholds.copy_(thr.to(torch.float32))
