"""Host draws of batch mixing (CutMix, Yun et al. 2019 / CutMix-Seg, French et al. 2020; ClassMix, Olsson et al. 2021): which
sample of the batch gives pixels to which, and where.  The device side is ``ops.mix_batch`` (csrc/mix.hip).

``MixSampler(kind, p, seed, num_classes, background).draw(B, H, W, step, rank)`` is stateless: every draw comes from a
``numpy.random.RandomState`` seeded by (seed, rank, step), so a resumed run repeats the draws of the run it resumes and every rank
draws its own.  The tables (CPU tensors):

    donor int32 [B]     one shift r per step, uniform in 1..B-1: donor[b] = (b + r) mod B — nobody is their own donor
    kind  int32 [B]     0 not mixed, 1 CutMix, 2 ClassMix; each sample is mixed with probability p, independently
    box   int32 [B,4]   (y0, x0, y1, x1), half-open: the box of the CutMix paper (lambda ~ U(0,1), cut ratio sqrt(1 - lambda), centre
                        uniform over the frame, clipped to it); drawn for every sample, read for kind 1
    order uint8 [B,16]  a permutation of 0..15 per sample: the order in which ClassMix picks half of the donor's classes; only
                        its entries < num_classes matter

With B = 1 nothing is mixed (kind is 0).  The streams of the four tables do not depend on ``kind`` or ``p``.

``draw(..., groups=)`` (a host int sequence of B entries; default None: the tables above, bit for bit): donors stay inside their
group — semi-supervised training mixes labelled frames among themselves and unlabelled frames among themselves.  In the place of
the one shift, one shift per group of more than one member is drawn, the groups in ascending id: with m_0 < m_1 < ... the n
members of a group and r uniform in 1..n-1, donor[m_i] = m_{(i + r) mod n}.  A group of one is not mixed (kind 0, its own donor).
The other three tables are drawn after the shifts exactly as without groups.
"""
from __future__ import annotations

import numpy as np
import torch

KINDS = {"cutmix": 1, "classmix": 2}
MAX_CLASSES = 16  # MAXC of csrc/bilinear_tap.h: the width of a class bit set and of a row of ``order``


class MixSampler:
    def __init__(self, kind: str, p: float = 1.0, seed: int = 0, num_classes: int = 2, background: bool = False):
        if kind not in KINDS:
            raise ValueError(f"mix must be one of {sorted(KINDS)}, got {kind!r}")
        if not 0.0 <= float(p) <= 1.0:
            raise ValueError(f"mix_p={p} must be in [0, 1]")
        if not 1 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"num_classes={num_classes} must be in 1..{MAX_CLASSES}")
        self.kind, self.p, self.seed = kind, float(p), int(seed)
        self.num_classes, self.background = int(num_classes), bool(background)

    def draw(self, B: int, H: int, W: int, step: int, rank: int = 0, groups=None) -> dict:
        B, H, W = int(B), int(H), int(W)
        if B < 1 or H < 1 or W < 1 or int(step) < 0 or int(rank) < 0:
            raise ValueError(f"draw: need B, H, W >= 1 and step, rank >= 0 (B={B} H={H} W={W} step={step} rank={rank})")
        r = np.random.RandomState([self.seed & 0xFFFFFFFF, int(rank) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF])
        if groups is None:
            shift = int(r.randint(1, B)) if B > 1 else 0
            donor = (np.arange(B) + shift) % B
            alone = np.full(B, B == 1)
        else:
            gid = np.asarray(groups).astype(np.int64).reshape(-1)
            if gid.shape[0] != B:
                raise ValueError(f"draw: groups has {gid.shape[0]} entries, the batch {B} samples")
            donor, alone = np.arange(B), np.zeros(B, dtype=bool)
            for g in np.unique(gid):   # ascending
                members = np.nonzero(gid == g)[0]
                n = len(members)
                if n == 1:
                    alone[members] = True
                    continue
                donor[members] = members[(np.arange(n) + int(r.randint(1, n))) % n]
        mixed = r.uniform(size=B) < self.p
        kind = np.where(mixed & ~alone, KINDS[self.kind], 0)
        ratio = np.sqrt(1.0 - r.uniform(size=B))
        ch, cw = (H * ratio).astype(np.int64), (W * ratio).astype(np.int64)
        cy, cx = r.randint(0, H, size=B), r.randint(0, W, size=B)
        box = np.stack([np.clip(cy - ch // 2, 0, H), np.clip(cx - cw // 2, 0, W), np.clip(cy + ch // 2, 0, H),
                        np.clip(cx + cw // 2, 0, W)], axis=1)
        order = np.stack([r.permutation(MAX_CLASSES) for _ in range(B)])
        return {"donor": torch.from_numpy(donor.astype(np.int32)), "kind": torch.from_numpy(kind.astype(np.int32)),
                "box": torch.from_numpy(box.astype(np.int32)), "order": torch.from_numpy(order.astype(np.uint8))}
