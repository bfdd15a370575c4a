"""Stochastic depth of the unfrozen ViT, host side: the random draws and the index tables of the row kernels in
csrc/droppath.hip.

Semantics (restated from the published DINOv2: `dinov2/layers/block.py:89-138`, `drop_path.py`), per residual branch
(attention, then FFN) and per stacked token batch of ``b`` samples, with the block's rate ``p``:

* ``p > 0.1`` (subset mode): keep ``k = max(int(b * (1 - p)), 1)`` samples, the first ``k`` of a random permutation of
  ``range(b)`` in drawn order; ``alpha = b / k``.
* ``0 < p <= 0.1`` (DropPath mode): every sample is kept with probability ``1 - p`` independently; ``alpha = 1 / (1 - p)``.
  The kept list may be empty or full.
* ``out = x`` and, on the kept samples, ``out += alpha * ls(branch(norm(x_kept)))``.

The draws come from a host generator (no device sync).  **Draw order** of ``DropPathSampler.plan``: block-major; inside a
block the attention branch before the FFN branch; inside a branch the segments in order.  Subset mode draws one
``Generator.permutation(b)`` per segment, DropPath mode one ``Generator.random(b)`` (sample ``j`` is kept when its number
is ``>= p``).  A block with rate 0 draws nothing and gets ``None``.

``pack`` turns the plan of one step into the kernels' tables: all of them in ONE pinned host buffer, sent to the device
in ONE non-blocking copy; a ``BranchKeep`` holds a view of its slice.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

SUBSET_THRESHOLD = 0.1     # `block.py:92,103`: sample_drop_ratio > 0.1 -> the subset form, else DropPath


def block_rates(drop_path_rate: float, depth: int, uniform: bool = False) -> List[float]:
    """the per-block rates of `vision_transformer.py:103-106`: uniform, or fp32 linspace(0, r, depth) as Python floats"""
    r = float(drop_path_rate)
    if not 0.0 <= r < 1.0:
        raise ValueError(f"drop_path_rate must be in [0, 1): got {drop_path_rate}")
    if uniform:
        return [r] * depth
    return [x.item() for x in torch.linspace(0, r, depth, device="cpu")]   # on the host even under a device context


def keep_count(b: int, p: float) -> int:
    """samples the subset form keeps of ``b`` (`block.py:126`), in Python float arithmetic as written there"""
    return max(int(b * (1 - p)), 1)


class BranchKeep:
    """The kept samples of ONE residual branch over the stacked token batches ``segs``: the compact segment list the GEMMs and
    the attention run on, and the device table of the row kernels (include/asis_hip.h: 3K + 3S + 2 int32 words)."""
    __slots__ = ("segs", "K", "S", "rows", "rows_c", "tab", "spec")

    def __init__(self, segs, K, S, rows, rows_c, tab, spec):
        self.segs, self.K, self.S, self.rows, self.rows_c, self.tab, self.spec = segs, K, S, rows, rows_c, tab, spec

    @property
    def empty(self) -> bool:
        return self.K == 0


def branch_words(segs: Sequence[Tuple[int, int]], spec) -> Tuple[np.ndarray, list, int, int, int, int]:
    """``spec`` = one ``(indices, alpha)`` per segment -> (table words int32, compact segs, K, S, rows, rows_c)."""
    if len(spec) != len(segs):
        raise ValueError("drop path: one (indices, alpha) per stacked token batch expected")
    cpre, src, alpha, spre, cpos, salpha, csegs = [0], [], [], [0], [], [], []
    row0 = 0
    for (b, n), (idx, a) in zip(segs, spec):
        idx = [int(i) for i in idx]
        if len(set(idx)) != len(idx) or any(i < 0 or i >= b for i in idx):
            raise ValueError(f"drop path: kept samples must be distinct and within range({b}): {idx}")
        pos = {}
        for i in idx:
            pos[i] = cpre[-1]
            src.append(row0 + i * n)
            alpha.append(float(a))
            cpre.append(cpre[-1] + n)
        for j in range(b):
            spre.append(spre[-1] + n)
            cpos.append(pos.get(j, -1))
            salpha.append(float(a))
        if idx:
            csegs.append((len(idx), n))
        row0 += b * n
    if row0 >= 2 ** 31:
        raise ValueError("drop path: the index tables hold rows as int32")
    K, S = len(src), len(cpos)
    words = np.concatenate([np.asarray(cpre, np.int32), np.asarray(src, np.int32), np.asarray(alpha, np.float32).view(np.int32),
                            np.asarray(spre, np.int32), np.asarray(cpos, np.int32), np.asarray(salpha, np.float32).view(np.int32)])
    assert words.size == 3 * K + 3 * S + 2
    return words, csegs, K, S, row0, cpre[-1]


def pack(plan, segs, device):
    """``plan`` (``DropPathSampler.plan``, or explicit lists of the same form) -> per block ``None`` or ``(BranchKeep attn,
    BranchKeep ffn)``.  One pinned buffer, one non-blocking host-to-device copy for the whole step."""
    segs = [(int(b), int(n)) for b, n in segs]
    metas, chunks, off = [], [], 0
    for entry in plan:
        if entry is None:
            metas.append(None)
            continue
        pair = []
        for spec in entry:
            words, csegs, K, S, rows, rows_c = branch_words(segs, spec)
            pair.append((off, words.size, csegs, K, S, rows, rows_c, spec))
            chunks.append(words)
            off += words.size
        metas.append(pair)
    if not chunks:
        return metas
    device = torch.device(device)
    host = torch.empty(off, dtype=torch.int32, pin_memory=device.type == "cuda")
    host.numpy()[:] = np.concatenate(chunks)
    dev = host.to(device, non_blocking=True)
    out = []
    for pair in metas:
        out.append(None if pair is None else
                   tuple(BranchKeep(csegs, K, S, rows, rows_c, dev[o:o + n], spec) for o, n, csegs, K, S, rows, rows_c, spec in pair))
    return out


def as_branch_keeps(keep, segs, device):
    """``keep`` of one block as ``Block.forward_train_rows`` takes it: ``None``, a packed ``(BranchKeep, BranchKeep)``, or explicit
    ``(keep_attn, keep_ffn)`` lists (one ``(indices, alpha)`` per segment; a branch ``None`` = nothing dropped there), which
    are packed here — a convenience for tests and one-off calls: an engine packs the whole step at once."""
    if keep is None:
        return None, None
    ka, kf = keep
    out = []
    for k in (ka, kf):
        if k is None or isinstance(k, BranchKeep):
            out.append(k)
        else:
            out.append(pack([(k, k)], segs, device)[0][0])
    return tuple(out)


class DropPathSampler:
    """The draws of stochastic depth for one engine: a ``numpy.random.Generator`` seeded with ``(seed, rank)``, so every
    data-parallel rank drops its own samples.  ``rates``: one rate per block."""

    def __init__(self, rates: Sequence[float], seed: int = 0, rank: int = 0):
        self.rates = [float(r) for r in rates]
        if any(not 0.0 <= r < 1.0 for r in self.rates):
            raise ValueError("drop path rates must be in [0, 1)")
        self.seed, self.rank = int(seed), int(rank)
        self.rng = np.random.default_rng([self.seed, self.rank])

    @property
    def active(self) -> bool:
        return any(r > 0.0 for r in self.rates)

    def _branch(self, p: float, segs):
        spec = []
        for b, _ in segs:
            if p > SUBSET_THRESHOLD:
                k = keep_count(b, p)
                spec.append(([int(i) for i in self.rng.permutation(b)[:k]], b / k))
            else:
                u = self.rng.random(b)
                spec.append(([j for j in range(b) if u[j] >= p], 1.0 / (1.0 - p)))
        return spec

    def plan(self, segs):
        """-> per block ``None`` (rate 0) or ``(keep_attn, keep_ffn)``, each one ``(indices, alpha)`` per segment of ``segs``.
        Draw order: block-major, attention before FFN, segments in order (module docstring)."""
        segs = [(int(b), int(n)) for b, n in segs]
        return [None if p == 0.0 else (self._branch(p, segs), self._branch(p, segs)) for p in self.rates]

    def step(self, segs, device):
        """the packed plan of one training step (``pack(self.plan(segs), ...)``)"""
        return pack(self.plan(segs), segs, device)
