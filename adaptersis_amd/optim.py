"""Flat fp32 parameter / gradient buckets, the HIP SGD step and the fused HIP AdamW step.

``FlatBucket`` re-points the parameters of the trainable modules at views of ONE contiguous fp32
buffer (and their ``.grad`` at views of a second one), ordered so that gradients become complete
front-to-back during the backward pass.  That gives: one ``asis_sgd_momentum`` launch per step, RCCL
all-reduces over contiguous ranges with no packing copies, and ``state_dict`` / checkpoint
compatibility (parameters stay ``nn.Parameter`` objects with their reference key names).

``SGD`` mirrors ``torch.optim.SGD`` as configured in `train.py:178-191` / `train_mla.py:178-183`
(momentum, weight decay, dampening 0, no Nesterov; ``param_groups[i]["lr"]`` is what
``CosineAnnealingLR`` mutates).

``AdamW`` has the same surface and is ``torch.optim.AdamW`` behind ``torch.nn.utils.clip_grad_norm_`` over ALL buckets, as the
DINOv2 half of the reference trains its transformer (`dinov2/train/train.py:62,250-259`: AdamW, gradient clipping, no weight
decay on 1-D parameters, layer-wise learning-rate decay) — three launches per step (csrc/adamw.hip), no host synchronisation.

``EMA`` keeps an exponential moving average of the buckets an optimizer steps, one fp32 shadow per bucket, updated behind the
optimizer's step and skipped with it on the device (csrc/ema.hip); ``ema_decay_at`` is its decay schedule on the host.
"""
from __future__ import annotations

import math
import re
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import torch
from torch import nn

from . import ops


class FlatBucket:
    def __init__(self, named_params: Sequence[Tuple[str, nn.Parameter]], momentum: bool = True):
        named_params = [(n, p) for n, p in named_params if p.requires_grad]
        if not named_params:
            raise ValueError("FlatBucket: no trainable parameters")
        dev = named_params[0][1].device
        self.names = [n for n, _ in named_params]
        self.params = [p for _, p in named_params]
        sizes = [p.numel() for p in self.params]
        # 16-byte align every tensor inside the bucket
        offs, o = [], 0
        for s in sizes:
            offs.append(o)
            o += (s + 3) // 4 * 4
        self.numel = o
        self.offsets = offs
        self.flat = torch.zeros(o, device=dev, dtype=torch.float32)
        self.grad = torch.zeros(o, device=dev, dtype=torch.float32)
        # gradient-only buckets (parameters that are all-reduced but never optimised) carry no momentum buffer
        self.momentum = torch.zeros(o, device=dev, dtype=torch.float32) if momentum else None
        with torch.no_grad():
            for p, off in zip(self.params, offs):
                v = self.flat[off:off + p.numel()].view(p.shape)
                v.copy_(p.detach().float())
                p.data = v
                p.grad = self.grad[off:off + p.numel()].view(p.shape)
        self.views: Dict[str, torch.Tensor] = {n: p.grad for n, p in zip(self.names, self.params)}

    def range_of(self, names: Iterable[str]) -> Tuple[int, int]:
        idx = [self.names.index(n) for n in names]
        lo = min(self.offsets[i] for i in idx)
        hi = max(self.offsets[i] + (self.params[i].numel() + 3) // 4 * 4 for i in idx)
        return lo, hi


class SGD:
    """``torch.optim.SGD``-shaped optimizer over FlatBuckets (one kernel launch per bucket and step)."""

    def __init__(self, buckets: Sequence[FlatBucket], lr: float, momentum: float = 0.0, weight_decay: float = 0.0):
        self.buckets = list(buckets)
        self.param_groups: List[dict] = [{"params": b.params, "lr": lr, "initial_lr": lr, "momentum": momentum,
                                          "weight_decay": weight_decay, "dampening": 0, "nesterov": False}
                                         for b in self.buckets]
        self._steps = 0
        # overflow guard of the static loss scale (config.loss_scale, 16-bit gradient tensors): a step whose all-reduced
        # gradients hold an inf / NaN is skipped on the device — no host sync; ``skipped_steps`` reads the counter
        self.guard = torch.zeros(2, device=self.buckets[0].flat.device, dtype=torch.int32) \
            if self.buckets and self.buckets[0].flat.is_cuda else None

    @property
    def skipped_steps(self) -> int:
        return 0 if self.guard is None else int(self.guard[1].item())

    def zero_grad(self, set_to_none: bool = False):
        pass  # every gradient element is overwritten by the backward kernels each step

    def step(self, inv_scale: float = 1.0):
        if self.guard is not None:
            for i, b in enumerate(self.buckets):
                ops.grad_guard(b.grad, self.guard, i == 0)
        for i, (b, g) in enumerate(zip(self.buckets, self.param_groups)):
            ops.sgd_momentum(b.flat, b.grad, b.momentum, g["lr"], g["momentum"], g["weight_decay"], inv_scale,
                             self._steps == 0, self.guard, count_skip=(i == 0))
            for p in b.params:  # changed in place behind torch's back: invalidate the packed 16-bit copies
                p._asis_gen = getattr(p, "_asis_gen", 0) + 1
        self._steps += 1

    def state_dict(self):
        return {"state": {i: {"momentum_buffer": b.momentum.clone()} for i, b in enumerate(self.buckets)},
                "steps": self._steps,
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    def load_state_dict(self, sd):
        # validate first (a `torch.optim.SGD` entry of a reference checkpoint holds per-parameter buffers): nothing is
        # modified when the entry does not fit, and `restart_from_checkpoint` reports + skips it
        state = sd.get("state", {})
        bufs = []
        for i, b in enumerate(self.buckets):
            ent = state.get(i, state.get(str(i)))
            mb = ent.get("momentum_buffer") if isinstance(ent, dict) else None
            if not torch.is_tensor(mb) or mb.numel() != b.numel:
                raise ValueError(f"optimizer state does not match flat bucket {i} ({b.numel} elements): not written by "
                                 "adaptersis_amd.optim.SGD with the same trainable set")
            bufs.append(mb)
        if len(sd.get("param_groups", [])) != len(self.param_groups):
            raise ValueError("optimizer state has a different number of parameter groups")
        for b, mb in zip(self.buckets, bufs):
            b.momentum.copy_(mb.reshape(-1))
        self._steps = int(sd.get("steps", 1))
        for g, s in zip(self.param_groups, sd["param_groups"]):
            g.update(s)


_TOKEN_PARAMS = ("cls_token", "pos_embed", "mask_token", "register_tokens")
_BLOCK_RE = re.compile(r"^blocks\.(?:\d+\.)?(\d+)\.")   # blocks.<i>.* (or blocks.<chunk>.<i>.* of a chunked DINOv2 ViT)
MAX_GROUPS = 256                                         # a group code is one byte


def param_groups_for(names: Sequence[str], shapes: Sequence[Sequence[int]], *, weight_decay: float, no_decay: bool = True,
                     layer_decay: Optional[float] = None, depth: Optional[int] = None) -> Tuple[List[int], List[Tuple[float, float]]]:
    """Per-parameter hyper-parameter groups of ``AdamW`` -> (group index per parameter, table of (lr_scale, weight_decay)).

    ``no_decay``: parameters with ``ndim <= 1`` (biases, LayerNorm / BatchNorm weights, LayerScale ``gamma``) and the token /
    position parameters (``cls_token``, ``pos_embed``, ``mask_token``, ``register_tokens``) get weight decay 0.
    ``layer_decay = d`` with ``depth = L`` (backbone names): ``blocks.i.*`` trains at ``lr * d ** (L - i)``, the patch and token
    embeddings at ``d ** (L + 1)``, the final ``norm.*`` and every other name at 1 (`dinov2/utils/param_groups.py`).
    Pure Python: no tensor is touched.  More than 256 distinct groups raise (the kernel's group code is one byte)."""
    if len(names) != len(shapes):
        raise ValueError("param_groups_for: names and shapes differ in length")
    if layer_decay is not None and (depth is None or depth < 1):
        raise ValueError("param_groups_for: layer_decay needs depth = the number of transformer blocks")
    index, table, where = [], [], {}
    for name, shape in zip(names, shapes):
        leaf = name.rsplit(".", 1)[-1]
        wd = float(weight_decay)
        if no_decay and (len(tuple(shape)) <= 1 or leaf in _TOKEN_PARAMS):
            wd = 0.0
        scale = 1.0
        if layer_decay is not None:
            m = _BLOCK_RE.match(name)
            if m:
                i = int(m.group(1))
                if i >= depth:
                    raise ValueError(f"param_groups_for: {name} lies outside depth={depth}")
                scale = float(layer_decay) ** (depth - i)
            elif name in _TOKEN_PARAMS or name.startswith("patch_embed."):
                scale = float(layer_decay) ** (depth + 1)
        key = (scale, wd)
        if key not in where:
            if len(table) == MAX_GROUPS:
                raise ValueError(f"param_groups_for: more than {MAX_GROUPS} distinct (lr_scale, weight_decay) groups")
            where[key] = len(table)
            table.append(key)
        index.append(where[key])
    return index, table


def quad_codes(bucket: FlatBucket, index: Sequence[int]) -> torch.Tensor:
    """uint8 [bucket.numel / 4] on the CPU: the group of the parameter every 4-element quad of the bucket belongs to (a
    ``FlatBucket`` aligns every tensor to 4 elements, so no quad straddles two); padding quads carry 0 and stay zero whatever
    their group, because their gradient, moments and values are zero."""
    codes = torch.zeros(bucket.numel // 4, dtype=torch.uint8)
    for off, p, gi in zip(bucket.offsets, bucket.params, index):
        codes[off // 4:(off + p.numel() + 3) // 4] = int(gi)
    return codes


class AdamW:
    """``torch.optim.AdamW`` (decoupled decay, ``amsgrad=False``) behind ``clip_grad_norm_(max_norm=clip_grad)`` over all
    buckets together, shaped like ``SGD`` above: per step one ``asis_grad_sumsq`` per bucket (gradient norm AND overflow check: it
    replaces the ``asis_grad_guard`` pass), one ``asis_adamw_prepare``, one ``asis_adamw_step`` per bucket; no host sync.

    ``bucket.momentum`` is ``exp_avg``.  The step count lives on the device (``guard[2]``): the host never learns whether a step
    was skipped.  ``layer_decay``: one value for every bucket, or one per bucket (``None`` = no layer decay there)."""

    def __init__(self, buckets: Sequence[FlatBucket], lr: float, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.01, clip_grad: Optional[float] = None, no_decay: bool = True,
                 layer_decay: Union[None, float, Sequence[Optional[float]]] = None, depth: Optional[int] = None):
        self.buckets = list(buckets)
        if not self.buckets:
            raise ValueError("AdamW: no buckets")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or eps <= 0.0:
            raise ValueError("AdamW: betas must lie in [0, 1) and eps must be positive")
        if clip_grad is not None and clip_grad <= 0.0:
            raise ValueError("AdamW: clip_grad must be positive (None: no clipping)")
        if any(b.momentum is None for b in self.buckets):
            raise ValueError("AdamW: a gradient-only bucket (momentum=False) cannot be optimised")
        decays = list(layer_decay) if isinstance(layer_decay, (list, tuple)) else [layer_decay] * len(self.buckets)
        if len(decays) != len(self.buckets):
            raise ValueError("AdamW: layer_decay needs one entry per bucket")
        dev = self.buckets[0].flat.device
        self.clip_grad = clip_grad
        self.param_groups: List[dict] = []
        self.exp_avg_sq, self.codes, self.lr_scale, self.weight_decay = [], [], [], []
        for b, d in zip(self.buckets, decays):
            index, table = param_groups_for(b.names, [tuple(p.shape) for p in b.params], weight_decay=weight_decay,
                                            no_decay=no_decay, layer_decay=d, depth=depth if d is not None else None)
            self.param_groups.append({"params": b.params, "lr": lr, "initial_lr": lr, "betas": tuple(betas), "eps": eps,
                                      "weight_decay": weight_decay, "group_table": [tuple(t) for t in table]})
            self.exp_avg_sq.append(torch.zeros_like(b.flat))
            self.codes.append(quad_codes(b, index).to(b.flat.device))
            self.lr_scale.append(torch.tensor([t[0] for t in table], dtype=torch.float32, device=b.flat.device))
            self.weight_decay.append(torch.tensor([t[1] for t in table], dtype=torch.float32, device=b.flat.device))
        counts = [ops.grad_sumsq_blocks(b.numel) for b in self.buckets]
        self._part_off = [sum(counts[:i]) for i in range(len(counts) + 1)]
        self.partials = torch.zeros(self._part_off[-1], device=dev, dtype=torch.float32)
        self.guard = torch.zeros(3, device=dev, dtype=torch.int32)     # skip flag, skipped steps, step count
        self.record = torch.zeros(4, device=dev, dtype=torch.float32)  # clip coefficient, 1/(1-b1^t), 1/sqrt(1-b2^t), norm

    @property
    def skipped_steps(self) -> int:
        return int(self.guard[1].item())

    @property
    def step_count(self) -> int:
        """steps applied so far (skipped ones do not count).  A host read: it waits for the device."""
        return int(self.guard[2].item())

    @property
    def last_grad_norm(self) -> float:
        """unscaled global gradient norm of the last step that was not skipped, before clipping.  A host read: it waits
        for the device (the training loop reads it next to the loss, which it synchronises on anyway)."""
        return float(self.record[3].item())

    def zero_grad(self, set_to_none: bool = False):
        pass  # every gradient element is overwritten by the backward kernels each step

    def step(self, inv_scale: float = 1.0):
        for i, b in enumerate(self.buckets):
            ops.grad_sumsq(b.grad, self.partials[self._part_off[i]:self._part_off[i + 1]])
        b1, b2 = self.param_groups[0]["betas"]
        ops.adamw_prepare(self.partials, self.guard, self.record, inv_scale, self.clip_grad, b1, b2)
        for i, (b, g) in enumerate(zip(self.buckets, self.param_groups)):
            ops.adamw_step(b.flat, b.grad, b.momentum, self.exp_avg_sq[i], self.codes[i], self.lr_scale[i], self.weight_decay[i],
                           g["lr"], b1, b2, g["eps"], inv_scale, self.guard, self.record)
            for p in b.params:  # changed in place behind torch's back: invalidate the packed 16-bit copies
                p._asis_gen = getattr(p, "_asis_gen", 0) + 1

    def state_dict(self):
        return {"state": {i: {"exp_avg": b.momentum.clone(), "exp_avg_sq": v.clone()}
                          for i, (b, v) in enumerate(zip(self.buckets, self.exp_avg_sq))},
                "step": self.step_count,
                "param_groups": [{k: v for k, v in g.items() if k != "params"} for g in self.param_groups]}

    def load_state_dict(self, sd):
        # validate first: an `optim.SGD` entry (momentum_buffer) or a `torch.optim.AdamW` one (per-parameter tensors, per-parameter
        # steps) does not fit; nothing is modified then, and `restart_from_checkpoint` reports + skips it
        state = sd.get("state", {}) if isinstance(sd, dict) else None
        if not isinstance(state, dict) or isinstance(sd.get("step"), bool) or not isinstance(sd.get("step"), int):
            raise ValueError("optimizer state was not written by adaptersis_amd.optim.AdamW (no flat state / device step count)")
        groups = sd.get("param_groups", [])
        if len(groups) != len(self.param_groups) or len(state) != len(self.buckets):
            raise ValueError("optimizer state has a different number of buckets / parameter groups")
        bufs = []
        for i, (b, g) in enumerate(zip(self.buckets, groups)):
            ent = state.get(i, state.get(str(i)))
            m = ent.get("exp_avg") if isinstance(ent, dict) else None
            v = ent.get("exp_avg_sq") if isinstance(ent, dict) else None
            if not torch.is_tensor(m) or not torch.is_tensor(v) or m.numel() != b.numel or v.numel() != b.numel:
                raise ValueError(f"optimizer state does not match flat bucket {i} ({b.numel} elements): not written by "
                                 "adaptersis_amd.optim.AdamW with the same trainable set")
            table = g.get("group_table") if isinstance(g, dict) else None
            if table is None or len(table) != len(self.param_groups[i]["group_table"]):
                raise ValueError(f"optimizer state of bucket {i} has a different group table")
            bufs.append((m, v))
        for i, (b, (m, v)) in enumerate(zip(self.buckets, bufs)):
            b.momentum.copy_(m.reshape(-1))
            self.exp_avg_sq[i].copy_(v.reshape(-1))
        self.guard[2] = int(sd["step"])
        for i, (g, s) in enumerate(zip(self.param_groups, groups)):
            g.update(s)
            g["betas"], g["group_table"] = tuple(g["betas"]), [tuple(t) for t in g["group_table"]]
            self.lr_scale[i].copy_(torch.tensor([t[0] for t in g["group_table"]], dtype=torch.float32))
            self.weight_decay[i].copy_(torch.tensor([t[1] for t in g["group_table"]], dtype=torch.float32))


def ema_decay_at(t: int, decay: float, warmup: bool = True) -> float:
    """The decay ``EMA`` applies at its ``t``-th update (t = 1, 2, ...): ``min(decay, (1 + t) / (10 + t))`` with ``warmup`` (the
    average follows the weights closely while they still move fast), else ``decay``.  The host restatement of what
    ``asis_ema_prepare`` computes on the device, in the same double arithmetic; for tests and logs."""
    t = int(t)
    if t < 1:
        raise ValueError("ema_decay_at: updates count from 1")
    d = float(decay)
    return min(d, (1.0 + t) / (10.0 + t)) if warmup else d


def consistency_ramp(t: int, rampup: int) -> float:
    """The ramp-up of the consistency weight in mean-teacher training (Tarvainen & Valpola 2017): ``exp(-5 (1 - min(t, R) / R)^2)``
    for ``R = rampup`` > 0 steps, t = 0, 1, ... the number of training steps so far — e^-5 at t = 0, rising monotonically, exactly
    1 from t = R on; 1 for R = 0 (no ramp-up).  A plain host function: ``SegEngine.train_step`` multiplies ``distill_weight`` by
    it."""
    t, R = int(t), int(rampup)
    if t < 0 or R < 0:
        raise ValueError("consistency_ramp: t and rampup count from 0")
    if R == 0 or t >= R:
        return 1.0
    return math.exp(-5.0 * (1.0 - t / R) ** 2)


class EMA:
    """Exponential moving average of the parameters in ``buckets``: one fp32 shadow per bucket, ``shadow += (1 - d_t) (flat -
    shadow)`` after every optimizer step, with ``d_t = ema_decay_at(t, decay, warmup)`` and t the number of updates APPLIED.

    ``guard``: the optimizer's guard tensor (``SGD.guard`` / ``AdamW.guard``; element 0 is the skip flag of its last step).  A step
    the optimizer skipped on the device is skipped here too, and does not count, without the host learning of it: ``update()`` is
    one ``asis_ema_prepare`` plus one ``asis_ema_update`` per bucket on the current stream (csrc/ema.hip), no host sync.
    Gradient-only buckets (``momentum=False``) are not averaged: nothing steps them.  Buffers (BatchNorm running statistics) are
    not parameters and are not averaged either."""

    def __init__(self, buckets: Sequence[FlatBucket], decay: float, warmup: bool = True, guard: Optional[torch.Tensor] = None):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError(f"EMA: decay must lie in (0, 1): got {decay}")
        self.buckets = [b for b in buckets if b.momentum is not None]
        if not self.buckets:
            raise ValueError("EMA: no bucket that an optimizer steps")
        self.decay, self.warmup, self.guard = decay, bool(warmup), guard
        dev = self.buckets[0].flat.device
        self.shadows = [b.flat.detach().clone() for b in self.buckets]
        self.state = torch.zeros(1, device=dev, dtype=torch.int32)      # updates applied
        self.record = torch.zeros(2, device=dev, dtype=torch.float32)   # 1 - decay of this update, apply flag
        self._live = None                                               # the parameters' own views while ``swapped`` is active

    @property
    def updates(self) -> int:
        """updates applied so far (skipped steps do not count).  A host read: it waits for the device."""
        return int(self.state[0].item())

    @property
    def swapped_in(self) -> bool:
        return self._live is not None

    def update(self):
        ops.ema_prepare(self.guard, self.state, self.record, self.decay, self.warmup)
        for b, e in zip(self.buckets, self.shadows):
            ops.ema_update(e, b.flat, self.record)

    def reset(self):
        """restart the average from the current weights (a resume from a checkpoint without an average)"""
        for b, e in zip(self.buckets, self.shadows):
            e.copy_(b.flat)
        self.state.zero_()

    def named_shadows(self) -> Iterable[Tuple[str, nn.Parameter, torch.Tensor]]:
        """(bucket name, parameter, its view of the shadow) for every averaged parameter"""
        for b, e in zip(self.buckets, self.shadows):
            for n, p, off in zip(b.names, b.params, b.offsets):
                yield n, p, e[off:off + p.numel()].view(p.shape)

    def swap_in(self):
        """Point ``p.data`` of every averaged parameter at its view of the shadow.  The address changes, so every pack keyed by
        ``packs.tag_of`` rebuilds; the live weights are not written."""
        if self._live is not None:
            raise RuntimeError("EMA: the averaged weights are already swapped in")
        self._live = []
        for _, p, view in self.named_shadows():
            self._live.append((p, p.data))
            p.data = view

    def swap_out(self):
        if self._live is None:
            return
        for p, data in self._live:
            p.data = data
        self._live = None

    def state_dict(self):
        return {"decay": self.decay, "warmup": self.warmup, "updates": self.updates,
                "state": {i: {"shadow": e.clone()} for i, e in enumerate(self.shadows)}}

    def load_state_dict(self, sd):
        # validate first, like the optimizers: nothing is modified when the entry does not fit
        state = sd.get("state") if isinstance(sd, dict) else None
        upd = sd.get("updates") if isinstance(sd, dict) else None
        if not isinstance(state, dict) or isinstance(upd, bool) or not isinstance(upd, int) or upd < 0:
            raise ValueError("EMA state was not written by adaptersis_amd.optim.EMA (no flat shadows / update count)")
        if len(state) != len(self.buckets):
            raise ValueError("EMA state has a different number of buckets")
        bufs = []
        for i, b in enumerate(self.buckets):
            ent = state.get(i, state.get(str(i)))
            e = ent.get("shadow") if isinstance(ent, dict) else None
            if not torch.is_tensor(e) or e.numel() != b.numel:
                raise ValueError(f"EMA state does not match flat bucket {i} ({b.numel} elements): not written by "
                                 "adaptersis_amd.optim.EMA with the same trainable set")
            bufs.append(e)
        for e, src in zip(self.shadows, bufs):
            e.copy_(src.reshape(-1))
        self.state[0] = upd
