"""Low-rank adaptation (LoRA) of the ViT's attention projections: rank-r updates of the q and v thirds of ``attn.qkv``.

Per block, with D the embed dim, r the rank and ``s = alpha / r``:

    A    [2r, D]   rows 0..r = A_q, rows r..2r = A_v          (``blocks.{i}.attn.qkv.lora_A``)
    B_q  [D, r],  B_v  [D, r]                                  (``.lora_B_q`` / ``.lora_B_v``)
    u = xn A^T ;   q += s u_q B_q^T ;   v += s u_v B_v^T

The parameters belong to a ``LoRA`` object, not to the model: every ``Attention`` only gets a handle (``attn._lora``, a plain
object), so ``model.state_dict()`` and its keys stay exactly as they are.  ``Block.forward_train_rows`` / ``Block.backward``
(dinov2/layers/blocks.py) take the rank-r route when the handle is there; everything else (validation, prediction) runs the
unchanged frozen forward under ``LoRA.merged(model)``, which swaps ``W + s B A`` in for the q and v rows.

The pack builders below are plain torch and run on any device: they lay the LoRA matrices into the K-augmented operands of the
GEMMs that run anyway (P = 64 padded columns for the stacked rank dimension, 2r <= 64) and into the operands of the two kernels
of csrc/lora.hip.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, Iterator, List, Optional, Tuple

import torch
from torch import nn

from .packs import tag_of

RANKS = (4, 8, 16, 32)
PAD = 64                    # ops.LORA_PAD: padded width of the stacked rank dimension


# ---- pack builders (pure torch) ------------------------------------------------------------------------------------------
def pack_wf(W: torch.Tensor, Bq: torch.Tensor, Bv: torch.Tensor, s: float) -> torch.Tensor:
    """[3D, D + 64] = [W_qkv | s B placed]: rows 0..D, columns D..D+r hold s B_q; rows 2D..3D, columns D+r..D+2r hold s B_v;
    everything else zero.  ``[xn | u] @ pack_wf.T`` is the LoRA forward of q | k | v."""
    D, r = Bq.shape
    out = W.new_zeros((3 * D, D + PAD))
    out[:, :D] = W
    out[:D, D:D + r] = s * Bq
    out[2 * D:, D + r:D + 2 * r] = s * Bv
    return out


def pack_wbt(W: torch.Tensor, A: torch.Tensor) -> torch.Tensor:
    """[D, 3D + 64] = [W_qkv^T | A^T | 0]: ``[dqkv | du] @ pack_wbt.T = dqkv W + du A``, the input gradient"""
    D = W.shape[1]
    out = W.new_zeros((D, 3 * D + PAD))
    out[:, :3 * D] = W.t()
    out[:, 3 * D:3 * D + A.shape[0]] = A.t()
    return out


def pack_wd_fwd(A: torch.Tensor) -> torch.Tensor:
    """[64, D]: A in rows 0..2r, zero rows behind (``u = xn @ pack_wd_fwd.T``, pad columns exactly zero)"""
    out = A.new_zeros((PAD, A.shape[1]))
    out[:A.shape[0]] = A
    return out


def pack_wd_bwd(Bq: torch.Tensor, Bv: torch.Tensor, s: float) -> torch.Tensor:
    """[64, 2D] = [s B_q^T | 0 ; 0 | s B_v^T ; 0]: ``du = [dQ | dV] @ pack_wd_bwd.T = s (dQ B_q | dV B_v)``"""
    D, r = Bq.shape
    out = Bq.new_zeros((PAD, 2 * D))
    out[:r, :D] = s * Bq.t()
    out[r:2 * r, D:] = s * Bv.t()
    return out


def merged_weight(W: torch.Tensor, A: torch.Tensor, Bq: torch.Tensor, Bv: torch.Tensor, s: float) -> torch.Tensor:
    """W + s B A on the q and v rows of the [3D, D] qkv weight"""
    D, r = Bq.shape
    out = W.clone()
    out[:D] += s * (Bq @ A[:r])
    out[2 * D:] += s * (Bv @ A[r:])
    return out


def _tag(*ts) -> tuple:
    return tag_of(ts)


class LoRAHandle:
    """What an ``Attention`` sees of its LoRA parameters (a plain object: nothing is registered on the module)."""

    def __init__(self, A: nn.Parameter, Bq: nn.Parameter, Bv: nn.Parameter, rank: int, scale: float, prefix: str):
        self.A, self.Bq, self.Bv = A, Bq, Bv
        self.rank, self.scale, self.prefix = rank, scale, prefix
        self.merged_w: Optional[torch.Tensor] = None     # persistent W + s B A
        self.merged_tag = None
        self.merged_cache: dict = {}                      # the attention's pack cache while the merged weight is swapped in

    @property
    def params(self) -> Tuple[nn.Parameter, nn.Parameter, nn.Parameter]:
        return self.A, self.Bq, self.Bv

    def names(self) -> Tuple[str, str, str]:
        return self.prefix + ".lora_A", self.prefix + ".lora_B_q", self.prefix + ".lora_B_v"


class LoRA:
    """Owner of the LoRA parameters of ``model`` (a DINOv2 ViT of this package).  ``alpha`` defaults to ``rank`` (s = 1).
    Init: A kaiming-uniform(a = sqrt(5)) — uniform in +-1/sqrt(D) — from a CPU generator seeded with ``seed`` (identical on
    every data-parallel rank), B = 0: the adapted model starts as the base model."""

    def __init__(self, model, rank: int, alpha: Optional[float] = None, seed: int = 0):
        if rank not in RANKS:
            raise ValueError(f"LoRA rank must be one of {RANKS}: got {rank}")
        alpha = float(rank) if alpha is None else float(alpha)
        if not (alpha > 0.0 and math.isfinite(alpha)):
            raise ValueError(f"LoRA alpha must be positive: got {alpha}")
        self.rank, self.alpha, self.seed = int(rank), alpha, int(seed)
        self.scale = alpha / rank
        gen = torch.Generator(device="cpu")
        gen.manual_seed(self.seed)
        self.handles: List[LoRAHandle] = []
        for i, blk in enumerate(model.blocks):
            qkv = blk.attn.qkv
            D = qkv.in_features
            if qkv.out_features != 3 * D or D % 64:
                raise ValueError("LoRA: attn.qkv must be a [3D, D] projection with D % 64 == 0")
            dev = qkv.weight.device
            bound = 1.0 / math.sqrt(D)       # kaiming_uniform_(a=sqrt(5)) on [2r, D]: gain sqrt(1/3), bound = sqrt(3) gain / sqrt(D)
            A = ((torch.rand((2 * rank, D), generator=gen, dtype=torch.float32) * 2.0 - 1.0) * bound).to(dev)
            mk = lambda t: nn.Parameter(t, requires_grad=True)
            h = LoRAHandle(mk(A), mk(torch.zeros((D, rank), device=dev)), mk(torch.zeros((D, rank), device=dev)), self.rank,
                           self.scale, f"blocks.{i}.attn.qkv")
            self.handles.append(h)
        self.attach(model)

    # ---- attachment -------------------------------------------------------------------------------------------------
    def attach(self, model) -> None:
        if len(model.blocks) != len(self.handles):
            raise ValueError("LoRA.attach: the model has another depth")
        for blk, h in zip(model.blocks, self.handles):
            object.__setattr__(blk.attn, "_lora", h)      # no submodule, no parameter: state_dict() keeps its keys

    @staticmethod
    def detach(model) -> None:
        for blk in model.blocks:
            blk.attn.__dict__.pop("_lora", None)

    # ---- parameters, checkpoint entry ---------------------------------------------------------------------------------
    def named_parameters(self) -> Iterator[Tuple[str, nn.Parameter]]:
        for h in self.handles:
            yield from zip(h.names(), h.params)

    def parameters(self) -> Iterator[nn.Parameter]:
        for _, p in self.named_parameters():
            yield p

    def state_dict(self) -> dict:
        return {"rank": self.rank, "alpha": self.alpha,
                "params": {n: p.detach().float().cpu().clone() for n, p in self.named_parameters()}}

    def load_state_dict(self, entry: dict, strict: bool = True) -> str:
        if int(entry["rank"]) != self.rank or float(entry["alpha"]) != self.alpha:
            raise ValueError(f"LoRA checkpoint entry has rank {entry['rank']} / alpha {entry['alpha']}, this one {self.rank} / {self.alpha}")
        params = entry["params"]
        named = dict(self.named_parameters())
        if set(params) != set(named):
            raise ValueError("LoRA checkpoint entry names do not match this model: "
                             f"{sorted(set(params) ^ set(named))[:4]} ...")
        with torch.no_grad():
            for n, p in named.items():
                if tuple(params[n].shape) != tuple(p.shape):
                    raise ValueError(f"LoRA checkpoint entry: {n} has shape {tuple(params[n].shape)}, expected {tuple(p.shape)}")
                p.copy_(params[n].to(p.device, torch.float32))
        return "<All LoRA keys matched successfully>"

    @classmethod
    def from_state(cls, model, entry: dict) -> "LoRA":
        """the ``lora`` entry of a checkpoint -> a ``LoRA`` attached to ``model`` (prediction)"""
        lo = cls(model, int(entry["rank"]), float(entry["alpha"]))
        lo.load_state_dict(entry)
        return lo

    # ---- merged weights for every forward that is not the training step ----------------------------------------------------------
    @contextlib.contextmanager
    def merged(self, model):
        """Inside the context every block's ``attn.qkv.weight`` IS ``W + s B A`` (q and v rows): a persistent per-block tensor,
        recomputed only when A, B or W changed, swapped in through ``.data`` and swapped out again on exit (the base weight is
        never written: it comes back bit for bit).  Every re-merge bumps the weight's ``_asis_gen``, which the pack caches of
        dinov2/layers/blocks.py key on next to ``data_ptr`` and ``_version``: the merged tensor keeps its address, so without the
        bump a 16-bit pack of the previous merge would be taken for current.  The handle is taken off the attention meanwhile:
        a training forward inside the context would add the update twice."""
        if len(model.blocks) != len(self.handles):
            raise ValueError("LoRA.merged: the model has another depth")
        undo = []
        try:
            for blk, h in zip(model.blocks, self.handles):
                attn = blk.attn
                w = attn.qkv.weight
                base = w.data
                tag = _tag(w, h.A, h.Bq, h.Bv)
                if h.merged_w is None or h.merged_tag != tag:
                    with torch.no_grad():
                        m = merged_weight(base.detach().float(), h.A.detach().float(), h.Bq.detach().float(), h.Bv.detach().float(),
                                          h.scale)
                        if h.merged_w is None or h.merged_w.shape != m.shape or h.merged_w.device != m.device:
                            h.merged_w = m.contiguous()
                        else:
                            h.merged_w.copy_(m)
                    w._asis_gen = getattr(w, "_asis_gen", 0) + 1
                    h.merged_tag = _tag(w, h.A, h.Bq, h.Bv)
                undo.append((attn, w, base, attn._cache, attn.__dict__.get("_lora")))
                w.data = h.merged_w
                attn._cache = h.merged_cache
                attn.__dict__.pop("_lora", None)
            yield model
        finally:
            for attn, w, base, cache, handle in undo:
                w.data = base
                attn._cache = cache
                if handle is not None:
                    object.__setattr__(attn, "_lora", handle)


def check_engine_args(*, mode: str, train_backbone: bool, optimize_backbone: bool, layer_decay, is_mla: bool, model, rank) -> None:
    """the combinations ``SegEngine(lora_rank=...)`` refuses"""
    if rank not in RANKS:
        raise ValueError(f"lora_rank must be one of {RANKS}: got {rank}")
    if is_mla:
        raise ValueError("lora_rank: the train_mla.py flow is not built for LoRA (the train.py adapter flow is)")
    if mode != "train_adapters" or not train_backbone:
        raise ValueError("lora_rank needs mode='train_adapters' and train_backbone=True: LoRA runs the backbone's training forward")
    if optimize_backbone:
        raise ValueError("lora_rank and optimize_backbone exclude each other: with LoRA the backbone weights stay frozen")
    if layer_decay is not None:
        raise ValueError("lora_rank: layer_decay scales the learning rates of backbone weights, which LoRA does not train")
    if any(float(getattr(blk, "sample_drop_ratio", 0.0)) > 0.0 for blk in model.blocks):
        raise ValueError("lora_rank needs drop_path_rate = 0: the gathered LayerNorm of stochastic depth has no strided output")
