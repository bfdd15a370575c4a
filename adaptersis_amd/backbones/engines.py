"""Engine entry points of the MI355X build (the reference's `backbones/engines.py` only holds the
unused ``pre_vit`` patch-embed clone, which is kept here for API parity).

``SegEngine`` is the fused form of the step body that the reference writes inline in
`train.py:268-436` (and copies into `validate_network`, `train.py:465-612`):

    encoder -> ViT pass A (cls + pos-embed, last-4 normed features) -> ViT pass B (raw patch tokens,
    blocks[0:-3]) -> 4 x [block, CAViT, CACNN, + pass-A feature] -> decoder input assembly ->
    FeatureDecoder -> resize + softmax + DC (softmax again) -> backward of the decoder (the only
    part of the graph that receives gradients: SURVEY.md fact 1) -> gradient all-reduce (RCCL,
    launched per decoder stage on a side stream as soon as that stage's gradients exist) -> SGD.

Everything is a HIP kernel from libasis_hip.so; torch provides device memory, streams and
``torch.distributed``.  No autograd graph is built: the engine calls the same functional cores
(`FeatureDecoder._forward_core/_backward_core`) that the reference-shaped modules wrap in
``torch.autograd.Function``.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist
from torch import nn

from .. import config, ops
from .. import lora as lora_mod
from ..dinov2.layers.blocks import _Packed, _pack, run_blocks
from ..droppath import DropPathSampler
from ..optim import EMA, SGD, AdamW, FlatBucket, consistency_ramp
from ..parallel import StageReducer, world_size
from .adapter_blocks import CACNN, CAViT, deform_inputs


class pre_vit(_Packed):
    """`backbones/engines.py:4-60`: (B, C, H, W) -> (B, N, D) patch embedding, Conv2d(k = s = patch).
    Unused by every reference script; implemented as an implicit-GEMM conv for completeness."""

    def __init__(self, img_size=84, patch_size=14, in_chans=256, embed_dim=384, norm_layer=None, flatten_embedding=True):
        super().__init__()
        if norm_layer is not None:
            raise ValueError("pre_vit: norm_layer is never set in the reference")
        self.img_size, self.patch_size = img_size, patch_size
        self.patches_resolution = (img_size // patch_size, img_size // patch_size)
        self.num_patches = self.patches_resolution[0] * self.patches_resolution[1]
        self.in_chans, self.embed_dim, self.flatten_embedding = in_chans, embed_dim, flatten_embedding
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)
        self.norm = nn.Identity()

    def forward(self, x):
        B, C, H, W = x.shape
        P = self.patch_size
        assert H % P == 0, f"Input image height {H} is not a multiple of patch height {P}"
        assert W % P == 0, f"Input image width {W} is not a multiple of patch width: {P}"
        dt = config.operand_dtype
        x16 = ops.cast_pad(x.permute(0, 2, 3, 1).contiguous().float().view(B * H * W, C), C, dt).view(B, H, W, C)
        w16 = _pack(self._cache, "w", self.proj.weight, lambda p: ops.pack_conv_weight(p.float().contiguous(), 0, dt))
        out = ops.conv_gemm(x16, w16, P, P, P, 0, bias_n=self._f32("b", self.proj.bias))
        out = out.view(B, (H // P) * (W // P), self.embed_dim)
        if not self.flatten_embedding:
            out = out.reshape(-1, H // P, W // P, self.embed_dim)
        return out


def _loss_scratch(engine, attr: str, need: int, device) -> torch.Tensor:
    """the scratch of a sort / select loss, kept on the engine between steps"""
    scratch = getattr(engine, attr, None)
    if scratch is None or scratch.numel() < need or scratch.device != device:
        scratch = torch.empty((need,), device=device, dtype=torch.uint8)
        setattr(engine, attr, scratch)
    return scratch


def loss_and_dz(engine, logits: torch.Tensor, target: torch.Tensor, S: float):
    """The loss stage of every engine's ``train_step``: logits fp32 NHWC [B,h,w,C], target int64 [B,H,W] ->
    (loss [1], dz fp32 [B,H,W,C] = S * d loss / d resized logits) for ``engine.loss_kind``, a key of ``SegEngine.LOSSES``.
    No host sync.  The Lovasz and the hard-pixel losses keep their scratch on the engine between steps.  Where the engine's step
    has an ignore value (``SegEngine(ignore_index=)`` or an unlabelled sample: ``engine._hard_ignore``) the fused family goes
    through ``ops.seg_loss_ignore`` and the valid pixels per sample are left in ``engine.last_hard_valid``."""
    n_region, lmode, eps, n_ce = SegEngine.LOSSES[engine.loss_kind]
    g = getattr(engine, "_hard_ignore", None)
    if g is not None:
        if lmode in (ops.LOSS_LOVASZ, ops.LOSS_TOPK, ops.LOSS_FOCAL):
            raise ValueError(f"loss {engine.loss_kind!r} has no ignore label: {SegEngine.IGNORE_LOSSES} have one")
        loss, dz, engine.last_hard_valid, _ = ops.seg_loss_ignore(logits, target, g, n_region, lmode, eps, n_ce, None, S)
        return loss, dz
    if lmode not in (ops.LOSS_LOVASZ, ops.LOSS_TOPK, ops.LOSS_FOCAL):
        loss, coef, _ = ops.seg_loss_fwd(logits, target, n_region, lmode, eps, n_ce, None, S)
        return loss, ops.seg_loss_bwd(logits, target, coef, n_region, lmode, n_ce, None)
    if lmode != ops.LOSS_LOVASZ:
        N = target.numel()
        scratch = _loss_scratch(engine, "_hardpixel_scratch", ops.hardpixel_scratch_bytes(N), logits.device)
        if lmode == ops.LOSS_FOCAL:   # FocalLoss(gamma)(softmax(out)): every pixel, alpha = ones, smooth 1e-5
            return ops.hardpixel_loss(logits, target, ops.HARDPIXEL_FOCAL, N, n_softmax=n_region,
                                      gamma=getattr(engine, "focal_gamma", 2.0), grad_scale=S, scratch=scratch)
        K = int(N * getattr(engine, "topk_percent", 10.0) / 100)   # TopKLoss: int(num_voxels * k / 100)
        if K < 1:
            raise ValueError(f"topk_percent selects no pixel of {N}")
        dz, dc = None, None
        if n_region:  # SoftDiceLoss(apply_nonlin=softmax_helper) half: its dz is the buffer the top-k gradient is added into
            dc, coef, _ = ops.seg_loss_fwd(logits, target, n_region, ops.LOSS_SOFTDICE, eps, 0, None, S)
            dz = ops.seg_loss_bwd(logits, target, coef, n_region, ops.LOSS_SOFTDICE, 0, None)
        loss, dz = ops.hardpixel_loss(logits, target, ops.HARDPIXEL_CE, K, grad_scale=S, dz=dz, scratch=scratch)
        return (loss if dc is None else dc.add_(loss)), dz
    scratch = _loss_scratch(engine, "_lovasz_scratch", ops.lovasz_scratch_bytes(target.numel(), logits.shape[-1]), logits.device)
    dz, ce = None, None
    if n_ce:  # CrossentropyND half: its dz is the buffer the Lovasz gradient is added into
        ce, coef, _ = ops.seg_loss_fwd(logits, target, 0, ops.LOSS_NONE, eps, n_ce, None, S)
        dz = ops.seg_loss_bwd(logits, target, coef, 0, ops.LOSS_NONE, n_ce, None)
    loss, _, dz = ops.lovasz_softmax(logits, target, n_region, "mean", S, dz=dz, scratch=scratch)
    return (loss if ce is None else ce.add_(loss)), dz


def loss_head(engine, logits: torch.Tensor, target: torch.Tensor):
    """The loss of every engine's ``train_step`` -> (loss [1], dz, target as the contiguous int64 the loss kernels read).  ``dz`` may
    still receive further terms (``SegEngine._add_consistency``) before ``logit_gradient`` takes it to the head."""
    target = target.long().contiguous()
    loss, dz = loss_and_dz(engine, logits, target, config.loss_scale)
    return loss, dz, target


def logit_gradient(engine, dz: torch.Tensor, logits: torch.Tensor):
    """``dz`` back through the bilinear resize to the head's logits -> (d16, d_lo | None, bias partials, inv) with ``inv`` the factor
    every gradient kernel of the backward applies."""
    _, hh, ww, _ = logits.shape
    r = ops.resize_bilinear_bwd(dz, hh, ww, config.operand_dtype, config.split_conv)
    d16, d_lo, bpart = r if config.split_conv else (r[0], None, r[1])
    inv = 1.0 / (config.loss_scale * world_size(engine.process_group))  # gradient mean over ranks folded into the un-scaling (DDP semantics)
    return d16, d_lo, bpart, inv


def _hi_lo(t: torch.Tensor, B: int, h: int, w: int, D: int):
    """fp32 token map [B * h * w, D] -> the 16-bit NHWC operand of a head, (hi, lo | None) [B, h, w, D]"""
    dt = config.operand_dtype
    hi = ops.cast_pad(t, D, dt).view(B, h, w, D)
    lo = ops.cast_pad(t, D, dt, part=1).view(B, h, w, D) if config.split_conv else None
    return hi, lo


def make_decoder_bucket(seg_decoder):
    """The head's parameters in the gradient-ready order of its backward (final conv first, decoder_1 last) -> (flat bucket,
    the bucket range of every stage of ``seg_decoder.GRAD_ORDER``: what a ``StageReducer`` exchanges per ``stage_done``)."""
    order = list(seg_decoder.GRAD_ORDER)
    named = dict(seg_decoder.named_parameters())
    ordered = [(n, named[n]) for pre in order for n in named if n.startswith(pre + ".")]
    assert len(ordered) == len(named)
    bucket = FlatBucket(ordered)
    return bucket, [bucket.range_of([n for n in named if n.startswith(pre + ".")]) for pre in order]


def make_ema(optimizer, ema_decay: Optional[float], ema_warmup: bool) -> Optional[EMA]:
    """The engines' ``ema_decay=`` switch: None builds nothing (no shadow buffer, no launch), a value in (0, 1) an ``optim.EMA``
    over every bucket ``optimizer`` steps, following its on-device skip decision."""
    if ema_decay is None:
        return None
    return EMA(optimizer.buckets, ema_decay, warmup=ema_warmup, guard=optimizer.guard)


def _optimizer_step(engine) -> None:
    """the end of every ``train_step``: the optimizer's step and, when the engine averages, the average's update behind it"""
    engine.optimizer.step(1.0)
    if engine.ema is not None:
        engine.ema.update()


def _check_trainable(engine) -> None:
    if engine.ema is not None and engine.ema.swapped_in:
        raise RuntimeError("train_step inside ema_weights(): the parameters point at the averaged weights, which are not trained")


@contextlib.contextmanager
def ema_weights(engine):
    """Inside the context every parameter the optimizer steps IS its exponential moving average: ``p.data`` points at the
    parameter's view of the shadow buffer and comes back to its view of ``bucket.flat`` on exit, also when the body raises.
    The live weights are never written.  The address of every parameter changes on entry and on exit, so every 16-bit pack, the
    merged LoRA weights included, rebuilds both times (``packs.tag_of`` keys on ``data_ptr``).  Buffers are not averaged: BatchNorm
    running statistics inside the context are the live ones.  ``train_step`` inside the context raises."""
    if engine.ema is None:
        raise ValueError("ema_weights(): the engine keeps no average (ema_decay=None)")
    engine.ema.swap_in()
    try:
        yield engine
    finally:
        engine.ema.swap_out()


class SegEngine(nn.Module):
    """One object owning the frozen ViT, the CNN encoder, the adapters, the decode head and the optimizer.

    mode="reference_exact" reproduces `train.py` as written: adapters/encoder run forward only (graph
    cut at `train.py:389-406`), ``level_embed`` is a fresh zero tensor (no-op), the loss applies
    softmax twice, only the decoder is optimised (momentum 0.99, wd 3e-5: `train.py:178-191`).
    """

    # loss name -> (n_region, region mode, eps / smooth, n_ce) of asis_seg_loss_fwd, all on softmax(resize(logits))
    # as the scripts apply `nn.Softmax(1)` before the loss (`train.py:424`) — except "ce_dc", which the decoder-only
    # scripts apply to the raw resized logits (`eval/eval_dinov2_unet.py:291-297`)
    LOSSES = {
        "dice": (2, ops.LOSS_DICE, 10e-20, 0),          # train.py:427-428  DC(2)(softmax(out))
        "iou": (2, ops.LOSS_IOU, 1e-6, 0),              # train_multi_class.py:390-393
        "softdice": (1, ops.LOSS_SOFTDICE, 1.0, 0),     # train.py:425 (commented alternative)
        "dc_and_ce": (1, ops.LOSS_SOFTDICE, 1.0, 2),    # train.py:426 (commented alternative)
        "tversky": (1, ops.LOSS_TVERSKY, 1.0, 0),       # train.py:50 import
        "ce_dc": (1, ops.LOSS_DICE, 10e-20, 1),         # eval/eval_dinov2_unet.py:291-297, eval_dinov2_setr_cross_ete.py:334-340
        # segloss/lovasz_loss.py: LovaszSoftmax()(softmax(out)) through asis_lovasz_softmax (eps unused), and CrossentropyND on
        # the resized logits plus that term (the analogue of "ce_dc"); see loss_and_dz
        "lovasz": (1, ops.LOSS_LOVASZ, 0.0, 0),
        "ce_lovasz": (1, ops.LOSS_LOVASZ, 0.0, 1),
        # hard-pixel losses through asis_hardpixel_loss (see loss_and_dz).  "topk": segloss/ND_Crossentropy.py TopKLoss(k=topk_percent)
        # on the raw resized logits (the convention of "ce_dc" / "ce_lovasz"); "dc_and_topk": segloss/dice_loss.py
        # DC_and_topk_loss({}, {"k": topk_percent}) = SoftDice (n_region 1, smooth 1) through asis_seg_loss_fwd + that;
        # "focal": segloss/focal_loss.py FocalLoss(gamma=focal_gamma)(softmax(out)) (n_region = its n_softmax)
        "topk": (0, ops.LOSS_TOPK, 0.0, 0),
        "dc_and_topk": (1, ops.LOSS_TOPK, 1.0, 0),
        "focal": (1, ops.LOSS_FOCAL, 0.0, 0),
    }
    # the losses of asis_seg_loss_fwd: the ones that have an ignore label (asis_semi_loss), so the ones a batch with unlabelled
    # frames can train with
    IGNORE_LOSSES = ("dice", "iou", "softdice", "dc_and_ce", "tversky", "ce_dc")

    def __init__(self, model, backbone_encoder, cross_vit: CAViT, cross_cnn: CACNN, seg_decoder, *,
                 n_last_blocks: int = 4, num_classes: int = 2, lr: float = 0.01, momentum: float = 0.99,
                 weight_decay: float = 3e-5, mode: str = "reference_exact", process_group=None, loss: str = "dice",
                 train_encoder: bool = False, train_backbone: bool = False, optimize_backbone: bool = False,
                 blocks_per_bucket: int = 4, grad_compress: Optional[str] = None, optimizer: str = "sgd",
                 betas=(0.9, 0.999), eps: float = 1e-8, clip_grad: Optional[float] = None, no_decay: bool = True,
                 layer_decay: Optional[float] = None, topk_percent: float = 10.0, focal_gamma: float = 2.0,
                 drop_path_seed: int = 0, lora_rank: Optional[int] = None, lora_alpha: Optional[float] = None,
                 ema_decay: Optional[float] = None, ema_warmup: bool = True, teacher=None, distill_weight: float = 1.0,
                 distill_temperature: float = 1.0, distill_threshold: Optional[float] = None, distill_rampup: int = 0,
                 distill_flip: bool = False, mix: Optional[str] = None, mix_p: float = 1.0, mix_seed: int = 0,
                 mix_background: bool = False, ignore_index: Optional[int] = None, distill_labelled_weight: float = 1.0,
                 distill_class_thresholds=None, distill_adaptive_momentum: float = 0.999):
        """``seg_decoder``: ``FeatureDecoder`` -> the `train.py` flow; ``DecoderMLA`` -> the `train_mla.py` flow
        (block -> CACNN -> CAViT order, the four adapter-stream maps feed the MLA head, `blocks[-2]` is evaluated
        twice and `blocks[-1]` never: `train_mla.py:318,340`).  ``loss``: a key of ``SegEngine.LOSSES``.

        ``train_backbone`` (with mode="train_adapters"; BASELINE config 4): the `train.py` adapter flow with its
        no_grad / inference_mode regions removed (`train.py:287,300-302,389-406`), i.e. the unfreezing pattern of
        `eval/eval_dinov2_setr_cross_ete.py:145-148,307-361` applied to this flow: BOTH ViT passes run with saved
        activations, the backward goes through the head, the four adapter stages, the encoder (``train_encoder``) and
        every block evaluation of both passes with weight gradients; the 304 M backbone gradients live in a flat
        gradient bucket all-reduced in ``blocks_per_bucket``-block chunks while earlier blocks are still in their
        backward.  Like the reference script (its optimizer lists the decoder only, `:224-229`) the backbone gradients are
        computed and exchanged but not applied unless ``optimize_backbone`` is set.  ``grad_compress`` ("bf16" | "none"; default: the ``ASIS_GRAD_COMPRESS``
        environment variable, else "bf16"): the backbone bucket travels as bfloat16 (parallel.StageReducer) — half the bytes of the
        one exchange that is large enough for an xGMI ring to notice (0.6 instead of 1.2 GB); the decoder / adapter / encoder buckets
        (63 + 31 MB) always travel as fp32 like the reference's DDP.

        ``optimizer``: "sgd" (default: ``optim.SGD`` with ``momentum`` / ``weight_decay``, the reference scripts) or "adamw"
        (``optim.AdamW`` with ``betas``, ``eps``, ``weight_decay``, global-norm clipping at ``clip_grad``, ``no_decay`` for 1-D and
        token parameters; ``layer_decay`` scales the learning rate of the ViT bucket per block, so it needs
        ``optimize_backbone``).  ``clip_grad`` with "sgd" raises: the SGD kernels do not clip.

        ``topk_percent``: the ``k`` of ``TopKLoss`` for the losses "topk" / "dc_and_topk" (the worst k % of the batch's pixels);
        ``focal_gamma``: the ``gamma`` of ``FocalLoss`` for "focal".

        ``drop_path_seed``: seed of the stochastic-depth draws of a model built with ``drop_path_rate`` > 0 (droppath.py); they
        act in the training forward of ``train_backbone`` only, and every rank draws its own.

        ``lora_rank`` (4 | 8 | 16 | 32, with mode="train_adapters" and ``train_backbone``; ``lora_alpha`` defaults to the rank):
        low-rank adaptation of the q and v projections of every block (lora.py).  The step is the ``train_backbone`` step with the
        backbone weights frozen: both ViT passes run the training forward on the K-augmented qkv GEMM, the backward produces
        input gradients plus the three LoRA gradients per block, no backbone gradient bucket exists, a small LoRA bucket is
        all-reduced once (after block 0's backward) and joins the optimizer; ``eval_logits`` (validation, prediction) runs the
        frozen forward on the merged weights.  Not with ``optimize_backbone``, ``layer_decay``, stochastic depth or the MLA flow.

        ``ema_decay`` (in (0, 1); default None: nothing is allocated or launched): ``self.ema`` = ``optim.EMA`` over every bucket the
        optimizer steps (decoder, adapters, encoder, the backbone under ``optimize_backbone``, LoRA), updated on the device right
        after every optimizer step and skipped with it; ``ema_warmup``: update t uses the decay ``min(ema_decay, (1 + t) / (10 + t))``.
        ``ema_weights()`` evaluates and predicts with the average.  BatchNorm running statistics are buffers and are not averaged:
        an evaluation under ``ema_weights()`` uses the live ones.

        ``teacher`` (default None: nothing is allocated, launched or loaded, the step is the one without the keyword): mean-teacher
        training.  "ema" (needs ``ema_decay``): the teacher is this engine under ``ema_weights()``; a ``SegEngine``: a frozen
        teacher, which is never stepped.  Every ``train_step`` first takes the teacher's logits of ``teacher_inp`` (and, with
        ``distill_flip``, of its mirror image) under the guard of ``predict``, then adds ``ops.consistency_loss`` against them
        (``distill_temperature``, ``distill_threshold``) to the hard loss: total = hard + lambda_t kd with lambda_t =
        ``distill_weight`` * ``optim.consistency_ramp(distill_step, distill_rampup)``, ``distill_step`` the number of steps so
        far (a host counter).

        ``mix`` (default None: nothing is drawn, allocated, launched or loaded, the step is the one without the keyword): "cutmix"
        or "classmix" — every ``train_step`` draws the tables of ``tools.mix.MixSampler(mix, mix_p, mix_seed, num_classes,
        mix_background)`` for step ``mix_step`` (a host counter) and rank ``mix_rank`` (an attribute, default 0), and, where the
        draw mixes a sample, the student's forward and the hard loss see ``ops.mix_batch`` of the batch.  A teacher still sees the
        unmixed batch; the consistency term reads its maps through the same mixing (``ops.consistency_loss(mix=)``).  A step
        whose draw mixes no sample is the unmixed step.  ``last_mix_pasted``: int32 [B] on the device, the pasted pixels per
        sample of the last step (None where nothing was mixed).

        ``ignore_index`` (an int outside 0..num_classes-1; default None: the step launches what it launches without the keyword and
        libasis_semi.so is never opened): pixels with that label take no part in the hard loss (``ops.seg_loss_ignore``; a loss
        of ``IGNORE_LOSSES``), ``last_hard_valid`` holds the valid pixels per sample of the last step.  ``train_step(labelled=)``
        marks whole samples as unlabelled (it needs a ``teacher``): their target rows are filled with the ignore value (255
        where ``ignore_index`` is None) on the device, the hard loss leaves them out, and the consistency term weighs them 1 and
        the labelled samples ``distill_labelled_weight`` (0: a labelled sample reads none of its teacher maps).  With ``mix`` the
        donors are drawn inside the two groups, and ClassMix takes the classes of an unlabelled donor from the teacher's
        prediction (``ops.predict_mask_views`` of its maps).

        ``distill_class_thresholds`` (default None: nothing is allocated, opened or launched; it needs a ``teacher`` and excludes
        ``distill_threshold``): a confidence threshold per class for the consistency term (``ops.consistency_loss(class_threshold=)``,
        csrc/adapt.hip).  A list of ``num_classes`` finite values: fixed thresholds.  "adaptive": self-adaptive thresholding
        (``adaptive_threshold.AdaptiveThreshold`` with ``distill_adaptive_momentum``, as ``self.adaptive``): between the teacher's
        prediction and the student's forward every ``train_step`` takes the statistics of the teacher's unmixed maps over the
        samples the consistency term weighs above 0, sums them over the ranks and updates the thresholds, so the batch takes part
        in its own thresholds (``taps``: ``kd_class_thr``, ``kd_conf_sums``)."""
        super().__init__()
        if grad_compress is None:   # default since round 5: bf16 transport for the 1.2 GB backbone bucket (ASIS_GRAD_COMPRESS=none: fp32)
            grad_compress = os.environ.get("ASIS_GRAD_COMPRESS", "bf16").lower()
        if grad_compress in ("", "0", "none", "off", "fp32"):
            grad_compress = None
        if mode not in ("reference_exact", "train_adapters"):
            raise ValueError("mode must be 'reference_exact' or 'train_adapters'")
        if loss not in self.LOSSES:
            raise ValueError(f"loss must be one of {sorted(self.LOSSES)}")
        self.loss_kind = loss
        if ignore_index is not None:
            if isinstance(ignore_index, bool) or not isinstance(ignore_index, int) or 0 <= ignore_index < num_classes:
                raise ValueError(f"ignore_index={ignore_index!r} must be an int outside the classes 0..{num_classes - 1}")
            if loss not in self.IGNORE_LOSSES:
                raise ValueError(f"loss {loss!r} has no ignore label: ignore_index needs one of {self.IGNORE_LOSSES}")
        if not float(distill_labelled_weight) >= 0.0 or float(distill_labelled_weight) == float("inf"):
            raise ValueError("distill_labelled_weight must be finite and >= 0")
        self.ignore_index, self.distill_labelled_weight = ignore_index, float(distill_labelled_weight)
        self._hard_ignore, self.last_hard_valid, self._semi_cache = ignore_index, None, {}
        if not 0.0 < topk_percent <= 100.0:
            raise ValueError("topk_percent must be in (0, 100]")
        if focal_gamma < 0.0:
            raise ValueError("focal_gamma must be >= 0")
        self.topk_percent, self.focal_gamma = float(topk_percent), float(focal_gamma)
        self.is_mla = type(seg_decoder).__name__ == "DecoderMLA"
        # UNet head (BASELINE config 2): fed with the adapter-stream map alone, (B, h, w, D)
        self.stream_only = type(seg_decoder).__name__ == "UNet"
        self.model, self.backbone_encoder = model, backbone_encoder
        self.cross_vit, self.cross_cnn, self.seg_decoder = cross_vit, cross_cnn, seg_decoder
        self.n_last_blocks, self.num_classes, self.mode = n_last_blocks, num_classes, mode
        self.patch = model.patch_size
        self.heads = model.num_heads
        self.process_group = process_group
        if train_encoder and mode != "train_adapters":
            raise ValueError("train_encoder needs mode='train_adapters'")
        self.train_encoder = train_encoder
        frozen = list(model.parameters()) + ([] if train_encoder else list(backbone_encoder.parameters()))
        if mode == "reference_exact":
            frozen += list(cross_vit.parameters()) + list(cross_cnn.parameters())
        for p in frozen:
            p.requires_grad_(False)  # no gradient reaches them in the reference step
        self.bucket, self.stage_ranges = make_decoder_bucket(seg_decoder)
        buckets = [self.bucket]
        self.adapter_bucket = None
        if mode == "train_adapters":
            # the trainable set the reference's optimiser lists for the adapters (`train.py:178-186`) and that its
            # no_grad block (`:389-406`) and forward-only MSDeformAttnFunction keep from ever training (SURVEY facts
            # 1-2): CAViT + CACNN parameters, one flat bucket, all-reduced once the adapter backward is enqueued
            if type(seg_decoder).__name__ not in ("FeatureDecoder", "DecoderSETR", "UNet", "DecoderMLA"):
                raise NotImplementedError("train_adapters is built for the train.py adapter flow (FeatureDecoder / UNet heads) and "
                                          "the train_mla.py flow (DecoderMLA)")
            if self.is_mla and train_backbone:
                raise NotImplementedError("the train_mla.py flow trains decoder + adapters (+ encoder); the unfrozen backbone "
                                          "(BASELINE config 4) is the train.py adapter flow")
            for p in list(cross_vit.parameters()) + list(cross_cnn.parameters()):
                p.requires_grad_(True)
            named_a = [("cross_vit." + n, p) for n, p in cross_vit.named_parameters()] + \
                      [("cross_cnn." + n, p) for n, p in cross_cnn.named_parameters()]
            self.adapter_bucket = FlatBucket(named_a)
            self.adapter_reducer = StageReducer(self.adapter_bucket.grad, [(0, self.adapter_bucket.numel)], process_group)
            buckets.append(self.adapter_bucket)
            self.encoder_bucket = None
            if train_encoder:  # the last member of the reference's optimiser list (`train.py:183`): the spatial-prior CNN
                for p in backbone_encoder.parameters():
                    p.requires_grad_(True)
                self.encoder_bucket = FlatBucket([("backbone_encoder." + n, p) for n, p in backbone_encoder.named_parameters()])
                self.encoder_reducer = StageReducer(self.encoder_bucket.grad, [(0, self.encoder_bucket.numel)], process_group)
                buckets.append(self.encoder_bucket)
        self.train_backbone = bool(train_backbone)
        # precision policy of the attention output (config.split_attn_out): hi + lo halves into the projection GEMM for the
        # heads that amplify a stream error most (UNet 3.9x, MLA 3.2x; FeatureDecoder 2x) and for the unfrozen backbone
        self.split_attn_out = config.split_attn_out_policy if config.split_attn_out_policy is not None else \
            bool(self.stream_only or self.is_mla or train_backbone)
        # precision level of the ViT blocks (config.precise_level): level 2 (every linear layer on hi + lo operands) for the one
        # geometry whose full-depth stress golden needs it — the MLA head (amplifies a stream error 3.2x) behind 2 x 40 block
        # evaluations (BASELINE config 5: 1.30e-3 on single 16-bit operands, 3.0e-4 on level 2; tests/test_gpu_fulldepth.py)
        self.precise_level = config.precise_level_policy if config.precise_level_policy is not None else \
            (2 if (self.is_mla and len(model.blocks) >= 40) else 0)
        # ... and WHICH linear layers of a block run split there (config.precise_parts): the automatic level 2 of config 5 needs
        # the attention output (proj) and the LayerNorm output in front of w12 only — 8.3e-4 on the full-depth stress golden at
        # 58.9 img/s against 3.1e-4 at 48.2 with all four layers split (A/B table in config.py); a level forced by
        # ASIS_PRECISE_LEVEL keeps all four unless ASIS_PRECISE_PARTS names a subset
        all_parts = frozenset(("qkv", "proj", "fc1", "fc2"))
        self.precise_parts = config.precise_parts_policy if config.precise_parts_policy is not None else \
            (frozenset(("proj", "fc1")) if (config.precise_level_policy is None and self.precise_level == 2) else all_parts)
        self.vit_bucket = None
        self.lora = self.lora_bucket = None
        if lora_rank is None and lora_alpha is not None:
            raise ValueError("lora_alpha needs lora_rank")
        if lora_rank is not None:
            lora_mod.check_engine_args(mode=mode, train_backbone=train_backbone, optimize_backbone=optimize_backbone,
                                       layer_decay=layer_decay, is_mla=self.is_mla, model=model, rank=lora_rank)
            # the backbone weights stay frozen (requires_grad False, above): no ViT bucket; the LoRA parameters live in a small
            # bucket of their own whose one exchange fires when block 0 (the last of the reverse walk) has written its gradients
            self.lora = lora_mod.LoRA(model, lora_rank, lora_alpha)
            self.lora_bucket = FlatBucket(list(self.lora.named_parameters()))
            self.vit_reducer = StageReducer(self.lora_bucket.grad, [(0, self.lora_bucket.numel)], process_group)
            self._fire_at = [0]
            buckets.append(self.lora_bucket)
        elif train_backbone:
            if mode != "train_adapters":
                raise ValueError("train_backbone needs mode='train_adapters' (the unfrozen variant of the adapter flow)")
            self.vit_bucket, self.vit_reducer, self._fire_at = make_vit_bucket(model, blocks_per_bucket, process_group,
                                                                               momentum=optimize_backbone,
                                                                               min_first_blocks=n_last_blocks,
                                                                               compress=grad_compress)
            if optimize_backbone:
                buckets.append(self.vit_bucket)
        if layer_decay is not None and not (train_backbone and optimize_backbone):
            raise ValueError("layer_decay scales the learning rates of the ViT blocks: it needs train_backbone and optimize_backbone")
        self.drop_path = make_drop_path_sampler(model, drop_path_seed, process_group)
        if self.drop_path is not None and not train_backbone:
            raise ValueError("drop_path_rate drops samples in the training forward of the ViT blocks: it needs train_backbone")
        self.optimizer = make_optimizer(optimizer, buckets, lr=lr, momentum=momentum, weight_decay=weight_decay, betas=betas, eps=eps,
                                        clip_grad=clip_grad, no_decay=no_decay, depth=len(model.blocks),
                                        layer_decay=[layer_decay if b is self.vit_bucket else None for b in buckets])
        self.ema = make_ema(self.optimizer, ema_decay, ema_warmup)
        self.reducer = StageReducer(self.bucket.grad, self.stage_ranges, process_group)
        self._geom = {}
        if teacher is not None and teacher != "ema" and not isinstance(teacher, SegEngine):
            raise ValueError("teacher must be None, 'ema' or a SegEngine")
        if isinstance(teacher, str) and self.ema is None:
            raise ValueError("teacher='ema' needs ema_decay: the teacher is the average of the weights")
        if isinstance(teacher, SegEngine) and teacher.num_classes != num_classes:
            raise ValueError(f"the teacher predicts {teacher.num_classes} classes, the student {num_classes}")
        if teacher is not None:
            if not float(distill_weight) >= 0.0:
                raise ValueError("distill_weight must be >= 0")
            if not float(distill_temperature) > 0.0:
                raise ValueError("distill_temperature must be > 0")
            if distill_threshold is not None and not float(distill_threshold) <= 1.0:
                raise ValueError("distill_threshold must be at most 1 (None or <= 0 keeps every pixel)")
            if int(distill_rampup) < 0:
                raise ValueError("distill_rampup counts steps: it must be >= 0")
        # not a submodule: a teacher engine's parameters are not this engine's (state_dict, .to(), the optimizer's buckets)
        object.__setattr__(self, "teacher", teacher)
        self.distill_weight, self.distill_temperature = float(distill_weight), float(distill_temperature)
        self.distill_threshold = None if distill_threshold is None else float(distill_threshold)
        self.distill_rampup, self.distill_flip = int(distill_rampup), bool(distill_flip)
        self.distill_step = 0
        self.last_loss_kd = self.last_kd_kept = None
        self.adaptive = self.class_thresholds = None
        if distill_class_thresholds is not None:
            if teacher is None:
                raise ValueError("distill_class_thresholds gates the consistency term: it needs a teacher")
            if distill_threshold is not None:
                raise ValueError("distill_class_thresholds and distill_threshold exclude each other")
            dev = self.bucket.grad.device
            if isinstance(distill_class_thresholds, str):
                if distill_class_thresholds != "adaptive":
                    raise ValueError("distill_class_thresholds must be None, 'adaptive' or a list of num_classes thresholds")
                from ..adaptive_threshold import AdaptiveThreshold
                self.adaptive = AdaptiveThreshold(num_classes, distill_adaptive_momentum, dev, process_group)
                self.class_thresholds = self.adaptive.thresholds
            else:
                vals = [float(v) for v in distill_class_thresholds]
                if len(vals) != num_classes or not all(math.isfinite(v) for v in vals):
                    raise ValueError(f"distill_class_thresholds must hold {num_classes} finite values, one per class")
                if not 1 <= num_classes <= ops.ADAPT_MAX_CLASSES:
                    raise ValueError(f"distill_class_thresholds: num_classes={num_classes} must be in 1..{ops.ADAPT_MAX_CLASSES}")
                self.class_thresholds = torch.tensor(vals, dtype=torch.float32).to(dev)
        self.mix_sampler = None
        if mix is not None:
            from ..tools.mix import MixSampler
            self.mix_sampler = MixSampler(mix, mix_p, mix_seed, num_classes, mix_background)
        self.mix_step, self.mix_rank = 0, 0
        self.last_mix_pasted = None

    ema_weights = ema_weights

    @torch.no_grad()
    def _teacher_maps(self, inp: torch.Tensor):
        """The teacher's logit maps of ``inp`` (and of its mirror image with ``distill_flip``) under the guard of ``predict``
        -> (maps, flips).  With ``teacher="ema"`` every averaged parameter is re-packed on the way in and on the way out
        (``packs.tag_of`` keys on ``data_ptr``)."""
        views, flips = [inp], [False]
        if self.distill_flip:
            views.append(inp.flip(-1))
            flips.append(True)
        if isinstance(self.teacher, SegEngine):
            return self.teacher._guarded_logits(views), flips
        with self.ema_weights():
            return self._guarded_logits(views), flips

    def _semi_tables(self, lab, dev):
        """the device tables of a ``labelled`` pattern, cached per pattern and uploaded without blocking: the unlabelled samples
        (int64 indices) and the consistency term's fp32 [B] weights (1 unlabelled, ``distill_labelled_weight`` labelled)"""
        key = (lab, self.distill_labelled_weight, str(dev))
        if key not in self._semi_cache:
            pin = torch.device(dev).type == "cuda"
            idx = torch.tensor([b for b, l in enumerate(lab) if not l], dtype=torch.int64)
            sw = torch.tensor([self.distill_labelled_weight if l else 1.0 for l in lab], dtype=torch.float32)
            if pin:
                idx, sw = idx.pin_memory(), sw.pin_memory()
            self._semi_cache[key] = (idx.to(dev, non_blocking=True), sw.to(dev, non_blocking=True), idx, sw)   # the staging tensors stay alive
        return self._semi_cache[key][:2]

    def _mix(self, inp: torch.Tensor, target: torch.Tensor, taps: Optional[dict], lab=None, unl=None, g=None, tmaps=None, tflips=None):
        """The draw of step ``mix_step`` and, where it mixes a sample, ``ops.mix_batch`` -> (inp, target, (sel, donor) or None).
        Counts the step.  With unlabelled samples (``unl``: their indices on the device; ``lab`` the host pattern): donors are drawn
        inside the labelled and inside the unlabelled group; ClassMix reads the classes of an unlabelled donor from the teacher's
        prediction, CutMix reads none; the unlabelled rows of the mixed target are filled with ``g`` by the caller."""
        tables = self.mix_sampler.draw(inp.shape[0], inp.shape[-2], inp.shape[-1], self.mix_step, self.mix_rank,
                                       groups=None if lab is None else [int(l) for l in lab])
        self.mix_step += 1
        self.last_mix_pasted = None
        if not bool(tables["kind"].any()):
            return inp, target, None
        target = target.long().contiguous()
        if unl is not None:   # the unlabelled rows the mixing reads: the teacher's classes (ClassMix), or the ignore value
            if bool((tables["kind"] == 2).any()):
                pseudo = ops.predict_mask_views(tmaps, tuple(target.shape[-2:]), flips=tflips)
                target = target.index_copy(0, unl, pseudo.index_select(0, unl).long())
                if taps is not None:
                    taps.update(pseudo_target=pseudo)
            else:
                target = target.index_fill(0, unl, g)
        inp, target, sel, pasted = ops.mix_batch(inp.contiguous(), target, tables, self.num_classes,
                                                 self.mix_sampler.background)
        self.last_mix_pasted = pasted
        if taps is not None:
            taps.update(mix_inp=inp, mix_target=target, mix_sel=sel, mix_tables=tables, mix_pasted=pasted)
        return inp, target, (sel, tables["donor"])

    def _add_consistency(self, logits, target, dz, hard, maps, flips, S: float, taps: Optional[dict], mix=None,
                         sample_weight=None) -> torch.Tensor:
        """The soft term of a step with a teacher: ``ops.consistency_loss`` against ``maps`` (read through ``mix`` where the
        batch was mixed) added into the hard term's ``dz`` at S lambda_t -> hard + lambda_t kd (a device tensor, no host sync).
        Counts the step."""
        lam = self.distill_weight * consistency_ramp(self.distill_step, self.distill_rampup)
        self.distill_step += 1
        scratch = _loss_scratch(self, "_consist_scratch", ops.consistency_scratch_bytes(target.numel()), logits.device)
        kd, kept, _ = ops.consistency_loss(logits, maps, target, flips=flips, temperature=self.distill_temperature,
                                           threshold=self.distill_threshold, sample_weight=sample_weight, grad_scale=S * lam, dz=dz,
                                           scratch=scratch, mix=mix,
                                           **({} if self.class_thresholds is None else {"class_threshold": self.class_thresholds}))
        self.last_loss_kd, self.last_kd_kept = kd, kept
        total = hard + lam * kd
        if taps is not None:
            taps.update(loss_hard=hard, loss_kd=kd, kd_kept=kept, teacher_logits=maps, distill_scale=lam)
            if self.class_thresholds is not None:
                taps.update(kd_class_thr=self.class_thresholds.clone(),
                            kd_conf_sums=None if self.adaptive is None else self.adaptive.sums.clone())
        return total

    def _ema_modules(self) -> Dict[str, nn.Module]:
        """checkpoint key -> module, for the modules this engine trains (the keys ``train_seg`` saves them under)"""
        mods = {"state_dict": self.seg_decoder}
        if self.mode == "train_adapters":
            mods.update(cross_vit=self.cross_vit, cross_cnn=self.cross_cnn)
            if self.train_encoder:
                mods["backbone_encoder"] = self.backbone_encoder
            if self.vit_bucket is not None and any(b is self.vit_bucket for b in self.optimizer.buckets):
                mods["backbone"] = self.model
        return mods

    def ema_state_dict(self) -> dict:
        """The ``ema`` entry of a checkpoint, shaped like the checkpoint itself: ``decay``, ``warmup``, ``updates`` (a host read)
        and, under the keys and ``module.`` prefixes of the live entries, the state of every module this engine trains —
        parameters from the average, buffers (BatchNorm running statistics) from the live module — plus ``lora`` with LoRA."""
        if self.ema is None:
            raise ValueError("ema_state_dict(): the engine keeps no average (ema_decay=None)")
        out = {"decay": self.ema.decay, "warmup": self.ema.warmup, "updates": self.ema.updates}
        with self.ema_weights():
            for key, mod in self._ema_modules().items():
                out[key] = {"module." + n: v.detach().clone() for n, v in mod.state_dict().items()}
            if self.lora is not None:
                out["lora"] = self.lora.state_dict()
        return out

    def load_ema_state_dict(self, entry: dict) -> str:
        """Restore the average and its update count from an ``ema_state_dict()`` entry.  Everything is checked before anything is
        written; buffers in the entry are ignored (they are the live module's, restored with it)."""
        if self.ema is None:
            raise ValueError("load_ema_state_dict(): the engine keeps no average (ema_decay=None)")
        upd = entry.get("updates") if isinstance(entry, dict) else None
        if isinstance(upd, bool) or not isinstance(upd, int) or upd < 0:
            raise ValueError("ema entry: no update count (not written by SegEngine.ema_state_dict)")
        shadow = {id(p): view for _, p, view in self.ema.named_shadows()}
        named = [(key, "module." + n, p) for key, mod in self._ema_modules().items() for n, p in mod.named_parameters()]
        sources = {key: entry.get(key) for key in self._ema_modules()}
        if self.lora is not None:
            named += [("lora", n, p) for n, p in self.lora.named_parameters()]
            sources["lora"] = entry["lora"].get("params") if isinstance(entry.get("lora"), dict) else None
        todo = []
        for key, n, p in named:
            if id(p) not in shadow:
                continue
            src = sources[key].get(n) if isinstance(sources[key], dict) else None
            if not torch.is_tensor(src) or tuple(src.shape) != tuple(p.shape):
                raise ValueError(f"ema entry: '{key}' does not hold '{n}' with shape {list(p.shape)}: not written with the same "
                                 "trainable set")
            todo.append((shadow[id(p)], src))
        if len(todo) != len(shadow):
            raise ValueError("ema entry: the modules of this engine do not cover every averaged parameter")
        for dst, src in todo:
            dst.copy_(src.to(dst.device, torch.float32))
        self.ema.state[0] = upd
        if float(entry.get("decay", self.ema.decay)) != self.ema.decay or bool(entry.get("warmup", self.ema.warmup)) != self.ema.warmup:
            print(f"ema entry was written with decay {entry.get('decay')} / warmup {entry.get('warmup')}; continuing with "
                  f"{self.ema.decay} / {self.ema.warmup}")
        return "<All EMA keys matched successfully>"

    # ------------------------------------------------------------------------------------------
    def _geometry(self, H, W, shapes, dev):
        key = (H, W, tuple(shapes), dev)
        g = self._geom.get(key)
        if g is None:
            d1, d2 = deform_inputs(torch.zeros(1, 3, H, W), self.patch, shapes)
            g = {"ref1": d1[0][0, :, 0, :].contiguous().to(dev), "shapes1": d1[1].to(torch.int32).to(dev),
                 "starts1": d1[2].to(torch.int32).to(dev), "ref2": d2[0][0, :, 0, :].contiguous().to(dev),
                 "shapes2": d2[1].to(torch.int32).to(dev), "starts2": d2[2].to(torch.int32).to(dev)}
            self._geom = {key: g}
        return g

    def _encoder_on_side_stream(self, inp: torch.Tensor):
        """The spatial-prior CNN (≈ 30 small, latency-bound launches + 6 SyncBatchNorm all-reduces of 2C doubles) is
        independent of the ViT until the first adapter stage: run it on a side HIP stream so it fills the gaps of the
        GEMM-bound block loop and — on N > 1 ranks — its six blocking statistic exchanges wait for each other there, not
        on the compute stream.  -> (c tokens, level shapes, event recorded behind the last encoder kernel)."""
        main = torch.cuda.current_stream()
        if getattr(self, "_enc_stream", None) is None:
            self._enc_stream = torch.cuda.Stream()
        side = self._enc_stream
        side.wait_stream(main)          # the input batch, and everything of the previous step that read recycled blocks
        with torch.cuda.stream(side):
            _, c, shapes = self.backbone_encoder.forward_tokens(inp, need_c1=not config.elide_c1)
            done = torch.cuda.Event()
            done.record(side)
        c.record_stream(main)           # allocated on the side stream, consumed on the compute stream
        return c, shapes, done

    def _trunk_dual(self, xcat: torch.Tensor, Ra: int, blocks, segs) -> torch.Tensor:
        """The trunk blocks with the two token batches on two HIP streams (config.dual_stream; ASIS_TRUNK_STREAMS=4 cuts each
        batch in two image groups: four streams) -> the stacked [Ra + Rb, D]."""
        main = torch.cuda.current_stream()
        nper = 2 if config.trunk_streams >= 4 and min(b for b, _ in segs) >= 2 else 1
        if getattr(self, "_dual_streams", None) is None or len(self._dual_streams) != 2 * nper:
            self._dual_streams = tuple(torch.cuda.Stream() for _ in range(2 * nper))
        parts = []                                   # (row slice, [(B, N)]) per stream, in row order
        r0 = 0
        for (B, N) in segs:
            cuts = [0, B] if nper == 1 else [0, B // 2, B]
            for a, b in zip(cuts[:-1], cuts[1:]):
                parts.append((slice(r0 + a * N, r0 + b * N), [(b - a, N)]))
            r0 += B * N
        xs = []
        for st, (sl, _) in zip(self._dual_streams, parts):
            st.wait_stream(main)
            xcat.record_stream(st)
            xs.append(xcat[sl])
        # block by block, alternating between the streams (the launch order the streams' kernels interleave in); inside the run
        # the residual stream stays in the two-plane form where Block.fold_ok allows (blocks.run_blocks semantics)
        nblk = len(blocks)
        for bi, blk in enumerate(blocks):
            for i, (st, (_, sg)) in enumerate(zip(self._dual_streams, parts)):
                with torch.cuda.stream(st):
                    R_i = xs[i][0].shape[0] if isinstance(xs[i], tuple) else xs[i].shape[0]
                    if blk.fold_ok(R_i, sg):
                        xs[i] = blk.forward_rows_fold(xs[i], sg, planes_out=bi + 1 < nblk and blocks[bi + 1].fold_ok(R_i, sg))
                    else:
                        xs[i] = blk.forward_rows(xs[i], sg)
        for st, x in zip(self._dual_streams, xs):
            main.wait_stream(st)
            x.record_stream(main)
        return torch.cat(xs, 0)

    def _cavit(self, x2, c2, g, B, Lq, Lin, save: bool = False):
        """-> (CAViT output, its saved activations | None)"""
        cv = self.cross_vit
        if save:
            # CAViT keeps its query for the LayerNorm backward; the callers overwrite the rows ``x2`` views in place (the stage
            # output, the next block's input), so the saved copy must be its own tensor
            return cv.forward16_train(x2.clone(), c2, g, B, Lq, Lin)
        return cv.attn.forward16(cv._ln16("query_norm", x2), cv._ln16("feat_norm", c2), g["ref1"], g["shapes1"],
                                 g["starts1"], B, Lq, Lin, res=x2, scale_n=cv._f32("gamma", cv.gamma)), None

    def _cacnn(self, c2, x2, g, B, Lq, Lin, grids, save: bool = False):
        """-> (CACNN output, its saved activations | None)"""
        cn = self.cross_cnn
        if save:
            return cn.forward16_train(c2, x2, g, B, Lq, Lin, grids)
        out = cn.attn.forward16(cn._ln16("query_norm", c2), cn._ln16("feat_norm", x2), g["ref2"], g["shapes2"],
                                g["starts2"], B, Lq, Lin, res=c2)
        return (cn.ffn.forward16(cn._ln16("ffn_norm", out), out, B, Lq, grids) if cn.with_cffn else out), None

    # ---- the pieces the three forward walks (``features``, ``features_mla``, ``_features_e2e``) share -------------------------
    def _begin(self, inp: torch.Tensor):
        """This engine's precision policy into ``config`` -> (the batch as contiguous fp32, (B, H, W, D, h, w, N, number of blocks))."""
        config.split_attn_out = self.split_attn_out
        config.precise_level = self.precise_level
        config.precise_parts = self.precise_parts
        B, _, H, W = inp.shape
        h, w = H // self.patch, W // self.patch
        return inp.float().contiguous(), (B, H, W, self.model.embed_dim, h, w, h * w, len(self.model.blocks))

    def _encode(self, inp: torch.Tensor, train: bool, side_stream: bool = False):
        """The spatial-prior CNN and the sampling geometry of its level shapes -> (c tokens, shapes, geometry, event | None).
        ``train``: a training forward, which keeps the activations of an encoder that trains (``_esaved``, for
        ``_encoder_backward``); ``side_stream``: a frozen encoder may run beside the trunk (config.encoder_stream), and the
        caller waits for the returned event before it reads ``c``."""
        done = None
        if train and self.train_encoder:
            c, shapes, esaved = self.backbone_encoder.forward_tokens_train(inp)
            self._esaved = (esaved, shapes)
        elif side_stream and config.encoder_stream and inp.is_cuda:
            c, shapes, done = self._encoder_on_side_stream(inp)
        else:
            _, c, shapes = self.backbone_encoder.forward_tokens(inp, need_c1=not config.elide_c1)
        return c, shapes, self._geometry(inp.shape[-2], inp.shape[-1], shapes, inp.device), done

    def _adapter_stage(self, xb, c2d, feat, g, shapes, dead: bool, save: bool):
        """One adapter stage of the `train.py` flow behind its block: CAViT, CACNN unless ``dead``, and the residual add of pass
        A's feature ``feat`` [B, N, D] into pass B's rows ``xb`` [B * N, D] of the stacked buffer, in place: the next block reads
        the stage output there -> (stage output [B, N, D], c, (CAViT save, CACNN save | None) when ``save`` else None)."""
        B, N, D = feat.shape
        Lc = c2d.shape[0] // B
        x2, s_cv = self._cavit(xb, c2d, g, B, N, Lc, save)
        s_cn = None
        if not dead:
            c2d, s_cn = self._cacnn(c2d, x2, g, B, Lc, N, shapes, save)
        x = ops.add_f32(x2.view(B, N, D), feat, out=xb.view(B, N, D))
        return x, c2d, ((s_cv, s_cn) if save else None)

    def _decoder_cat(self, x, c_orig, feats, c2d, shapes, hw, taps: Optional[dict], mx: bool = False):
        """`train.py:389-406`: the last stage's output ``x`` [B, N, D] -> the head's input (hi, lo | None): the FeatureDecoder concat
        [x | c4 of the ENCODER output, zero-padded | last pass-A feature] as NHWC [B, h, w, 3D], or ``x`` alone for the UNet head."""
        B, N, D = x.shape
        Lc = c_orig.shape[1]
        if self.stream_only:
            cat = _hi_lo(x.reshape(B * N, D), B, *hw, D)
        else:
            n4 = shapes[2][0] * shapes[2][1]
            cat = ops.decoder_input(x, c_orig[:, Lc - n4:], feats[-1], hw, shapes[2], config.operand_dtype, config.split_conv, mx=mx)
            if not config.split_conv:
                cat = (cat, None)
        if taps is not None:
            taps.update(feats=feats, x_final=x, c_final=c2d.view(B, Lc, D), cat=cat[0])
        return cat

    def _slab_views(self, slabs: torch.Tensor, s: int) -> Dict[str, torch.Tensor]:
        """CAViT / CACNN are the same modules in every stage, so every stage writes its own gradient slab (the slabs are summed in
        a fixed order afterwards) -> name -> view of slab ``s``, shaped like the parameter"""
        ab = self.adapter_bucket
        return {n: slabs[s, o:o + p.numel()].view(p.shape) for n, p, o in zip(ab.names, ab.params, ab.offsets)}

    def _adapter_stage_backward(self, s_cv, s_cn, dx, dc_next, gs, inv: float):
        """Backward of ``_adapter_stage``.  ``dx`` [B, N, D]: gradient of the stage's stream output (the residual add is the
        identity, ``dx`` is not written); ``dc_next``: what the stage behind sent back for c, None for the last stage, whose CACNN
        fed nothing.  CACNN, which sends its share of the stream gradient too, then CAViT -> (gradient of the block output in
        front of the stage [B * N, D], gradient of the stage's c input [B * Lc, D])."""
        B, _, D = dx.shape
        dc_in = None
        if dc_next is not None:
            dc_in, dx_extra = self.cross_cnn.backward16(s_cn, dc_next, inv, gs, "cross_cnn")
            dx = ops.add_f32(dx, dx_extra.view_as(dx))
        dx_in, dc = self.cross_vit.backward16(s_cv, dx.view(-1, D), inv, gs, "cross_vit")
        if dc_in is not None:
            dc3 = dc.view(B, -1, D)
            ops.add_f32(dc3, dc_in.view_as(dc3), out=dc3)
        return dx_in, dc

    @torch.no_grad()
    def features(self, inp: torch.Tensor, taps: Optional[dict] = None, adapter_saves: Optional[list] = None):
        """`train.py:275-406`: image batch -> decoder input, NHWC 16-bit [B, h, w, 3D] as (hi, lo|None).
        ``adapter_saves`` (train_adapters mode): list that receives, per stage, the saved activations of the frozen
        block on pass B and of CAViT / CACNN."""
        inp, (B, H, W, D, h, w, N, nb) = self._begin(inp)
        m, nl = self.model, self.n_last_blocks
        train = self.mode == "train_adapters" and adapter_saves is not None
        c, shapes, g, enc_done = self._encode(inp, train, side_stream=True)
        Lc = c.shape[1]
        # ---- pass A (train.py:287): cls + pos-embed, all blocks, final norm on the last n outputs ----
        # ---- both passes stacked along the rows: every block evaluation of pass A (cls + pos-embed tokens, all
        # blocks, `train.py:287`) has a pass-B partner on the same frozen weights (raw patch tokens through
        # blocks[0:-3], `train.py:300-302`, then one more block per adapter stage), so each launch carries 2x the rows.
        # The patch embedding (shared by both passes: same conv on the same input) writes pass B's rows of the stacked
        # buffer directly, the cls / pos-embed form goes into pass A's rows: no concatenation copy.
        Ra, Rb = B * (N + 1), B * N
        segs = [(B, N + 1), (B, N)]
        xcat = torch.empty((Ra + Rb, D), device=inp.device, dtype=torch.float32)
        tokens, _ = m.patch_embed.tokens(inp, out=xcat[Ra:])
        if not config.share_patch_embed:   # the reference's second evaluation (pass A's own, `vision_transformer.py:190`): same values
            tokens, _ = m.patch_embed.tokens(inp)
        pos = m._pos_for(N, H, W)
        ops.add_cls_pos(tokens, m.cls_token.detach().reshape(-1).float().contiguous(),
                        pos.detach().reshape(-1, D).float().contiguous(), out=xcat[:Ra].view(B, N + 1, D))
        feats = []
        trunk = list(m.blocks[: nb - (nl - 1)])
        if config.dual_stream and inp.is_cuda and getattr(self, "_dual_warm", False) and nb - nl == len(trunk) - 1:
            xcat = self._trunk_dual(xcat, Ra, trunk, segs)
            feats.append(m._final_norm(xcat[:Ra].view(B, N + 1, D))[:, 1:])
            trunk = []
        self._dual_warm = True      # the first step runs in order: it fills the per-module operand caches on one stream
        if trunk:   # only the LAST trunk block's output is read as fp32 (final norm + adapter stage 0): one run
            assert nb - nl == len(trunk) - 1
            xcat = run_blocks(trunk, xcat, segs)
            feats.append(m._final_norm(xcat[:Ra].view(B, N + 1, D))[:, 1:])   # [B, N, D] view, batch stride (N+1)*D
        if enc_done is not None:
            torch.cuda.current_stream().wait_event(enc_done)   # the pyramid tokens are first needed by adapter stage 0
        if taps is not None:
            taps.update(c=c, x_b0=xcat[Ra:].view(B, N, D).clone(), shapes=shapes)
        c2d = c.view(B * Lc, D)
        for s in range(nl):
            bsaved = None
            if s > 0:
                blk = m.blocks[nb - (nl - 1) + s - 1]
                if train:  # pass B through the frozen block with saved activations (input gradient needed), pass A plain
                    xa_s = blk.forward_rows(xcat[:Ra], [(B, N + 1)])
                    xb_s, bsaved = blk.forward_train(xcat[Ra:].view(B, N, D))
                    xcat = torch.cat([xa_s, xb_s.reshape(Rb, D)], 0)
                else:
                    xcat = run_blocks([blk], xcat, segs)
                feats.append(m._final_norm(xcat[:Ra].view(B, N + 1, D))[:, 1:])
            # the last stage's CACNN output (`train.py:372-386`) feeds nothing: the decoder input takes c4 from the
            # ENCODER output (`:395`), so unless a caller asks for the taps it is dead code and skipped (same results)
            dead = s == nl - 1 and taps is None and config.elide_dead_cacnn
            x, c2d, saves = self._adapter_stage(xcat[Ra:], c2d, feats[s], g, shapes, dead, train)
            if train:
                adapter_saves.append((bsaved, *saves))
        d1 = getattr(self.seg_decoder, "decoder_1", None)     # FeatureDecoder: its first conv takes MX lo operands (config.mx_conv)
        mx = bool(config.mx_conv_on() and config.split_conv and d1 is not None and "d1" not in config.unsplit_layers and
                  ops.mx_conv_ok(B * h * w, 3 * D, d1[0].out_channels))
        # the one difference to the tail of ``_features_e2e``, which never asks for the MX form: kept as it is
        return self._decoder_cat(x, c, feats, c2d, shapes, (h, w), taps, mx=mx)

    # ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def features_mla(self, inp: torch.Tensor, taps: Optional[dict] = None, adapter_saves: Optional[list] = None):
        """`train_mla.py:266-383`: -> the four MLA inputs [(hi, lo|None)] in decoder argument order
        (output_last, output_last_2, output_last_3, output_last_4), each NHWC 16-bit [B, h, w, D].
        ``adapter_saves`` (train_adapters): receives, per adapter use, (saved activations of the frozen block in front of it on
        pass B | None, CAViT save, CACNN save | None) — stage 0 is CAViT alone, stages 1..3 are block -> CACNN -> CAViT."""
        inp, (B, H, W, D, h, w, N, nb) = self._begin(inp)
        m = self.model
        train = self.mode == "train_adapters" and adapter_saves is not None
        c, shapes, g, _ = self._encode(inp, train)
        Lc = c.shape[1]
        tokens = m.patch_embed(inp)
        if not config.share_patch_embed:   # pass A's own evaluation in the reference (same values)
            m.patch_embed(inp)
        # pass A (`train_mla.py:361-366`, only its last layer is used) rides along with pass B on the same weights:
        # both token batches stacked along the rows for blocks[0:-1] (see ``features``)
        xa = ops.add_cls_pos(tokens, m.cls_token.detach().reshape(-1).float().contiguous(),
                             m._pos_for(N, H, W).detach().reshape(-1, D).float().contiguous())
        Ra = B * (N + 1)
        segs = [(B, N + 1), (B, N)]
        xcat = torch.cat([xa.view(Ra, D), tokens.reshape(B * N, D)], 0)
        xcat = run_blocks(list(m.blocks[: nb - 3]), xcat, segs)
        c2d = c.view(B * Lc, D)
        x2, s_cv = self._cavit(xcat[Ra:], c2d, g, B, N, Lc, train)
        if train:
            adapter_saves.append((None, s_cv, None))
        outs = [x2]
        for j, bi in enumerate((nb - 3, nb - 2, nb - 2)):  # the reference's repeated [-2:-1]
            bsaved = None
            if train:   # pass B through the frozen block with saved activations (its input gradient is needed), pass A plain
                if j < 2:
                    xa_s = m.blocks[bi].forward_rows(xcat[:Ra], [(B, N + 1)])
                    xb_s, bsaved = m.blocks[bi].forward_train(x2.view(B, N, D))
                    xcat = torch.cat([xa_s, xb_s.reshape(B * N, D)], 0)
                    x2 = xcat[Ra:]
                else:
                    xb_s, bsaved = m.blocks[bi].forward_train(x2.view(B, N, D))
                    x2 = xb_s.reshape(B * N, D)
            elif j < 2:
                xcat[Ra:].copy_(x2)
                xcat = m.blocks[bi].forward_rows(xcat, segs)
                x2 = xcat[Ra:]
            else:
                x2 = m.blocks[bi](x2.view(B, N, D)).view(B * N, D)
            c2d, s_cn = self._cacnn(c2d, x2, g, B, Lc, N, shapes, train)
            x2, s_cv = self._cavit(x2, c2d, g, B, N, Lc, train)
            if train:
                adapter_saves.append((bsaved, s_cv, s_cn))
            outs.append(x2)
        xa = m.blocks[nb - 1](xcat[:Ra].view(B, N + 1, D))
        vit_last = m._final_norm(xa)[:, 1:]
        last = ops.add_f32(outs[3].view(B, N, D), vit_last)
        maps = [last.view(B * N, D), outs[2], outs[1], outs[0]]
        if taps is not None:
            taps.update(mla_inputs=[t.view(B, N, D) for t in maps])
        return [_hi_lo(t, B, h, w, D) for t in maps]

    @torch.no_grad()
    def train_step(self, inp: torch.Tensor, target: torch.Tensor, taps: Optional[dict] = None,
                   teacher_inp: Optional[torch.Tensor] = None, labelled=None) -> torch.Tensor:
        """One `train.py:268-436` (or `train_mla.py:260-407`) iteration; returns the loss as a 0-dim device
        tensor (no host sync).  With a ``teacher``: the teacher sees ``teacher_inp`` (default ``inp``; the same geometry), and the
        loss is hard + lambda_t kd (``taps``: ``loss_hard``, ``loss_kd``, ``kd_kept``, ``teacher_logits``, ``distill_scale``).  With
        ``mix``: the teacher sees the unmixed batch, the student's forward and the hard loss the mixed one (``taps``: ``mix_inp``,
        ``mix_target``, ``mix_sel``, ``mix_tables``, ``mix_pasted``).  ``labelled``: a host sequence of B bools (default None: every
        sample is labelled); a False needs a teacher: that sample's target row is filled with the ignore value on the device
        (what the caller put there does not matter), the hard loss leaves it out and the consistency term weighs it 1 (``taps``:
        ``labelled``, ``hard_valid``, ``sample_weight``, with ClassMix ``pseudo_target``)."""
        _check_trainable(self)
        lab = unl = sw = None
        if labelled is not None:
            lab = tuple(bool(v) for v in labelled)
            if len(lab) != inp.shape[0]:
                raise ValueError(f"train_step: labelled has {len(lab)} entries, the batch {inp.shape[0]} samples")
            if not all(lab):
                if self.teacher is None:
                    raise ValueError("train_step: an unlabelled sample needs a teacher: the consistency term is all it trains with")
                unl, sw = self._semi_tables(lab, inp.device)
        if unl is None and self.teacher is not None and self.distill_labelled_weight != 1.0:
            sw = self._semi_tables((True,) * inp.shape[0], inp.device)[1]
        g = self.ignore_index if self.ignore_index is not None else (255 if unl is not None else None)
        self._hard_ignore = g
        if g is not None and self.loss_kind not in self.IGNORE_LOSSES:
            raise ValueError(f"loss {self.loss_kind!r} has no ignore label: an unlabelled sample needs one of {self.IGNORE_LOSSES}")
        if self.teacher is not None:   # before the student's forward: the teacher's activations are gone when the student's are saved
            tmaps, tflips = self._teacher_maps(inp if teacher_inp is None else teacher_inp)
            if self.adaptive is not None:   # the batch takes part in its own thresholds: before the student's loss reads them
                self.adaptive.update(tmaps, tflips, target, self.distill_temperature, sw)
        elif teacher_inp is not None:
            raise ValueError("train_step: teacher_inp without a teacher")
        mixed = None
        if self.mix_sampler is not None:   # after the teacher, which sees the batch as it came
            if unl is None:
                inp, target, mixed = self._mix(inp, target, taps, lab)
            else:
                inp, target, mixed = self._mix(inp, target, taps, lab, unl, g, tmaps, tflips)
        if unl is not None:   # a copy: the caller's tensor keeps what it held
            target = target.long().index_fill(0, unl, g)
            if taps is not None and mixed is not None:
                taps.update(mix_target=target)
        dec = self.seg_decoder
        adapters = self.mode == "train_adapters"     # the head's input is trainable upstream: its gradient is needed
        asaves = [] if adapters else None            # what the two walks on the frozen backbone keep for the adapter backward
        if self.is_mla:
            dec_in = (self.features_mla(inp, taps, asaves),)
        elif self.train_backbone:
            dec_in, e2e = self._features_e2e(inp, taps)
        else:
            dec_in = self.features(inp, taps, asaves)
        # the UNet head alone takes the flag in its forward too: it keeps the arg-max of its first MaxPool for that gradient
        fwd_kw = {"need_input_grad": True} if (self.stream_only and adapters) else {}
        logits, saved = dec._forward_core(*dec_in, save=True, training=True, **fwd_kw)
        loss, dz, target = loss_head(self, logits, target)
        if self.teacher is not None:
            loss = self._add_consistency(logits, target, dz, loss, tmaps, tflips, config.loss_scale, taps, mixed, sw)
        if taps is not None and (g is not None or sw is not None):
            taps.update(labelled=lab, hard_valid=self.last_hard_valid if g is not None else None, sample_weight=sw)
        d16, d_lo, bpart, inv = logit_gradient(self, dz, logits)
        # every reducer this step fires, in the order they are finished below (``begin`` only resets host counters)
        reducers = []
        if self.train_backbone:
            reducers.append(self.vit_reducer)
        if self.train_encoder:
            reducers.append(self.encoder_reducer)
        if adapters:
            reducers.append(self.adapter_reducer)
        reducers.append(self.reducer)
        for r in reducers:
            r.begin()
        dgrad = dec._backward_core(saved, d16, bpart, inv, self.bucket.views, stage_done=self.reducer.stage_done, d_lo=d_lo,
                                   need_input_grad=adapters)
        if self.stream_only and (self.train_backbone or self.train_encoder):
            # UNet head: the decoder input is the adapter stream alone; the encoder / backbone backward walks take the
            # FeatureDecoder layout [stream | c4 (padded) | pass-A feature], whose other two gradient slices are zero here
            Bq, hq, wq, Dq = dgrad.shape
            full = ops.zeros((Bq, hq, wq, 3 * Dq), dgrad.device, dgrad.dtype)
            ops.copy_channels(dgrad.view(-1, Dq), full.view(-1, 3 * Dq)[:, :Dq])
            dgrad = full
        if self.train_backbone:     # fires the adapter, encoder and backbone exchanges itself, from inside the walk
            self._e2e_backward(e2e, dgrad, inv)
        elif adapters:
            dc0 = self._mla_adapter_backward(asaves, dgrad, inv) if self.is_mla else self._adapter_backward(asaves, dgrad, inv)
            self.adapter_reducer.stage_done()
            if self.train_encoder:   # on the train_mla.py flow c reaches the head through the adapters only: no c4 slice to add
                self._encoder_backward(dc0, None if self.is_mla else dgrad, inv)
                self.encoder_reducer.stage_done()
        for r in reducers:
            r.finish()
        _optimizer_step(self)
        if taps is not None:
            taps.update(logits=logits, loss=loss)
        return loss.view(())

    # ---- BASELINE config 4: the adapter flow with the backbone unfrozen ------------------------------------------------
    @torch.no_grad()
    def _features_e2e(self, inp: torch.Tensor, taps: Optional[dict] = None):
        """``features`` with everything kept for the backward: both ViT passes stacked along the rows run
        ``Block.forward_train_rows`` (so each block's weight gradients are later taken over the rows of both passes in
        one GEMM), the final norm's inputs of the last ``n_last_blocks`` outputs, CAViT / CACNN activations, the encoder's
        when it trains.  -> ((cat_hi, cat_lo|None), saved)."""
        inp, (B, H, W, D, h, w, N, nb) = self._begin(inp)
        m, nl = self.model, self.n_last_blocks
        c, shapes, g, _ = self._encode(inp, train=True)
        tokens, a16 = m.patch_tokens_train(inp)           # shared by both passes: its gradient is the sum of both
        xa = ops.add_cls_pos(tokens, m.cls_token.detach().reshape(-1).float().contiguous(),
                             m._pos_for(N, H, W).detach().reshape(-1, D).float().contiguous())
        Ra, Rb = B * (N + 1), B * N
        segs = [(B, N + 1), (B, N)]
        xcat = torch.cat([xa.view(Ra, D), tokens.reshape(Rb, D)], 0)
        bsaves, feats, fin, asaves = [], [], [], []
        # stochastic depth: this step's draws for every block, their index tables in one host-to-device copy (droppath.py)
        keeps = self.drop_path.step(segs, inp.device) if self.drop_path is not None else [None] * nb
        blk_train = lambda j, xin: m.blocks[j].forward_train_rows(xin, segs) if keeps[j] is None else \
            m.blocks[j].forward_train_rows(xin, segs, keep=keeps[j])
        for i, blk in enumerate(m.blocks[: nb - (nl - 1)]):
            xcat, sv = blk_train(i, xcat)
            bsaves.append(sv)
            if i >= nb - nl:
                feats.append(m._final_norm(xcat[:Ra].view(B, N + 1, D))[:, 1:])
                fin.append(xcat)                           # rows [:Ra] = input of that final norm (never overwritten)
        if taps is not None:
            taps.update(c=c, x_b0=xcat[Ra:].view(B, N, D).clone(), shapes=shapes)
        c2d = c.view(-1, D)
        for s in range(nl):
            if s > 0:
                xcat, sv = blk_train(nb - nl + s, xcat)
                bsaves.append(sv)
                feats.append(m._final_norm(xcat[:Ra].view(B, N + 1, D))[:, 1:])
                fin.append(xcat)
            dead = s == nl - 1 and taps is None and config.elide_dead_cacnn   # see ``features``: the last CACNN output feeds nothing
            x, c2d, saves = self._adapter_stage(xcat[Ra:], c2d, feats[s], g, shapes, dead, save=True)
            asaves.append(saves)
        # unlike ``features`` this walk does not ask for the MX form of the FeatureDecoder's lo operand: kept as it is
        cat = self._decoder_cat(x, c, feats, c2d, shapes, (h, w), taps)
        return cat, (a16, bsaves, fin, asaves, (B, N, H, W))

    def _block_done(self, i: int) -> None:
        if i in self._fire_at:
            self.vit_reducer.stage_done()

    def _e2e_backward(self, saved, dcat: torch.Tensor, inv: float) -> None:
        """Backward of ``_features_e2e``.  G = gradient of the stacked token matrix [pass A rows | pass B rows] at the
        current point of the reverse walk.  Per adapter stage (last to first): the stage output x = CAViT(x_B, c) + f_s
        sends its gradient to the CAViT output and to f_s = final_norm(pass-A block output)[:, 1:] (LayerNorm backward
        into the pass-A rows; the last feature also receives the pass-A slice of the decoder input); CACNN (when it fed a
        later stage) and CAViT run their backward; then the block in front of the stage takes G for both passes at once.
        ``model.norm``, CAViT and CACNN are used once per stage: per-stage gradient slabs summed in a fixed order."""
        a16, bsaves, fin, asaves, (B, N, H, W) = saved
        m = self.model
        D3 = dcat.shape[-1]
        D = D3 // 3
        nb, nl = len(m.blocks), self.n_last_blocks
        Ra, Rb = B * (N + 1), B * N
        dev = dcat.device
        lora = self.lora is not None      # frozen backbone weights: the blocks write their LoRA gradients, nothing else of the ViT
        ab, vg = self.adapter_bucket, (self.lora_bucket if lora else self.vit_bucket).views
        slabs = ops.zeros((nl, ab.numel), dev)
        nslab = None if lora else ops.zeros((nl, 2 * D), dev)
        nw = m.norm.weight.detach().float().contiguous()
        dcat2 = dcat.view(B * N, D3)
        G = ops.zeros((Ra + Rb, D), dev)
        ops.copy_channels(dcat2[:, :D], G[Ra:])
        dvit = torch.empty((B * N, D), device=dev, dtype=torch.float32)       # pass-A slice of the decoder input
        ops.copy_channels(dcat2[:, 2 * D:], dvit)
        dc_next = None
        for s in range(nl - 1, -1, -1):
            # d f_s: the stage's residual add, + the decoder input's third slice for the last feature
            dyA = ops.zeros((B, N + 1, D), dev)
            ops.copy_channels(G[Ra:].view(B, N * D), dyA.view(B, (N + 1) * D)[:, D:])
            if s == nl - 1:
                ops.add_f32(dyA[:, 1:], dvit.view(B, N, D), out=dyA[:, 1:])
            Gn = torch.empty((Ra + Rb, D), device=dev, dtype=torch.float32)
            _, part = ops.layernorm_bwd(dyA.view(Ra, D), fin[s][:Ra], nw, m.norm.eps, res=G[:Ra], out=Gn[:Ra])
            if not lora:
                ops.reduce_rows(part.view(part.shape[0], 2 * D), inv, nslab[s])
            gs = self._slab_views(slabs, s)
            dx_in, dc_next = self._adapter_stage_backward(*asaves[s], G[Ra:].view(B, N, D), dc_next, gs, inv)
            ops.copy_channels(dx_in, Gn[Ra:])
            if s == 0:   # every use of model.norm / CAViT / CACNN has contributed: finish their gradients, start the exchanges
                if not lora:
                    red = ops.reduce_rows(nslab, 1.0)
                    vg["norm.weight"].copy_(red[:D]); vg["norm.bias"].copy_(red[D:])
                self._block_done(nb)
                ops.reduce_rows(slabs, 1.0, ab.grad)
                self.adapter_reducer.stage_done()
                if self.train_encoder:
                    self._encoder_backward(dc_next, dcat, inv)
                    self.encoder_reducer.stage_done()
            bi = nb - nl + s
            G = m.blocks[bi].backward(bsaves[bi], Gn, inv, vg, f"blocks.{bi}")
            bsaves[bi] = None
            self._block_done(bi)
        for i in range(nb - nl - 1, -1, -1):
            G = m.blocks[i].backward(bsaves[i], G, inv, vg, f"blocks.{i}")
            bsaves[i] = None
            self._block_done(i)
        if not lora:
            m.embed_backward(a16, G[:Ra].view(B, N + 1, D), G[Ra:], H, W, inv, vg)
        self._block_done(-1)

    def _adapter_backward(self, asaves, dcat: torch.Tensor, inv: float) -> torch.Tensor:
        """(``dcat`` [B, h, w, 3D] = gradient of the FeatureDecoder input concat, or [B, h, w, D] = gradient of the
        adapter-stream map alone for the UNet head.)
        Backward of the four adapter stages (`train.py:304-387` under autograd, minus its no_grad):
        d cat[..., :D] is the gradient of the adapter stream; the c4 and pass-A slices of the decoder input come from
        the frozen encoder / backbone.  Per stage, in reverse: x = x2 + feat (identity), CACNN (only when its output
        fed a later stage: the last one is dead code in the reference flow), CAViT, and the input gradient of the
        frozen ViT block in front of the stage (``_slab_views``: one gradient slab per stage)."""
        m = self.model
        B, h, w, D3 = dcat.shape
        D = m.embed_dim
        N = h * w
        nl = self.n_last_blocks
        nb = len(m.blocks)
        ab = self.adapter_bucket
        slabs = ops.zeros((nl, ab.numel), dcat.device)
        dx = torch.empty((B * N, D), device=dcat.device, dtype=torch.float32)
        ops.copy_channels(dcat.view(B * N, D3)[:, :D], dx)
        dc_next = None
        for s in range(nl - 1, -1, -1):
            bsaved, s_cv, s_cn = asaves[s]
            dx_in, dc_next = self._adapter_stage_backward(s_cv, s_cn, dx.view(B, N, D), dc_next, self._slab_views(slabs, s), inv)
            if s > 0:
                dx = m.blocks[nb - (nl - 1) + s - 1].backward(bsaved, dx_in, inv, None)
        ops.reduce_rows(slabs, 1.0, ab.grad)
        return dc_next  # gradient of the encoder's pyramid tokens c (stage-0 input), fp32 [B*Lc, D]

    def _mla_adapter_backward(self, asaves, dmaps, inv: float) -> torch.Tensor:
        """Backward of the four adapter uses of the `train_mla.py:300-383` flow: x0 = CAViT(x, c0); for j = 1..3:
        x = block_j(x_{j-1}), c_j = CACNN(c_{j-1}, x), x_j = CAViT(x, c_j); MLA inputs (x3 + f, x2, x1, x0).
        ``dmaps``: gradients of the four MLA inputs in decoder argument order, fp32 [B, h, w, D], times the loss scale.
        Writes the adapter bucket; -> gradient of the encoder's pyramid tokens c0, fp32 [B * Lc, D]."""
        m, cv, cn = self.model, self.cross_vit, self.cross_cnn
        nb = len(m.blocks)
        B, h, w, D = dmaps[0].shape
        N = h * w
        ab = self.adapter_bucket
        slabs = ops.zeros((4, ab.numel), dmaps[0].device)
        d_out = [dmaps[3], dmaps[2], dmaps[1], dmaps[0]]          # gradients of x0, x1, x2, x3
        dx = d_out[3].reshape(B * N, D).contiguous()
        dc_from_next = None                                        # gradient of c_j through CACNN_{j+1}'s query input
        for j in (3, 2, 1):
            bsaved, s_cv, s_cn = asaves[j]
            gs = self._slab_views(slabs, j)
            dx_q, dc_j = cv.backward16(s_cv, dx, inv, gs, "cross_vit")          # query (block output) and feat (c_j)
            if dc_from_next is not None:
                Lc = dc_j.shape[0] // B
                ops.add_f32(dc_j.view(B, Lc, D), dc_from_next.view(B, Lc, D), out=dc_j.view(B, Lc, D))
            dc_from_next, dx_f = cn.backward16(s_cn, dc_j, inv, gs, "cross_cnn")  # c_{j-1} and the block output as CACNN's feat
            dxb = ops.add_f32(dx_q.view(B, N, D), dx_f.view(B, N, D)).view(B * N, D)
            bi = (nb - 3, nb - 2, nb - 2)[j - 1]
            dx_prev = m.blocks[bi].backward(bsaved, dxb, inv, None)
            dx = ops.add_f32(dx_prev.view(B, N, D), d_out[j - 1].reshape(B, N, D)).view(B * N, D)
        _, dc0 = cv.backward16(asaves[0][1], dx, inv, self._slab_views(slabs, 0), "cross_vit")
        Lc = dc0.shape[0] // B
        ops.add_f32(dc0.view(B, Lc, D), dc_from_next.view(B, Lc, D), out=dc0.view(B, Lc, D))
        ops.reduce_rows(slabs, 1.0, ab.grad)
        return dc0

    def _encoder_backward(self, dc0: torch.Tensor, dcat: torch.Tensor, inv: float) -> None:
        """d c = what the adapter stages send back + the c4 slice of the decoder input (`train.py:395-400`: c4 is
        zero-padded, centred, into channels [D, 2D) of the concat) -> FeatureEncoder.backward_tokens."""
        esaved, shapes = self._esaved
        self._esaved = None
        D = self.model.embed_dim
        if dcat is None:            # train_mla.py flow: c reaches the head through the adapters only
            dc = dc0.view(-1, sum(a * b for a, b in shapes), D)
        else:
            B, h, w, D3 = dcat.shape
            h4, w4 = shapes[2]
            n4 = h4 * w4
            Lc = dc0.shape[0] // B
            top, left = (h - h4) // 2, (w - w4) // 2
            d4 = dcat[:, top:top + h4, left:left + w4, D:2 * D].reshape(B, n4, D).contiguous()
            dc = dc0.view(B, Lc, D)
            ops.add_f32(dc[:, Lc - n4:], d4, out=dc[:, Lc - n4:])
        gviews = {n[len("backbone_encoder."):]: v for n, v in self.encoder_bucket.views.items()}
        self.backbone_encoder.backward_tokens(esaved, dc, inv, gviews)

    @torch.no_grad()
    def eval_logits(self, inp: torch.Tensor) -> torch.Tensor:
        """Decoder logits, NHWC fp32, with the decoder's BatchNorm in its current train/eval mode.  With LoRA the frozen forward
        runs on the merged weights W + s B A (``LoRA.merged``)."""
        with (self.lora.merged(self.model) if self.lora is not None else contextlib.nullcontext()):
            if self.is_mla:
                logits, _ = self.seg_decoder._forward_core(self.features_mla(inp), save=False)
            else:
                logits, _ = self.seg_decoder._forward_core(*self.features(inp), save=False)
        return logits

    @torch.no_grad()
    def validate_step(self, inp: torch.Tensor, target: torch.Tensor, ce_weight: Optional[torch.Tensor] = None,
                      with_counts: bool = False):
        """`train.py:465-642` for one batch: -> device tensor [4] = (weighted CE, dice, pixel accuracy, n_images).
        The decoder runs in eval mode (running BatchNorm statistics, `train.py:451`); the encoder's SyncBatchNorm
        stays in train mode exactly like the reference."""
        was = self.seg_decoder.training
        self.seg_decoder.eval()
        logits = self.eval_logits(inp)
        self.seg_decoder.train(was)
        target = target.long().contiguous()
        if with_counts:  # + per-class pixel counts [C,3] for ch_iou / isi_iou (train_multi_class.py:582-589)
            m, counts = ops.ce_acc(logits, target, ce_weight, counts=True)
        else:
            m = ops.ce_acc(logits, target, ce_weight)
        loss1, _, _ = ops.dice_fwd(logits, target, 1, 10e-20, 1.0)
        return (m, loss1, counts) if with_counts else (m, loss1)

    @torch.no_grad()
    def _guarded_logits(self, inps) -> List[torch.Tensor]:
        """``eval_logits`` of every input under the guard of prediction: decoder in eval mode, the encoder's running statistics
        not updated, both restored afterwards, also when a forward raises."""
        enc = self.backbone_encoder
        was, upd = self.seg_decoder.training, enc.update_running_stats
        self.seg_decoder.eval()
        enc.update_running_stats = False
        try:
            return [self.eval_logits(inp) for inp in inps]
        finally:
            self.seg_decoder.train(was)
            enc.update_running_stats = upd

    @torch.no_grad()
    def predict(self, inp: torch.Tensor, size=None, **kw):
        """Masks of ``inp`` (float [B,3,S,S] as validation feeds it) at ``size`` = (H, W) (None: the input's own), uint8 [B,H,W]:
        ``ops.predict_mask`` (keywords: ``encode``, ``frames`` / ``palette`` / ``alpha`` for the overlay, ``target`` / ``lut``
        for the per-class counts) on the logits ``validate_step`` sees — decoder in eval mode and restored afterwards, the
        encoder's SyncBatchNorm in train mode as validation leaves it, so a frame's mask depends on the batch it is predicted
        in exactly as the validation metrics do.  Forward only: no optimizer state, BatchNorm running buffer
        or saved activation of a training step is touched."""
        logits = self._guarded_logits([inp])[0]
        return ops.predict_mask(logits, tuple(inp.shape[-2:]) if size is None else size, **kw)

    @torch.no_grad()
    def predict_views(self, inps, flips, size, **kw):
        """Test-time augmentation: masks at ``size`` = (H, W) from several views of one batch.  ``inps[k]`` is float [B,3,S_k,S_k]
        as validation feeds it (the sizes may differ; a mirrored view is given mirrored), ``flips[k]`` tells whether view k is
        mirrored.  ``eval_logits`` runs once per view under the guard of ``predict`` (decoder in eval mode, the encoder's running
        statistics not updated, both restored afterwards), so the encoder's BatchNorm normalises every view with that view's own
        batch statistics; one ``ops.predict_mask_views`` call then averages the class probabilities of the views at native size
        (keywords as there: ``encode``, ``confidence``, ``frames`` / ``palette`` / ``alpha``, ``target`` / ``lut``)."""
        inps, flips = list(inps), list(flips)
        if len(inps) != len(flips):
            raise ValueError(f"predict_views: {len(inps)} inputs and {len(flips)} flips")
        return ops.predict_mask_views(self._guarded_logits(inps), size, flips=flips, **kw)

    @torch.no_grad()
    def predict_tiles(self, inps, tiles, work, size, **kw):
        """Sliding-window prediction: masks at ``size`` = (H, W) from several tiles of one batch.  ``inps[k]`` is float [B,3,S,S]
        as validation feeds it: the crop (or, for a context tile, the resized whole) of the working frame ``work`` = (Lh, Lw)
        that ``tiles[k]`` = (oy, ox, sy, sx, flip) names, given mirrored when ``flip``.  ``eval_logits`` runs once per tile under
        the guard of ``predict`` (decoder in eval mode, the encoder's running statistics not updated, both restored afterwards).
        Each tile is its own forward of batch B, so the encoder's BatchNorm normalises every tile with that tile's own batch
        statistics: the tiles of a frame differ by more than their place, and a frame's mask still depends on the batch it is
        predicted in.  One ``ops.predict_mask_tiles`` call then blends the class probabilities of the tiles at native size
        (keywords as there: ``encode``, ``blend``, ``ramp``, ``confidence``, ``frames`` / ``palette`` / ``alpha``, ``target`` /
        ``lut``)."""
        inps, tiles = list(inps), list(tiles)
        if len(inps) != len(tiles):
            raise ValueError(f"predict_tiles: {len(inps)} inputs and {len(tiles)} tiles")
        return ops.predict_mask_tiles(self._guarded_logits(inps), tiles, work, size, **kw)


def make_optimizer(kind: str, buckets, *, lr, momentum, weight_decay, betas=(0.9, 0.999), eps=1e-8, clip_grad=None, no_decay=True,
                   layer_decay=None, depth=None):
    """The engines' ``optimizer=`` switch: "sgd" builds exactly the ``optim.SGD`` they always built, "adamw" an ``optim.AdamW``."""
    if kind == "sgd":
        if clip_grad is not None:
            raise ValueError("clip_grad needs optimizer='adamw': the SGD kernels do not clip")
        if layer_decay is not None and any(d is not None for d in layer_decay):
            raise ValueError("layer_decay needs optimizer='adamw'")
        return SGD(buckets, lr=lr, momentum=momentum, weight_decay=weight_decay)
    if kind == "adamw":
        return AdamW(buckets, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, clip_grad=clip_grad, no_decay=no_decay,
                     layer_decay=layer_decay, depth=depth)
    raise ValueError("optimizer must be 'sgd' or 'adamw'")


def make_drop_path_sampler(model, seed: int, process_group=None):
    """the ``DropPathSampler`` of an engine that trains ``model``'s blocks, seeded with this process's rank; None when every
    block's ``sample_drop_ratio`` is 0 (nothing changes on that path)"""
    rates = [float(getattr(blk, "sample_drop_ratio", 0.0)) for blk in model.blocks]
    if not any(rates):
        return None
    rank = dist.get_rank(process_group) if (dist.is_available() and dist.is_initialized()) else 0
    return DropPathSampler(rates, seed=seed, rank=rank)


def make_vit_bucket(model, blocks_per_bucket: int, process_group, momentum: bool = False, min_first_blocks: int = 0,
                    compress: Optional[str] = None):
    """Flat gradient bucket of the whole backbone in gradient-ready order (final norm, blocks last..first, then the token
    embedding parameters) + a reducer over ``blocks_per_bucket``-block chunks (the last chunk takes the embeddings along).
    -> (bucket, reducer, fire_at) with fire_at = block indices after whose backward the next chunk is complete (-1 = after
    the embedding backward).  ``min_first_blocks``: the first chunk (which holds ``norm.*``) does not fire before that many
    blocks are done — the adapter flow writes the final-norm gradients only after its ``n_last_blocks`` stages, so a smaller
    first chunk would be all-reduced before they exist."""
    vnamed = dict(model.named_parameters())
    depth = len(model.blocks)
    groups = [[n for n in vnamed if n.startswith("norm.")]]
    groups += [[n for n in vnamed if n.startswith(f"blocks.{i}.")] for i in range(depth - 1, -1, -1)]
    groups.append([n for n in vnamed if not n.startswith("norm.") and not n.startswith("blocks.")])
    assert sum(len(g) for g in groups) == len(vnamed)
    for p in model.parameters():
        p.requires_grad_(True)
    bucket = FlatBucket([(n, vnamed[n]) for g in groups for n in g], momentum=momentum)
    fire_at, ranges, start = [], [], 0
    for j in range(1, depth + 1):                       # j = number of blocks finished
        if j % blocks_per_bucket == 0 and j != depth and j >= min_first_blocks:
            names = [n for g in groups[start:j + 1] for n in g]
            ranges.append(bucket.range_of(names)); fire_at.append(depth - j); start = j + 1
    ranges.append(bucket.range_of([n for g in groups[start:] for n in g])); fire_at.append(-1)
    return bucket, StageReducer(bucket.grad, ranges, process_group, compress=compress), fire_at


class EndToEndEngine(nn.Module):
    """BASELINE config 4 — the unfrozen end-to-end variant (`eval/eval_dinov2_setr_cross_ete.py:145-148,307-361`):

        x_norm_patchtokens = model(inp, is_training=True)          whole ViT under autograd / DDP
        logits = seg_decoder(tokens as (B, D, h, w)) ; resize to the label size ; loss = CE + DC(2)
        backward through the decoder AND all ViT blocks ; DDP all-reduces every gradient
        optimizer.step() on the decoder only (`:224-229` — the backbone gradients are computed and exchanged, then
        discarded; reproduced as written, DESIGN.md "config 4").

    The ViT runs ``forward_train`` / ``backward`` (fused attention forward+backward, LayerNorm / GELU / LayerScale
    backward kernels, weight-gradient GEMMs); its gradients live in a gradient-only flat bucket that is all-reduced
    in ``blocks_per_bucket``-block chunks on the side stream while earlier blocks are still in their backward.
    """

    def __init__(self, model, seg_decoder, *, lr: float = 0.01, momentum: float = 0.9, weight_decay: float = 0.0,
                 loss: str = "ce_dc", process_group=None, blocks_per_bucket: int = 4, optimizer: str = "sgd",
                 betas=(0.9, 0.999), eps: float = 1e-8, clip_grad: Optional[float] = None, no_decay: bool = True,
                 drop_path_seed: int = 0, lora_rank: Optional[int] = None, ema_decay: Optional[float] = None,
                 ema_warmup: bool = True):
        """``ema_decay`` / ``ema_warmup``: as in ``SegEngine``; the optimizer steps the decoder bucket alone, so that is what is
        averaged (``self.ema``, ``ema_weights()``)."""
        super().__init__()
        if lora_rank is not None:
            raise ValueError("EndToEndEngine trains every backbone weight: LoRA (lora_rank) is built for SegEngine's adapter flow")
        self.drop_path = make_drop_path_sampler(model, drop_path_seed, process_group)   # stochastic depth of ``train_step``
        if loss not in SegEngine.LOSSES:
            raise ValueError(f"loss must be one of {sorted(SegEngine.LOSSES)}")
        self.model, self.seg_decoder, self.loss_kind, self.process_group = model, seg_decoder, loss, process_group
        self.patch = model.patch_size
        for p in model.parameters():
            p.requires_grad_(True)
        self.bucket, self.stage_ranges = make_decoder_bucket(seg_decoder)
        self.optimizer = make_optimizer(optimizer, [self.bucket], lr=lr, momentum=momentum, weight_decay=weight_decay, betas=betas,
                                        eps=eps, clip_grad=clip_grad, no_decay=no_decay)
        self.ema = make_ema(self.optimizer, ema_decay, ema_warmup)
        self.reducer = StageReducer(self.bucket.grad, self.stage_ranges, process_group)
        # backbone: gradient-ready order = final norm, blocks last..first, then the token embedding parameters; reduced
        # after every `blocks_per_bucket` blocks
        self.vit_bucket, self.vit_reducer, self._fire_at = make_vit_bucket(model, blocks_per_bucket, process_group)

    ema_weights = ema_weights

    def _block_done(self, i: int) -> None:
        if i in self._fire_at:
            self.vit_reducer.stage_done()

    @torch.no_grad()
    def train_step(self, inp: torch.Tensor, target: torch.Tensor, taps: Optional[dict] = None) -> torch.Tensor:
        _check_trainable(self)
        m, dec = self.model, self.seg_decoder
        B, _, H, W = inp.shape
        h, w = H // self.patch, W // self.patch
        N, D = h * w, m.embed_dim
        if self.drop_path is not None:
            tok, vsaved = m.forward_train(inp, keep=self.drop_path.step([(B, N + 1)], inp.device))
        else:
            tok, vsaved = m.forward_train(inp)
        t2 = torch.empty((B * N, D), device=inp.device, dtype=torch.float32)
        ops.copy_channels(vsaved_tokens_view(tok, B, N, D), t2.view(B, N * D))
        logits, saved = dec._forward_core(*_hi_lo(t2, B, h, w, D), save=True, training=True)
        loss, dz, _ = loss_head(self, logits, target)
        d16, d_lo, bpart, inv = logit_gradient(self, dz, logits)
        self.reducer.begin()
        self.vit_reducer.begin()
        dX = dec._backward_core(saved, d16, bpart, inv, self.bucket.views, stage_done=self.reducer.stage_done, d_lo=d_lo,
                                need_input_grad=True)
        m.backward(vsaved, dX.view(B, N, D), inv, self.vit_bucket.views, block_done=self._block_done)
        self.reducer.finish()
        self.vit_reducer.finish()
        _optimizer_step(self)
        if taps is not None:
            taps.update(logits=logits, loss=loss, tokens=t2.view(B, N, D))
        return loss.view(())


def vsaved_tokens_view(tok: torch.Tensor, B: int, N: int, D: int) -> torch.Tensor:
    """x_norm_patchtokens is the [:, 1:] view of the (B, N+1, D) normalised tokens: as [B, N*D] rows with the batch
    stride of the full tensor (what asis_copy_channels compacts)."""
    return tok.as_strided((B, N * D), (tok.stride(0), 1))
