"""Drop-in for the reference's `train.py`: same CLI (`train.py:654-683`), same function signatures
(`train_seg` :63, `train` :260, `validate_network` :449), same checkpoint / log formats (:244-255) — the step
body runs on the HIP engine (`backbones.engines.SegEngine`) instead of eager PyTorch modules.

    python -m adaptersis_amd.train --arch vit_large --patch_size 14 --imsize 588 --batch_size_per_gpu 12 \
        --data_path synthetic --epochs 1 --output_dir /tmp/out
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m adaptersis_amd.train ...

Differences forced by the environment (no network, no torchvision/albumentations/omegaconf here): the four
`configs/eval/vit*14_pretrain.yaml` files reduce to the arch table below; `--data_path synthetic` (default when the
path does not exist) trains on the synthetic set of SURVEY.md §8d; `--data_path <dir>` expects ``images.npy``
(N,3,H,W float in [0,1]) and ``masks.npy`` (N,H,W int) per split directory (``train/``, ``validation/``).
"""
from __future__ import annotations

import argparse
import contextlib
import json
import math
import os
from pathlib import Path
from typing import Optional

import torch
from torch import nn

from .backbones.adapter_blocks import CACNN, CAViT
from .backbones.decoders import DecoderMLA, FeatureDecoder
from .backbones.encoders import FeatureEncoder
from . import config, parallel
from .backbones.engines import SegEngine
from .dinov2.models import vision_transformer as vits
from .utils import misc as utils
from .utils import weights as W

ARCH_FFN = {"vit_tiny_test": "mlp", "vit_small": "mlp", "vit_base": "mlp", "vit_large": "mlp", "vit_giant2": "swiglufused"}
_ENGINES = {}


class _SegData(torch.utils.data.Dataset):
    """(img float[0,1] CHW, mask long HW, index) like `tools/dataset.py:127-167`."""

    def __init__(self, path, split, imsize, n_synth=24, num_classes=2):
        d = os.path.join(path, split)
        if os.path.isfile(os.path.join(d, "images.npy")):
            import numpy as np
            self.img = torch.from_numpy(np.load(os.path.join(d, "images.npy"))).float()
            self.msk = torch.from_numpy(np.load(os.path.join(d, "masks.npy"))).long()
        else:
            self.img, self.msk = W.synthetic_batch(n_synth, imsize, num_classes, seed=1 if split == "train" else 2)

    def __len__(self):
        return self.img.shape[0]

    def __getitem__(self, i):
        return self.img[i], self.msk[i], i


_AUGMENTERS = {}
_IDENTITY = {"crop": None, "flip": False, "rotk": 0, "alpha": 1.0, "beta": 0.0, "gamma": None}


_LAST_STRONG = {"applied": None}   # the share of the last strong batch's samples with a strong draw, counted on the host


def _to_device_batch(inp, target, train: bool, non_rigid_p: float = 0.0, weak: bool = False, strong=None, strong_apply=None):
    """Batch from the loader -> (float [B,3,S,S] in [0,1], long [B,S,S]) on the device.  uint8 HWC batches (``tools.dataset.Robomis``
    without a host transform) go through the GPU augmentation pipeline (`train.py:139-163`) when training, and through the same
    kernel with identity parameters (= `/255`, `tools/dataset.py:159`; the reference's val transform is a no-op Resize to the
    image size, `train.py:119-122`) when validating.  A ``tools.dataset.collate_frames`` batch (native-size frames) is uploaded and
    resized on the device first (``ops.frame_resize``, PIL-exact), then takes the same uint8 path.
    ``weak`` (training batches, --distill_weak): -> (inp, target, teacher_inp), the third the same frames under the same drawn
    geometry without the photometric stage (``tools.augment.weak_params``: a second ``ops.augment`` call, no further draw); a batch
    that does not go through the GPU augmentation has no photometric stage, its ``teacher_inp`` is ``inp`` itself.
    ``strong`` (training batches, --aug_strong: the ``strong`` configuration of ``TrainAugment``): -> (inp, target, teacher_inp) as
    well; ``inp`` is the strong view (``ops.strong_view``, out of place) of the samples ``strong_apply`` names (a sequence of truth
    values; default all), ``teacher_inp`` the tensor in front of it, or with ``weak`` the geometry-only view as above: the strong
    stage never reaches a teacher.  The strong draws come from a generator of their own: crop, flip, CLAHE and the tables are those
    of the call without ``strong``.  A batch that does not go through the GPU augmentation is left alone, as for ``weak``."""
    from .tools.dataset import FrameBatch
    if isinstance(inp, FrameBatch):
        inp, target = _resize_frames(inp)
    inp, target = inp.cuda(non_blocking=True), target.cuda(non_blocking=True)
    strong = strong if train else None
    if inp.dtype != torch.uint8:
        if strong is not None:
            _LAST_STRONG["applied"] = 0.0
        return (inp, target, inp) if weak or strong is not None else (inp, target)
    from .tools.augment import TrainAugment
    S = inp.shape[1]
    aug = _AUGMENTERS.get(S)
    if strong is not None:
        from .tools.augment import _strong_config
        strong = _strong_config(strong)
    # --aug_non_rigid, --aug_strong: training batches only
    if aug is None or (train and (aug.non_rigid_p != non_rigid_p or aug.strong != strong)):
        aug = _AUGMENTERS[S] = TrainAugment(size=S, seed=1000 + utils.get_rank(), non_rigid_p=non_rigid_p if train else 0.0,
                                            strong=strong)
    img, msk = inp.contiguous(), target.to(torch.uint8).contiguous()
    if not weak and strong is None:
        return aug(img, msk, None if train else [dict(_IDENTITY) for _ in range(inp.shape[0])])
    from .tools.augment import weak_params
    if strong is None:
        x, y, params = aug(img, msk, None, return_params=True)
        return x, y, aug(img, msk, weak_params(params))[0]
    if strong_apply is not None and len(strong_apply) != inp.shape[0]:
        raise ValueError(f"_to_device_batch: strong_apply has {len(strong_apply)} entries, the batch has {inp.shape[0]} samples")
    x, y, params, pre = aug(img, msk, None, return_params=True, return_strong=True, strong_apply=strong_apply)
    drawn = [p.get("strong") is not None and (strong_apply is None or bool(strong_apply[b])) for b, p in enumerate(params)]
    _LAST_STRONG["applied"] = sum(drawn) / max(1, len(drawn))
    return x, y, (aug(img, msk, weak_params(params))[0] if weak else pre)


def _append_unlabelled(inp, target, frames, masks):
    """The loader's labelled batch followed by the unlabelled frames (uint8 [U,S,S,3], masks of 255) -> (inp, target, labelled) on
    the device, in the labelled batch's own form: a uint8 batch (a ``FrameBatch`` is resized first) stays uint8 and goes through
    the GPU augmentation as one batch; a float batch takes the frames as float CHW / 255."""
    from .tools.dataset import FrameBatch
    if isinstance(inp, FrameBatch):
        inp, target = _resize_frames(inp)
    inp, target = inp.cuda(non_blocking=True), target.cuda(non_blocking=True)
    frames, masks = frames.cuda(non_blocking=True), masks.cuda(non_blocking=True)
    labelled = [True] * inp.shape[0] + [False] * frames.shape[0]
    if inp.dtype == torch.uint8:
        return torch.cat([inp, frames]), torch.cat([target.to(torch.uint8), masks]), labelled
    return torch.cat([inp, frames.permute(0, 3, 1, 2).to(inp.dtype) / 255.0]), torch.cat([target, masks.to(target.dtype)]), labelled


def _resize_frames(fb):
    """FrameBatch -> (uint8 [B,S,S,3], uint8 [B,S,S] labels) on the device; items the collate already resized on the host
    are put back in their places."""
    from . import ops
    fb = fb.to("cuda", non_blocking=True)
    img, msk = ops.frame_resize(fb.frames, fb.masks, fb.size, fb.lut)
    if fb.host_pos.numel() == 0:
        return img, msk
    B, S = fb.shape[0], fb.size
    full_img = torch.empty((B, S, S, 3), device=img.device, dtype=torch.uint8)
    full_msk = torch.empty((B, S, S), device=img.device, dtype=torch.uint8)
    full_img[fb.pos], full_msk[fb.pos] = img, msk
    full_img[fb.host_pos], full_msk[fb.host_pos] = fb.host_frames, fb.host_masks
    return full_img, full_msk


def _open_datasets(args):
    """-> (train set, val set, collate_fn).  ``--data_path`` with the reference's layout (`images/<split>/*.png` +
    `annotations/<split>/`, `tools/dataset.py:127-141`) or decode-free ``<split>/images.npy`` uint8 arrays -> ``Robomis`` +
    GPU augmentation; otherwise the float ``.npy`` / synthetic set of ``_SegData``."""
    from .tools.dataset import Robomis, collate_u8
    p = args.data_path
    if os.path.isdir(os.path.join(p, "images", "training")) or os.path.isfile(os.path.join(p, "training", "images.npy")):
        return (Robomis(p, "training", transform=None, imsize=args.imsize), Robomis(p, "validation", transform=None, imsize=args.imsize),
                collate_u8)
    return _SegData(p, "train", args.imsize), _SegData(p, "validation", args.imsize), None


class BatchShardSampler(torch.utils.data.Sampler):
    """``batch_sampler`` of the sharded validation (``--shard_val``): the val set in its natural order cut into batches of
    ``batch_size`` exactly as the reference's sequential loader cuts it (`train.py:125-130`), rank r takes batches
    r, r + world, ...  No padding, no duplicates: ranks may hold different batch counts (validation issues no collective per
    batch — `parallel.local_batchnorm`); every batch has the composition, hence the BatchNorm statistics, of the reference's."""

    def __init__(self, n: int, batch_size: int, rank: int, world: int):
        self.batches = [list(range(i, min(i + batch_size, n))) for i in range(0, n, batch_size)][rank::world]

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


def broadcast_module_states(modules, src: int = 0, group=None) -> None:
    """What ``DistributedDataParallel.__init__`` does for the reference (`train.py:84-116`): every parameter and buffer of
    the trainable / SyncBN modules takes rank ``src``'s value.  One flat fp32 message per module (plus one for integer
    buffers), no-op without an initialised process group."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return
    with torch.no_grad():
        for m in modules:
            ts = [t for t in list(m.parameters()) + list(m.buffers())]
            for dtype in sorted({t.dtype for t in ts}, key=str):
                part = [t for t in ts if t.dtype == dtype]
                flat = torch.cat([t.detach().reshape(-1) for t in part])
                dist.broadcast(flat, src, group=group)
                o = 0
                for t in part:
                    t.copy_(flat[o:o + t.numel()].view(t.shape))
                    o += t.numel()


def _engine_for(model, backbone_encoder, cross_vit, cross_cnn, seg_decoder, lr=0.01, momentum=0.99, weight_decay=3e-5,
                mode="reference_exact", train_encoder=False, num_classes=2, loss="dice", **optimizer_args):
    key = id(seg_decoder)
    if key not in _ENGINES:
        _ENGINES[key] = SegEngine(model, backbone_encoder, cross_vit, cross_cnn, seg_decoder, lr=lr, momentum=momentum,
                                  weight_decay=weight_decay, mode=mode, train_encoder=train_encoder, num_classes=num_classes,
                                  loss=loss, **optimizer_args)
    return _ENGINES[key]


def _optimizer_args(args) -> dict:
    """The optimizer flags of ``get_args_parser`` as ``SegEngine`` arguments (a namespace built without them: the SGD defaults)."""
    kind = getattr(args, "optimizer", "sgd")
    if kind == "sgd":   # clip_grad / layer_decay are passed on so that the engine rejects them
        return {"optimizer": "sgd", "clip_grad": getattr(args, "clip_grad", None), "layer_decay": getattr(args, "layer_decay", None)}
    return {"optimizer": kind, "betas": (args.adam_beta1, args.adam_beta2), "eps": args.adam_eps, "clip_grad": args.clip_grad,
            "layer_decay": args.layer_decay}


def _backbone_args(args) -> dict:
    """The backbone fine-tuning flags (--train_backbone, --optimize_backbone, --drop_path_seed) as ``SegEngine`` arguments; a
    namespace built without them, or with all of them at their defaults: nothing is passed and the engine is what it was."""
    out = {}
    if getattr(args, "train_backbone", False):
        out["train_backbone"] = True
    if getattr(args, "optimize_backbone", False):
        out["optimize_backbone"] = True
    if getattr(args, "drop_path_seed", 0):
        out["drop_path_seed"] = int(args.drop_path_seed)
    if getattr(args, "lora_rank", None) is not None:      # LoRA on q / v (lora.py); the engine rejects what it excludes
        out["lora_rank"] = int(args.lora_rank)
        out["lora_alpha"] = getattr(args, "lora_alpha", None)
    return out


def check_backbone_args(args) -> Optional[str]:
    """What is wrong with the combination of the backbone fine-tuning flags, or None"""
    if getattr(args, "train_backbone", False) and not getattr(args, "train_adapters", False):
        return "--train_backbone needs --train_adapters (the unfrozen variant of the adapter flow)"
    if getattr(args, "optimize_backbone", False) and not getattr(args, "train_backbone", False):
        return "--optimize_backbone needs --train_backbone"
    r = float(getattr(args, "drop_path", 0.0))
    if not 0.0 <= r < 1.0:
        return "--drop_path must be in [0, 1)"
    if r > 0.0 and not getattr(args, "train_backbone", False):
        return "--drop_path drops samples in the training forward of the ViT blocks: it needs --train_backbone"
    if getattr(args, "lora_alpha", None) is not None and getattr(args, "lora_rank", None) is None:
        return "--lora_alpha needs --lora_rank"
    if getattr(args, "lora_rank", None) is not None:
        if not (getattr(args, "train_adapters", False) and getattr(args, "train_backbone", False)):
            return "--lora_rank needs --train_adapters --train_backbone (LoRA runs the backbone's training forward)"
        if getattr(args, "optimize_backbone", False):
            return "--lora_rank and --optimize_backbone exclude each other (with LoRA the backbone weights stay frozen)"
        if r > 0.0:
            return "--lora_rank needs --drop_path 0"
    d = getattr(args, "ema_decay", None)
    if d is not None and not 0.0 < float(d) < 1.0:
        return "--ema_decay must lie in (0, 1)"
    if d is None and (getattr(args, "ema_no_warmup", False) or getattr(args, "ema_validate_live", False)):
        return "--ema_no_warmup / --ema_validate_live need --ema_decay"
    return None


DISTILL_FLAGS = ("distill_teacher_arch", "distill_teacher_ema", "distill_weight", "distill_temperature", "distill_threshold",
                 "distill_rampup", "distill_flip", "distill_weak", "distill_class_thresholds", "distill_adaptive_threshold",
                 "distill_adaptive_momentum")


def check_distill_args(args) -> Optional[str]:
    """What is wrong with the combination of the mean-teacher flags (--distill_*), or None.  Needs no device and no process group."""
    t = getattr(args, "distill_teacher", None)
    if t is None:
        given = [f for f in DISTILL_FLAGS if getattr(args, f, None) is not None and getattr(args, f) is not False]
        return f"--{given[0]} needs --distill_teacher (ema or the path of a checkpoint)" if given else None
    if t == "ema":
        if getattr(args, "ema_decay", None) is None:
            return "--distill_teacher ema needs --ema_decay: the teacher is the average of the weights"
        if getattr(args, "distill_teacher_arch", None) is not None or getattr(args, "distill_teacher_ema", False):
            return "--distill_teacher_arch / --distill_teacher_ema describe a checkpoint teacher: not with --distill_teacher ema"
    elif not os.path.isfile(t):
        return f"--distill_teacher {t}: no such checkpoint (ema, or the path of a file train_seg wrote)"
    elif getattr(args, "distill_teacher_arch", None) is not None and args.distill_teacher_arch not in ARCH_FFN:
        return f"--distill_teacher_arch must be one of {sorted(ARCH_FFN)}"
    w, T = getattr(args, "distill_weight", None), getattr(args, "distill_temperature", None)
    th, R = getattr(args, "distill_threshold", None), getattr(args, "distill_rampup", None)
    if w is not None and not float(w) >= 0.0:
        return "--distill_weight must be >= 0"
    if T is not None and not float(T) > 0.0:
        return "--distill_temperature must be > 0"
    if th is not None and not float(th) <= 1.0:
        return "--distill_threshold must be at most 1 (0 or less keeps every pixel)"
    if R is not None and int(R) < 0:
        return "--distill_rampup counts steps: it must be >= 0"
    ct, ad = getattr(args, "distill_class_thresholds", None), bool(getattr(args, "distill_adaptive_threshold", False))
    m = getattr(args, "distill_adaptive_momentum", None)
    if ct is not None and ad:
        return "--distill_class_thresholds sets the thresholds by hand, --distill_adaptive_threshold adapts them: pick one"
    if (ct is not None or ad) and th is not None:
        return "--distill_threshold is one threshold for every class: not with --distill_class_thresholds / --distill_adaptive_threshold"
    if ct is not None and not all(math.isfinite(float(v)) for v in ct):
        return "--distill_class_thresholds must be finite (0 or less keeps every pixel of a class, above 1 drops them all)"
    nc = getattr(args, "num_classes", None)
    if ct is not None and nc is not None and len(ct) != int(nc):
        return f"--distill_class_thresholds has {len(ct)} values for --num_classes {int(nc)}"
    if m is not None and not ad:
        return "--distill_adaptive_momentum needs --distill_adaptive_threshold"
    if m is not None and not 0.0 <= float(m) < 1.0:
        return "--distill_adaptive_momentum must lie in [0, 1)"
    return None


def _distill_engine_args(args, teacher) -> dict:
    """The mean-teacher flags as ``SegEngine`` arguments (``teacher``: "ema" or the engine ``build_teacher`` made); without
    --distill_teacher nothing is passed and the engine is what it was."""
    if teacher is None:
        return {}
    pick = lambda name, default: default if getattr(args, name, None) is None else getattr(args, name)
    out = {"teacher": teacher, "distill_weight": float(pick("distill_weight", 1.0)),
           "distill_temperature": float(pick("distill_temperature", 1.0)), "distill_threshold": getattr(args, "distill_threshold", None),
           "distill_rampup": int(pick("distill_rampup", 0)), "distill_flip": bool(getattr(args, "distill_flip", False))}
    if getattr(args, "distill_adaptive_threshold", False):   # the keywords are passed only with the flags
        out.update(distill_class_thresholds="adaptive", distill_adaptive_momentum=float(pick("distill_adaptive_momentum", 0.999)))
    elif getattr(args, "distill_class_thresholds", None) is not None:
        out.update(distill_class_thresholds=[float(v) for v in args.distill_class_thresholds])
    return out


def teacher_shares_backbone(args, src: dict) -> bool:
    """Whether a checkpoint teacher runs on the student's ViT module: the same architecture, a student that does not step the
    backbone weights (no --optimize_backbone) and a teacher file (``src``: the entry loaded) without a 'backbone' / 'lora' entry;
    otherwise the teacher owns one."""
    same = (getattr(args, "distill_teacher_arch", None) or args.arch) == args.arch
    return same and not getattr(args, "optimize_backbone", False) and "backbone" not in src and "lora" not in src


def build_teacher(args, head: str, num_classes: int, dev, student_model) -> SegEngine:
    """The frozen teacher of --distill_teacher PATH: modules as ``build_modules`` makes them for --distill_teacher_arch (default:
    the student's), the checkpoint loaded as ``adaptersis_amd.predict`` loads it (--distill_teacher_ema: its 'ema' entry), one
    ``SegEngine`` that is never stepped."""
    import copy
    from . import predict as _p
    from .lora import LoRA
    path = args.distill_teacher
    ck = _p.read_checkpoint(path)
    _p.modules_not_in_checkpoint(ck, None, path)
    src = ck
    if getattr(args, "distill_teacher_ema", False):
        src = ck.get("ema")
        if not isinstance(src, dict) or "state_dict" not in src:
            raise ValueError(f"{path} holds no 'ema' entry: --distill_teacher_ema needs a checkpoint of a run with --ema_decay")
    targs = copy.copy(args)
    targs.arch = getattr(args, "distill_teacher_arch", None) or args.arch
    targs.drop_path = 0.0
    shared = teacher_shares_backbone(args, src)
    model, enc, cv, cn, dec = build_modules(targs, head, num_classes, dev, model=student_model if shared else None)
    eng = SegEngine(model, enc, cv, cn, dec, num_classes=num_classes)
    _p.load_checkpoint(path, dec, {"cross_vit": cv, "cross_cnn": cn, "backbone_encoder": enc, "backbone": model},
                       hint=f" (the teacher: --distill_teacher_arch {targs.arch}, {num_classes} classes)", ck=src)
    if "lora" in src:
        eng.lora = LoRA.from_state(model, src["lora"])
    print(f"teacher: loaded {path} (epoch {ck.get('epoch')}" + ("; averaged weights" if src is not ck else "")
          + ("; on the student's ViT" if shared else "; on a ViT of its own") + ")")
    return eng


MIX_FLAGS = ("mix_p", "mix_seed", "mix_background")


def check_mix_args(args) -> Optional[str]:
    """What is wrong with the combination of the batch-mixing flags (--mix, --mix_*), or None.  Needs no device and no process group."""
    from .tools.mix import KINDS
    kind = getattr(args, "mix", None)
    if kind is None:
        given = [f for f in MIX_FLAGS if getattr(args, f, None) is not None and getattr(args, f) is not False]
        return f"--{given[0]} needs --mix ({' or '.join(sorted(KINDS))})" if given else None
    if kind not in KINDS:
        return f"--mix must be one of {sorted(KINDS)}"
    p = getattr(args, "mix_p", None)
    if p is not None and not 0.0 <= float(p) <= 1.0:
        return "--mix_p must be a probability in [0, 1]"
    bs = getattr(args, "batch_size_per_gpu", None)
    if bs is not None and int(bs) < 2:
        return "--mix pastes pixels of another sample of the rank's batch: it needs --batch_size_per_gpu of at least 2"
    return None


def _mix_engine_args(args) -> dict:
    """The batch-mixing flags as ``SegEngine`` arguments; without --mix nothing is passed and the engine is what it was."""
    if getattr(args, "mix", None) is None:
        return {}
    pick = lambda name, default: default if getattr(args, name, None) is None else getattr(args, name)
    return {"mix": args.mix, "mix_p": float(pick("mix_p", 1.0)), "mix_seed": int(pick("mix_seed", 0)),
            "mix_background": bool(getattr(args, "mix_background", False))}


STRONG_FLAGS = ("aug_strong_jitter", "aug_strong_grey", "aug_strong_blur")


def check_strong_args(args) -> Optional[str]:
    """What is wrong with the combination of the strong-view flags (--aug_strong, --aug_strong_*), or None.  Needs no device and no
    process group."""
    on = getattr(args, "aug_strong_on", None) or "all"
    if not getattr(args, "aug_strong", False):
        given = [f for f in STRONG_FLAGS if getattr(args, f, None) is not None]
        if on != "all":
            given.append("aug_strong_on")
        return f"--{given[0]} needs --aug_strong" if given else None
    jit = getattr(args, "aug_strong_jitter", None)
    if jit is not None:
        if len(jit) != 4 or not all(0.0 <= float(v) <= 1.0 for v in jit[:3]) or not 0.0 <= float(jit[3]) <= 0.5:
            return "--aug_strong_jitter takes B C S H: brightness, contrast and saturation in [0, 1], hue in [0, 0.5]"
    for f in ("aug_strong_grey", "aug_strong_blur"):
        v = getattr(args, f, None)
        if v is not None and not 0.0 <= float(v) <= 1.0:
            return f"--{f} must be a probability in [0, 1]"
    if on not in ("all", "unlabelled"):
        return "--aug_strong_on must be all or unlabelled"
    if on == "unlabelled" and getattr(args, "unlabelled_path", None) is None:
        return "--aug_strong_on unlabelled needs --unlabelled_path: without it no sample would get the strong view"
    return None


def _strong_config(args) -> Optional[dict]:
    """The strong-view flags as the ``strong`` argument of ``tools.augment.TrainAugment``; None without --aug_strong."""
    if not getattr(args, "aug_strong", False):
        return None
    out = {}
    if getattr(args, "aug_strong_jitter", None) is not None:
        out["jitter"] = tuple(float(v) for v in args.aug_strong_jitter)
    if getattr(args, "aug_strong_grey", None) is not None:
        out["grey_p"] = float(args.aug_strong_grey)
    if getattr(args, "aug_strong_blur", None) is not None:
        out["blur_p"] = float(args.aug_strong_blur)
    return out


class _MixEntry:
    """the ``mix`` entry of a checkpoint as ``restart_from_checkpoint`` sees it: the step the next draw is seeded with"""

    def __init__(self, engine):
        self.engine = engine

    def load_state_dict(self, entry):
        self.engine.mix_step = int(entry["step"])
        return f"<mix step {self.engine.mix_step}>"


class _DistillEntry:
    """the ``distill`` entry of a checkpoint as ``restart_from_checkpoint`` sees it: the step count of the ramp-up"""

    def __init__(self, engine):
        self.engine = engine

    def load_state_dict(self, entry):
        self.engine.distill_step = int(entry["step"])
        adaptive = getattr(self.engine, "adaptive", None)
        if adaptive is not None:   # --distill_adaptive_threshold: tau and the class averages
            if "adaptive" in entry:
                adaptive.load_state_dict(entry["adaptive"])
            else:
                print("=> the checkpoint's 'distill' entry holds no adaptive thresholds: they start from tau = ptilde = 1 / C")
        return f"<distill step {self.engine.distill_step}>"


SEMI_FLAGS = ("unlabelled_per_batch", "distill_labelled_weight")


def check_semi_args(args, loss: Optional[str] = None) -> Optional[str]:
    """What is wrong with the combination of the semi-supervision flags (--unlabelled_path, --unlabelled_per_batch, --ignore_index,
    --distill_labelled_weight), or None.  ``loss``: the loss the run trains with (default --loss).  Needs no device and no
    process group."""
    path, g = getattr(args, "unlabelled_path", None), getattr(args, "ignore_index", None)
    loss = loss or getattr(args, "loss", "dice")
    if path is not None and getattr(args, "distill_teacher", None) is None:
        return "--unlabelled_path needs --distill_teacher: the consistency term is all an unlabelled frame trains with"
    if path is None and getattr(args, "unlabelled_per_batch", None) is not None:
        return "--unlabelled_per_batch needs --unlabelled_path (a directory of frames, or synthetic)"
    if getattr(args, "distill_labelled_weight", None) is not None:
        if getattr(args, "distill_teacher", None) is None:
            return "--distill_labelled_weight needs --distill_teacher (ema or the path of a checkpoint)"
        if not 0.0 <= float(args.distill_labelled_weight) < float("inf"):
            return "--distill_labelled_weight must be finite and >= 0"
    if path is not None and path != "synthetic" and not os.path.isdir(path):
        return f"--unlabelled_path {path}: no such directory (a directory of *.png / *.jpg frames, or synthetic)"
    u = getattr(args, "unlabelled_per_batch", None)
    if u is not None and int(u) < 1:
        return "--unlabelled_per_batch must be at least 1"
    if (path is not None or g is not None) and loss not in SegEngine.IGNORE_LOSSES:
        flag = "--ignore_index" if g is not None else "--unlabelled_path"
        return f"{flag} needs a loss with an ignore label (--loss one of {', '.join(SegEngine.IGNORE_LOSSES)}), not {loss}"
    return None


def _semi_engine_args(args) -> dict:
    """The semi-supervision flags as ``SegEngine`` arguments; without them nothing is passed and the engine is what it was."""
    out = {}
    if getattr(args, "ignore_index", None) is not None:
        out["ignore_index"] = int(args.ignore_index)
    if getattr(args, "distill_labelled_weight", None) is not None:
        out["distill_labelled_weight"] = float(args.distill_labelled_weight)
    return out


class UnlabelledStream:
    """The unlabelled half of a step's batch (--unlabelled_path): ``tools.dataset.UnlabelledFrames`` behind a
    ``DistributedSampler`` and an epoch counter of its own.  ``next()`` -> (uint8 [U,S,S,3] frames, uint8 [U,S,S] masks of 255);
    when the rank's share is used up the epoch is counted and the stream starts over under that epoch's shuffle.  The labelled
    loader's epochs and the learning-rate schedule do not see it.  ``epoch`` is what the checkpoint's ``semi`` entry holds."""

    def __init__(self, dataset, per_batch: int, num_workers: int = 0):
        from .tools.dataset import collate_u8
        self.dataset, self.per_batch, self.epoch, self._it = dataset, int(per_batch), 0, None
        self.sampler = torch.utils.data.distributed.DistributedSampler(dataset, num_replicas=utils.get_world_size(),
                                                                       rank=utils.get_rank())
        self.loader = torch.utils.data.DataLoader(dataset, sampler=self.sampler, batch_size=self.per_batch, num_workers=num_workers,
                                                  pin_memory=True, collate_fn=collate_u8, drop_last=len(self.sampler) >= self.per_batch)

    def next(self):
        for _ in range(2):
            if self._it is None:
                self.sampler.set_epoch(self.epoch)
                self._it = iter(self.loader)
            try:
                frames, masks, _ = next(self._it)
                return frames, masks
            except StopIteration:
                self._it = None
                self.epoch += 1
        raise RuntimeError("the unlabelled stream gave no frame")

    def load_state_dict(self, entry):
        """the ``semi`` entry of a checkpoint as ``restart_from_checkpoint`` sees it: the unlabelled epoch"""
        self.epoch, self._it = int(entry["epoch"]), None
        return f"<unlabelled epoch {self.epoch}>"


def _ema_args(args) -> dict:
    """The weight-averaging flags (--ema_decay, --ema_no_warmup) as ``SegEngine`` arguments; without --ema_decay nothing is passed
    and the engine is what it was."""
    if getattr(args, "ema_decay", None) is None:
        return {}
    return {"ema_decay": float(args.ema_decay), "ema_warmup": not getattr(args, "ema_no_warmup", False)}


class _EmaEntry:
    """the ``ema`` entry of a checkpoint as ``restart_from_checkpoint`` sees it: loaded into the engine's average"""

    def __init__(self, engine):
        self.engine, self.loaded = engine, False

    def load_state_dict(self, entry):
        msg = self.engine.load_ema_state_dict(entry)
        self.loaded = True
        return msg


def _loss_args(args) -> dict:
    """The parameters of the hard-pixel losses (--topk_percent, --focal_gamma) as ``SegEngine`` arguments."""
    return {"topk_percent": getattr(args, "topk_percent", 10.0), "focal_gamma": getattr(args, "focal_gamma", 2.0)}


def _build_vit(args, arch: str, dev):
    # dinov2/eval/setup.py:62-75 + models/__init__.py:14-29 (teacher, img_size 518, layerscale 1e-5, block_chunks 0)
    model = vits.__dict__[arch](patch_size=args.patch_size, img_size=518, init_values=1e-5, ffn_layer=ARCH_FFN[arch],
                                block_chunks=0, drop_path_rate=float(getattr(args, "drop_path", 0.0)),
                                drop_path_uniform=bool(getattr(args, "drop_path_uniform", False)))
    if args.pretrained_weights and os.path.isfile(args.pretrained_weights):
        utils.load_pretrained_weights(model, args.pretrained_weights, args.checkpoint_key)   # dinov2/utils/utils.py:20-33
    else:
        model.load_state_dict(W.make_vit_state_dict(arch, patch_size=args.patch_size, layerscale="init"))
        print("No pretrained weights: deterministic synthetic initialisation (adaptersis_amd.utils.weights)")
    return model.to(dev).eval()


def build_modules(args, head: str, num_classes: int, dev, model=None):
    """The five modules of `train.py:170-191` on ``dev``, constructed in the reference's order (so a seeded run draws the same
    initial weights wherever it is called from: ``train_seg`` and ``adaptersis_amd.predict``):
    -> (model, backbone_encoder, cross_vit, cross_cnn, seg_decoder).  ``model``: a ViT of this architecture that exists already
    (a teacher on the student's backbone): none is built."""
    arch = args.arch if args.arch in ARCH_FFN else "vit_large"
    D = W.VIT_CONFIGS[arch][0]
    if model is None:
        model = _build_vit(args, arch, dev)
    backbone_encoder = FeatureEncoder(embed_dim=D).to(dev)
    cross_vit = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4).to(dev)
    cross_cnn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25).to(dev)
    if head == "mla":
        seg_decoder = DecoderMLA(img_size=args.imsize, mla_channels=D, num_classes=num_classes).to(dev)
    else:
        seg_decoder = FeatureDecoder(embed_dim=D, num_classes=num_classes, features=[D, 512, 256, 128, 64]).to(dev)
    return model, backbone_encoder, cross_vit, cross_cnn, seg_decoder


def train_seg(args, head: str = "feature", *, num_classes: int = 2, loss: Optional[str] = None, open_datasets=None, validate=None):
    """``head``: "feature" = `train.py` (FeatureDecoder, SGD lr / 0.99 / 3e-5, `train.py:178-191`); "mla" = `train_mla.py`
    (DecoderMLA, SGD lr * batch * world / 16, momentum 0.9, no weight decay, `train_mla.py:178-184`).
    ``num_classes`` (head and engine), ``loss`` (a key of ``SegEngine.LOSSES``; default: ``--loss``, "dice" in a namespace
    built without it), ``open_datasets(args) -> (train set, val set,
    collate_fn)`` and ``validate`` (signature of ``validate_network``) are what `train_multi_class.py` changes; the defaults
    are `train.py`'s."""
    open_datasets = open_datasets or _open_datasets
    validate = validate or validate_network
    if loss is None:
        loss = getattr(args, "loss", "dice")
    non_rigid_p = float(getattr(args, "aug_non_rigid", 0.0))
    if not 0.0 <= non_rigid_p <= 1.0:
        raise ValueError("--aug_non_rigid must be a probability in [0, 1]")
    bad = (check_backbone_args(args) or check_distill_args(args) or check_mix_args(args) or check_semi_args(args, loss)
           or check_strong_args(args))
    if bad:
        raise ValueError(bad)
    utils.init_distributed_mode(args)
    print("\n".join("%s: %s" % (k, str(v)) for k, v in sorted(dict(vars(args)).items())))
    dev = torch.device("cuda", args.gpu)
    model, backbone_encoder, cross_vit, cross_cnn, seg_decoder = build_modules(args, head, num_classes, dev)
    feature_model = model  # ModelWithIntermediateLayers(model, 4, autocast) collapses into the engine's pass A
    # the reference wraps these four modules in DistributedDataParallel (`train.py:84-116`), whose constructor broadcasts
    # rank 0's parameters and buffers: without it every rank would train its own randomly initialised copy
    broadcast_module_states([backbone_encoder, cross_vit, cross_cnn, seg_decoder])
    wd = getattr(args, "weight_decay", None)   # --weight_decay; default: the script's own value
    # --distill_teacher: "ema" = the engine's own average; a path = a frozen engine built after the student's modules (whose
    # initial draws are then those of a run without the flag)
    teacher = getattr(args, "distill_teacher", None)
    if teacher is not None and teacher != "ema":
        teacher = build_teacher(args, head, num_classes, dev, model)
    distill = {**_distill_engine_args(args, teacher), **_mix_engine_args(args), **_semi_engine_args(args)}
    if head == "mla":
        lr = args.lr * (args.batch_size_per_gpu * utils.get_world_size()) / 16.0  # linear scaling rule
        engine = _engine_for(model, backbone_encoder, cross_vit, cross_cnn, seg_decoder, lr=lr, momentum=0.9,
                             weight_decay=0.0 if wd is None else wd, num_classes=num_classes, loss=loss, **_optimizer_args(args),
                             **_loss_args(args), **_backbone_args(args), **_ema_args(args), **distill)
    else:
        engine = _engine_for(model, backbone_encoder, cross_vit, cross_cnn, seg_decoder, lr=args.lr,
                             weight_decay=3e-5 if wd is None else wd,
                             mode="train_adapters" if getattr(args, "train_adapters", False) else "reference_exact",
                             train_encoder=getattr(args, "train_encoder", False), num_classes=num_classes, loss=loss,
                             **_optimizer_args(args), **_loss_args(args), **_backbone_args(args), **_ema_args(args), **distill)
    optimizer = engine.optimizer
    engine.aug_non_rigid = non_rigid_p      # read by train(): its signature is the reference's and carries no arguments
    engine.distill_weak = bool(getattr(args, "distill_weak", False))
    engine.mix_rank = utils.get_rank()      # --mix: every rank draws its own tables
    engine.unlabelled = None                # --unlabelled_path: read by train(), like aug_non_rigid
    engine.aug_strong = _strong_config(args)   # --aug_strong: None, or the strong configuration of the augmenter; read by train()
    engine.aug_strong_on = getattr(args, "aug_strong_on", None) or "all"

    dataset_train, dataset_val, collate = open_datasets(args)
    workers = args.num_workers if collate is not None else 0      # PNG decode runs in loader workers; tensors in memory do not need any
    if getattr(args, "shard_val", False) and utils.get_world_size() > 1:
        # the reference lets all ranks evaluate the whole val set; here every rank takes every world-th batch
        val_loader = torch.utils.data.DataLoader(dataset_val, num_workers=workers, pin_memory=True, collate_fn=collate,
                                                 batch_sampler=BatchShardSampler(len(dataset_val), args.batch_size_per_gpu,
                                                                                 utils.get_rank(), utils.get_world_size()))
    else:
        val_loader = torch.utils.data.DataLoader(dataset_val, batch_size=args.batch_size_per_gpu, num_workers=workers, pin_memory=True,
                                                 collate_fn=collate)
    sampler = torch.utils.data.distributed.DistributedSampler(dataset_train, num_replicas=utils.get_world_size(),
                                                               rank=utils.get_rank())
    train_loader = torch.utils.data.DataLoader(dataset_train, sampler=sampler, batch_size=args.batch_size_per_gpu,
                                               num_workers=workers, pin_memory=True, collate_fn=collate)   # no drop_last: train.py:168-174
    if getattr(args, "unlabelled_path", None) is not None:
        from .tools.dataset import UnlabelledFrames
        unl_set = UnlabelledFrames(args.unlabelled_path, args.imsize)
        per = getattr(args, "unlabelled_per_batch", None)
        engine.unlabelled = UnlabelledStream(unl_set, args.batch_size_per_gpu if per is None else per,
                                             0 if args.unlabelled_path == "synthetic" else args.num_workers)
        print(f"Unlabelled stream: {len(unl_set)} frames, {engine.unlabelled.per_batch} a step.")
    print(f"Data loaded with {len(dataset_train)} train and {len(dataset_val)} val imgs.")

    class _Cosine:  # torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, epochs, eta_min=0), stepped per epoch
        def __init__(self, opt, T):
            self.opt, self.T, self.e = opt, T, 0
            self.base = [g["lr"] for g in opt.param_groups]

        def step(self):
            self.e += 1
            for g, b in zip(self.opt.param_groups, self.base):
                g["lr"] = b * (1 + math.cos(math.pi * self.e / self.T)) / 2

        def state_dict(self):
            return {"last_epoch": self.e, "base_lrs": self.base, "T_max": self.T}

        def load_state_dict(self, sd):
            self.e = sd["last_epoch"]
            for g, b in zip(self.opt.param_groups, self.base):
                g["lr"] = b * (1 + math.cos(math.pi * self.e / self.T)) / 2

    scheduler = _Cosine(optimizer, args.epochs)
    to_restore = {"epoch": 0, "best_acc": 0.0}
    # reference keys (`train.py:244-255`) + the adapters / encoder when they train (without them a resume
    # would put the restored momentum on freshly re-randomised weights)
    extra = {}
    if engine.mode == "train_adapters":
        extra = {"cross_vit": cross_vit, "cross_cnn": cross_cnn}
        if engine.train_encoder:
            extra["backbone_encoder"] = backbone_encoder
        if getattr(args, "optimize_backbone", False):   # a fine-tuned ViT is part of the trained model: saved and restored
            extra["backbone"] = model
    lora = getattr(engine, "lora", None)       # --lora_rank: the checkpoint gains a "lora" entry (parameters, rank, alpha)
    # --ema_decay: the checkpoint gains an "ema" entry; it is restored after the live modules, and a file without one restarts
    # the average from the weights just restored
    ema_entry = None if engine.ema is None else _EmaEntry(engine)
    ckpt_path = os.path.join(args.output_dir, "checkpoint.pth.tar")
    resumed = os.path.isfile(ckpt_path)
    utils.restart_from_checkpoint(ckpt_path, run_variables=to_restore,
                                  state_dict=seg_decoder, **extra, **({} if lora is None else {"lora": lora}), optimizer=optimizer,
                                  scheduler=scheduler, **({} if ema_entry is None else {"ema": ema_entry}),
                                  **({} if engine.teacher is None else {"distill": _DistillEntry(engine)}),
                                  **({} if engine.mix_sampler is None else {"mix": _MixEntry(engine)}),
                                  **({} if engine.unlabelled is None else {"semi": engine.unlabelled}))
    if ema_entry is not None and resumed and not ema_entry.loaded:
        engine.ema.reset()
        print(f"=> no usable 'ema' entry in '{ckpt_path}': the average starts from the restored live weights")
    start_epoch, best_acc = to_restore["epoch"], to_restore["best_acc"]
    live_validate = validate

    def validate(*a):
        """with --ema_decay the metrics are those of the averaged weights; --ema_validate_live adds the live ones as live_*"""
        if engine.ema is None:
            return live_validate(*a)
        with engine.ema_weights():
            stats = live_validate(*a)
        if getattr(args, "ema_validate_live", False):
            stats = {**stats, **{f"live_{k}": v for k, v in live_validate(*a).items()}}
        return stats

    if args.evaluate:
        stats = validate(val_loader, model, feature_model, backbone_encoder, cross_vit, cross_cnn, seg_decoder,
                                 args.n_last_blocks, args.avgpool_patchtokens)
        print(f"Accuracy of the network on the {len(dataset_val)} test images: {stats['acc1']:.1f}%")
        return stats
    log_stats = {}
    for epoch in range(start_epoch, args.epochs):
        train_loader.sampler.set_epoch(epoch)
        train_stats = train(model, feature_model, backbone_encoder, cross_vit, cross_cnn, seg_decoder, optimizer,
                            train_loader, epoch, args.n_last_blocks, args.avgpool_patchtokens)
        scheduler.step()
        log_stats = {**{f"train_{k}": v for k, v in train_stats.items()}, "epoch": epoch}
        if getattr(engine, "class_thresholds", None) is not None:   # behind the synchronize of the epoch's last step
            log_stats["distill_class_thr"] = [float(v) for v in engine.class_thresholds.tolist()]
        if epoch % args.val_freq == 0 or epoch == args.epochs - 1:
            test_stats = validate(val_loader, model, feature_model, backbone_encoder, cross_vit, cross_cnn,
                                          seg_decoder, args.n_last_blocks, args.avgpool_patchtokens)
            print(f"Accuracy at epoch {epoch} of the network on the {len(dataset_val)} test images: {test_stats['acc1']:.1f}%")
            best_acc = max(best_acc, test_stats["acc1"])
            print(f"Max accuracy so far: {best_acc:.2f}%")
            log_stats = {**log_stats, **{f"test_{k}": v for k, v in test_stats.items()}}
        if utils.is_main_process():
            Path(args.output_dir).mkdir(parents=True, exist_ok=True)
            with (Path(args.output_dir) / "log.txt").open("a") as f:
                f.write(json.dumps(log_stats) + "\n")
            ckpt = {"epoch": epoch + 1,
                    "state_dict": {"module." + k: v for k, v in seg_decoder.state_dict().items()},  # DDP prefix kept
                    "optimizer": optimizer.state_dict(), "scheduler": scheduler.state_dict(), "best_acc": best_acc}
            for k, mod in extra.items():
                ckpt[k] = {"module." + n: v for n, v in mod.state_dict().items()}
            if lora is not None:
                ckpt["lora"] = lora.state_dict()
            if engine.ema is not None:
                ckpt["ema"] = engine.ema_state_dict()
            if engine.teacher is not None:     # --distill_teacher: where the ramp-up of the consistency weight stands
                ckpt["distill"] = {"step": engine.distill_step}
                if getattr(engine, "adaptive", None) is not None:   # --distill_adaptive_threshold: tau and the class averages
                    ckpt["distill"]["adaptive"] = engine.adaptive.state_dict()
            if engine.mix_sampler is not None:  # --mix: the step the next draw is seeded with
                ckpt["mix"] = {"step": engine.mix_step}
            if engine.unlabelled is not None:   # --unlabelled_path: the epoch of the unlabelled stream
                ckpt["semi"] = {"epoch": engine.unlabelled.epoch}
            torch.save(ckpt, os.path.join(args.output_dir, "checkpoint.pth.tar"))
    print("Training of the supervised linear classifier on frozen features completed.\n"
          "Top-1 test accuracy: {acc:.1f}".format(acc=best_acc))
    return log_stats


def train(model, feature_model, backbone_encoder, cross_vit, cross_cnn, seg_decoder, optimizer, loader, epoch, n, avgpool):
    """`train.py:260-445`; the body of the loop is ``SegEngine.train_step``."""
    seg_decoder.train()
    engine = _engine_for(model, backbone_encoder, cross_vit, cross_cnn, seg_decoder)
    if optimizer is not engine.optimizer:
        raise ValueError("train(): pass the engine's optimizer (engine.optimizer: adaptersis_amd.optim.SGD or AdamW over the "
                         "flat buckets)")
    metric_logger = utils.MetricLogger(delimiter="  ")
    metric_logger.add_meter("lr", utils.SmoothedValue(window_size=1, fmt="{value:.6f}"))
    with_norm = hasattr(optimizer, "last_grad_norm")   # optim.AdamW: one more scalar read behind the step's synchronize
    # SyncBatchNorm element counts: with the reference's DistributedSampler every rank holds the same number of images in every
    # iteration (also in the short last batch); any other loader may not, so the ranks' batch sizes are exchanged per step
    ragged = parallel.collectives_on() and not isinstance(getattr(loader, "sampler", None),
                                                          torch.utils.data.distributed.DistributedSampler)
    stream = getattr(engine, "unlabelled", None)
    strong = getattr(engine, "aug_strong", None)
    for (inp, target, idx) in metric_logger.log_every(loader, 20, "Epoch: [{}]".format(epoch)):
        if ragged:
            parallel.set_batch_ratio(int(inp.shape[0]))
        labelled = None
        if stream is not None:   # the labelled batch followed by the unlabelled frames, through the augmentation in one call
            inp, target, labelled = _append_unlabelled(inp, target, *stream.next())
        skw = {}
        if strong is not None:   # --aug_strong: the student's view; --aug_strong_on unlabelled: of the unlabelled frames alone
            only_unl = getattr(engine, "aug_strong_on", "all") == "unlabelled" and labelled is not None
            skw = {"strong": strong, "strong_apply": [not l for l in labelled] if only_unl else None}
        batch = _to_device_batch(inp, target, train=True, non_rigid_p=getattr(engine, "aug_non_rigid", 0.0),
                                 weak=engine.teacher is not None and getattr(engine, "distill_weak", False), **skw)
        if strong is not None and engine.teacher is None:   # nobody takes the view in front of the strong stage
            batch = batch[:2]
        if labelled is None:
            loss = engine.train_step(batch[0], batch[1], None, *batch[2:])
        else:
            loss = engine.train_step(batch[0], batch[1], None, *batch[2:], labelled=labelled)
        torch.cuda.synchronize()  # the reference syncs and reads the loss every step (train.py:439-440)
        metric_logger.update(loss=loss.item())
        if engine.teacher is not None:     # the soft term and the share of the pixels its confidence gate let through
            metric_logger.update(loss_kd=engine.last_loss_kd.item(), kd_kept=engine.last_kd_kept.item() / batch[1].numel())
            if getattr(engine, "adaptive", None) is not None:   # the global threshold the class thresholds are scaled from
                metric_logger.update(kd_tau=engine.adaptive.state[0].item())
        if stream is not None or getattr(engine, "ignore_index", None) is not None:   # the share of the pixels that carry a label
            metric_logger.update(hard_valid=int(engine.last_hard_valid.sum()) / batch[1].numel())
        if engine.mix_sampler is not None:  # the share of the batch's pixels that came from another sample
            pasted = engine.last_mix_pasted
            metric_logger.update(mix_pasted=0.0 if pasted is None else int(pasted.sum()) / batch[1].numel())
        if strong is not None:              # the share of the samples with a strong draw
            metric_logger.update(strong_applied=_LAST_STRONG["applied"])
        metric_logger.update(lr=optimizer.param_groups[0]["lr"])
        if with_norm:
            metric_logger.update(grad_norm=optimizer.last_grad_norm)
    if ragged:
        parallel.set_batch_ratio(None)
    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    # overflow guard of the static 16-bit loss scale (optim.SGD / optim.AdamW): a step whose gradients hold an inf / NaN is skipped on the
    # device.  One host read per epoch; an epoch in which EVERY step was skipped means the scale is too large for this data —
    # the reference's torch.optim.SGD has no skip, so a silent stall would be a behaviour change.
    skipped = optimizer.skipped_steps
    prev = getattr(optimizer, "_skipped_reported", 0)
    optimizer._skipped_reported = skipped
    if skipped > prev:
        print(f"WARNING: {skipped - prev} of {len(loader)} optimizer steps of epoch {epoch} were skipped (non-finite gradients "
              f"under loss scale {config.loss_scale:g}); lower ASIS_LOSS_SCALE if this persists")
        if len(loader) > 0 and skipped - prev >= len(loader):
            raise RuntimeError(f"every optimizer step of epoch {epoch} was skipped: non-finite gradients under the static loss "
                               f"scale {config.loss_scale:g} (set ASIS_LOSS_SCALE to a smaller power of two)")
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def _val_meters():
    """The validation MetricLogger with its three meters created up front, in a fixed order, on EVERY rank: with ``--shard_val``
    a rank whose shard is empty (fewer batches than ranks) must issue the same barrier + all-reduce per meter in
    ``synchronize_between_processes`` as the others, or the job hangs; the summary line reads all three."""
    ml = utils.MetricLogger(delimiter="  ")
    for name in ("loss", "acc1", "dice"):
        ml.meters[name]
    return ml


def _val_summary(metric_logger) -> str:
    return "* Acc@1 {top1.global_avg:.3f} loss {losses.global_avg:.3f} Dice {dice.global_avg:.3f}".format(
        top1=metric_logger.acc1, losses=metric_logger.loss, dice=metric_logger.meters["dice"])


@torch.no_grad()
def validate_network(val_loader, model, feature_model, backbone_encoder, cross_vit, cross_cnn, seg_decoder, n, avgpool):
    """`train.py:448-651`: weighted CE ([0.1, 10]), dice = 1 - DC(logits), pixel accuracy; decoder in eval mode."""
    engine = _engine_for(model, backbone_encoder, cross_vit, cross_cnn, seg_decoder)
    metric_logger = _val_meters()
    wt = torch.tensor([0.1, 10.0], device=next(seg_decoder.parameters()).device)
    sharded = isinstance(getattr(val_loader, "batch_sampler", None), BatchShardSampler)
    with (parallel.local_batchnorm() if sharded else contextlib.nullcontext()):
        for (inp, target, idx) in metric_logger.log_every(val_loader, 20, "Test:"):
            inp, target = _to_device_batch(inp, target, train=False)
            m, dloss = engine.validate_step(inp, target, wt)
            m = m.cpu()
            bs = inp.shape[0]
            metric_logger.update(loss=float(m[0] / m[1]))
            metric_logger.meters["acc1"].update(float(m[2]) / target.numel(), n=bs)
            metric_logger.meters["dice"].update(1.0 - float(dloss), n=bs)
    if sharded:   # per-rank sums -> the whole-set averages every rank of the reference computes redundantly
        metric_logger.synchronize_between_processes()
    print(_val_summary(metric_logger))
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


class _ArgumentParser(argparse.ArgumentParser):
    """``ArgumentParser`` that also rejects combinations of the backbone fine-tuning flags no engine can be built from
    (``check_backbone_args``), as a usage error like any other"""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        bad = check_backbone_args(ns) or check_distill_args(ns) or check_mix_args(ns) or check_semi_args(ns) or check_strong_args(ns)
        if bad:
            self.error(bad)
        return ns, rest


def get_args_parser():
    p = _ArgumentParser("Evaluation with semantic segmentation on RobustMIS2019")
    p.add_argument("--n_last_blocks", default=4, type=int)
    p.add_argument("--avgpool_patchtokens", default=False, type=utils.bool_flag)
    p.add_argument("--arch", default="vit_large", type=str)
    p.add_argument("--patch_size", default=14, type=int)
    p.add_argument("--imsize", default=588, type=int)
    p.add_argument("--checkpoint_key", default="teacher", type=str)
    p.add_argument("--epochs", default=100, type=int)
    p.add_argument("--lr", default=0.01, type=float)
    p.add_argument("--batch_size_per_gpu", default=12, type=int)
    p.add_argument("--dist_url", default="env://", type=str)
    p.add_argument("--local-rank", default=0, type=int)
    p.add_argument("--data_path", default="synthetic", type=str)
    p.add_argument("--num_workers", default=10, type=int)
    p.add_argument("--val_freq", default=1, type=int)
    p.add_argument("--output_dir", default=".")
    p.add_argument("--opts", default=[], nargs=argparse.REMAINDER)
    p.add_argument("--num_labels", default=1000, type=int)
    p.add_argument("--evaluate", dest="evaluate", action="store_true")
    p.add_argument("--config_file", type=str)
    p.add_argument("--pretrained_weights", type=str)
    # extension (not in the reference CLI): train CAViT / CACNN too — what `train.py:178-186` lists in its optimiser but
    # its no_grad block keeps from training
    p.add_argument("--train_adapters", action="store_true")
    p.add_argument("--train_encoder", action="store_true", help="with --train_adapters: also the CNN encoder")
    p.add_argument("--shard_val", action="store_true",
                   help="validation sharded over the ranks (every world-th batch per rank, metric sums all-reduced) instead of the "
                        "reference's whole val set on every rank (train.py:125-130,236-238); same batches, same per-batch results")
    # extension: the optimizer (default: the reference's SGD).  adamw = optim.AdamW, the fused HIP AdamW with global-norm clipping
    p.add_argument("--optimizer", default="sgd", choices=("sgd", "adamw"))
    p.add_argument("--weight_decay", default=None, type=float,
                   help="default: the script's own value (train.py 3e-5, train_mla.py / train_multi_class.py 0)")
    p.add_argument("--adam_beta1", default=0.9, type=float)
    p.add_argument("--adam_beta2", default=0.999, type=float)
    p.add_argument("--adam_eps", default=1e-8, type=float)
    p.add_argument("--clip_grad", default=None, type=float, help="adamw: clip the global gradient norm at this value")
    p.add_argument("--layer_decay", default=None, type=float,
                   help="adamw: layer-wise learning-rate decay of the ViT blocks (needs --train_backbone --optimize_backbone)")
    # extension: fine-tune the ViT itself (BASELINE config 4: SegEngine train_backbone / optimize_backbone) with stochastic depth
    p.add_argument("--train_backbone", action="store_true",
                   help="with --train_adapters: both ViT passes run with saved activations and the backward reaches every block")
    p.add_argument("--optimize_backbone", action="store_true",
                   help="with --train_backbone: the optimizer also steps the ViT; the checkpoint gains a 'backbone' entry")
    p.add_argument("--lora_rank", default=None, type=int, choices=(4, 8, 16, 32), metavar="R",
                   help="with --train_adapters --train_backbone: low-rank adaptation of the q and v projections of every ViT block "
                        "instead of full backbone gradients (4 | 8 | 16 | 32); the checkpoint gains a 'lora' entry")
    p.add_argument("--lora_alpha", default=None, type=float, help="LoRA scale numerator: the update is (alpha / rank) B A (default: the rank)")
    p.add_argument("--drop_path", default=0.0, type=float, metavar="R",
                   help="stochastic depth rate of the ViT (DINOv2's drop_path_rate; needs --train_backbone): block i gets "
                        "linspace(0, R, depth)[i]; above 0.1 a branch runs on a random subset of the batch only")
    p.add_argument("--drop_path_uniform", action="store_true", help="every block gets --drop_path")
    p.add_argument("--drop_path_seed", default=0, type=int, help="seed of the stochastic-depth draws (the generator is seeded with this and the rank)")
    # extension: an exponential moving average of the trained weights (optim.EMA), used for validation and kept in the checkpoint
    p.add_argument("--ema_decay", default=None, type=float, metavar="D",
                   help="keep an exponential moving average of every trained weight with this decay (in (0, 1)); validation, "
                        "--evaluate and best_acc then use the averaged weights and the checkpoint gains an 'ema' entry")
    p.add_argument("--ema_no_warmup", action="store_true",
                   help="with --ema_decay: use D from the first update on instead of min(D, (1 + t) / (10 + t))")
    p.add_argument("--ema_validate_live", action="store_true",
                   help="with --ema_decay: also validate the live weights and log their metrics as test_live_*")
    # extension: mean-teacher training (SegEngine teacher=): a consistency loss against the averaged weights or a frozen checkpoint
    p.add_argument("--distill_teacher", default=None, type=str, metavar="ema|PATH",
                   help="add a gated consistency term (ops.consistency_loss) against a teacher: 'ema' = this run's averaged weights "
                        "(needs --ema_decay), or the checkpoint of an earlier run (a frozen teacher)")
    p.add_argument("--distill_teacher_arch", default=None, type=str, help="architecture of a checkpoint teacher (default: --arch)")
    p.add_argument("--distill_teacher_ema", action="store_true", help="checkpoint teacher: load its 'ema' entry, as predict --ema does")
    p.add_argument("--distill_weight", default=None, type=float, help="weight of the consistency term (default 1)")
    p.add_argument("--distill_temperature", default=None, type=float, help="temperature of both distributions (default 1)")
    p.add_argument("--distill_threshold", default=None, type=float,
                   help="keep a pixel where the teacher's largest class probability (at the temperature) reaches this (default: all)")
    p.add_argument("--distill_class_thresholds", default=None, type=float, nargs="+", metavar="T",
                   help="one confidence threshold per class in place of --distill_threshold (--num_classes values)")
    p.add_argument("--distill_adaptive_threshold", action="store_true",
                   help="self-adaptive thresholds (FreeMatch): a global threshold that follows the teacher's mean confidence, scaled "
                        "per class by a moving average of the teacher's class distribution, kept on the device")
    p.add_argument("--distill_adaptive_momentum", default=None, type=float, metavar="L",
                   help="momentum of both moving averages of --distill_adaptive_threshold (default 0.999)")
    p.add_argument("--distill_rampup", default=None, type=int, metavar="STEPS",
                   help="ramp the weight up over this many steps by exp(-5 (1 - t / STEPS)^2) (default 0: none)")
    p.add_argument("--distill_flip", action="store_true", help="the teacher also sees the mirrored batch (two views averaged)")
    p.add_argument("--distill_weak", action="store_true",
                   help="the teacher sees the batch under the student's geometry without CLAHE / brightness-contrast / gamma "
                        "(uint8 datasets; other batches have no photometric stage)")
    # extension: batch mixing (SegEngine mix=): CutMix / ClassMix on the device, with or without a teacher
    p.add_argument("--mix", default=None, choices=["cutmix", "classmix"],
                   help="paste pixels of another sample of the rank's batch into each sample (ops.mix_batch): cutmix = a box, "
                        "classmix = half of the donor's classes; a teacher's targets are mixed the same way")
    p.add_argument("--mix_p", default=None, type=float, help="probability that a sample is mixed (default 1)")
    p.add_argument("--mix_seed", default=None, type=int, help="seed of the draws, which depend on (seed, rank, step) alone (default 0)")
    p.add_argument("--mix_background", action="store_true", help="classmix: class 0 may be pasted too")
    # extension: semi-supervised training (SegEngine ignore_index=, train_step labelled=): unlabelled frames in every batch
    p.add_argument("--unlabelled_path", default=None, type=str, metavar="DIR|synthetic",
                   help="a stream of frames without labels (every *.png / *.jpg below DIR): each step's batch is the labelled "
                        "batch followed by --unlabelled_per_batch of them, which train through the consistency term alone "
                        "(needs --distill_teacher)")
    p.add_argument("--unlabelled_per_batch", default=None, type=int, metavar="U", help="unlabelled frames a step (default: --batch_size_per_gpu)")
    p.add_argument("--ignore_index", default=None, type=int, metavar="G",
                   help="label value that takes no part in the training loss (outside the classes; the fused losses only; "
                        "validation takes its sets as fully labelled)")
    p.add_argument("--distill_labelled_weight", default=None, type=float, metavar="W",
                   help="weight of the consistency term on labelled samples (default 1; unlabelled samples have 1; 0: a labelled "
                        "sample reads none of its teacher maps)")
    # extension: the training loss (default: what each script applies, train.py:427-428 Dice, train_multi_class.py:390-393 soft IoU)
    p.add_argument("--loss", default="dice", choices=sorted(SegEngine.LOSSES),
                   help="training loss; lovasz = segloss/lovasz_loss.py LovaszSoftmax on softmax(out), ce_lovasz = CrossentropyND + that; "
                        "topk = TopKLoss (the worst --topk_percent %% of the batch's pixels), dc_and_topk = SoftDice + that, "
                        "focal = segloss/focal_loss.py FocalLoss on softmax(out)")
    p.add_argument("--topk_percent", default=10.0, type=float, help="--loss topk / dc_and_topk: the k of TopKLoss, in percent")
    p.add_argument("--focal_gamma", default=2.0, type=float, help="--loss focal: the gamma of FocalLoss")
    # extension: the switch the reference comments out (`train.py:158-159`, `#p=0.8 if self.use_vis_aug_non_rigid else 0`)
    p.add_argument("--aug_non_rigid", default=0.0, type=float,
                   help="probability of the non-rigid block OneOf([ElasticTransform, GridDistortion, OpticalDistortion]) of the "
                        "GPU augmentation (uint8 datasets, training batches only); 0 = the reference as it stands")
    # extension: the strong student view of FixMatch / UniMatch-style training (ops.strong_view), after the augmentation
    p.add_argument("--aug_strong", action="store_true",
                   help="the student trains on a strong view: colour jitter (p 0.8), greyscale (p 0.2), Gaussian blur (p 0.5) on the "
                        "device after the augmentation (uint8 datasets, training batches only); a teacher never sees it")
    p.add_argument("--aug_strong_jitter", default=None, type=float, nargs=4, metavar=("B", "C", "S", "H"),
                   help="amplitudes of brightness, contrast, saturation (factors in 1 +- a; each in [0, 1]) and hue (shift in +- H; "
                        "in [0, 0.5]); default 0.5 0.5 0.5 0.25")
    p.add_argument("--aug_strong_grey", default=None, type=float, metavar="P", help="probability of greyscale (default 0.2)")
    p.add_argument("--aug_strong_blur", default=None, type=float, metavar="P", help="probability of the Gaussian blur (default 0.5)")
    p.add_argument("--aug_strong_on", default="all", choices=("all", "unlabelled"),
                   help="the samples that get the strong view: all, or the unlabelled frames alone (needs --unlabelled_path)")
    return p


if __name__ == "__main__":
    train_seg(get_args_parser().parse_args())
