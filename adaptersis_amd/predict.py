"""Prediction: a checkpoint and a folder of frames -> label images at each frame's native size.

    python -m adaptersis_amd.predict --arch vit_large --imsize 588 --head mla --num_classes 8 --output_dir /tmp/out \
        --input /data/endovis2017 --dataset endovis2017 --split Test --encode endovis2017 --pred_dir /tmp/pred --overlay --masks
    python -m adaptersis_amd.predict --arch vit_large --imsize 588 --checkpoint run/checkpoint.pth.tar --input frames/ \
        --pred_dir pred/ --encode binary255

What the reference's authors did by hand in commented-out blocks (`train.py:624-640`, `train_multi_class.py:563-579`: argmax,
times 255, ``draw_segmentation_masks(alpha=.5, colors="green")``, ``imsave``), as a tool: frames are read at native size, uploaded
as uint8, resized on the device (``ops.frame_resize``, PIL-exact) and normalised by the validation path of
``train._to_device_batch``; ``SegEngine.predict`` makes the masks at native size in one fused pass (``ops.predict_mask``:
bilinear resize of the logits, argmax, pixel value; optionally the overlay and the per-class pixel counts against the ground
truth); with ``--surface`` the boundary statistics of every frame are made from that mask and the ground truth where they already
are, on the device (``ops.surface_stats``: exact distance transform; Dice, normalised surface distance, Hausdorff and mean
surface distance per class under ``"surface"`` in ``metrics.json``, ``segloss/surface.py``; with ``--hd_percentile`` also the
percentile Hausdorff distance, HD95 by default, its order statistics selected on the device); PNGs are written by a small thread pool under ``--pred_dir`` with the input's relative path and stem.

Batches: frames are grouped by native size, sizes in ascending order, paths sorted inside a size, ``--batch_size_per_gpu``
frames per batch (the last batch of a size may be short).  The composition is a function of the file list and the batch size
only, and it matters: the encoder's BatchNorm normalises with batch statistics in validation as in training (the reference never
puts it in eval mode), so a frame's mask depends on the batch it is predicted in, exactly as the validation metrics do.

The checkpoint is the file ``train_seg`` writes: the decoder under ``state_dict`` and, when they were trained, ``cross_vit`` /
``cross_cnn`` / ``backbone_encoder``.  In the reference's flow the adapters and the encoder keep the random initial weights of
the training process, and neither the reference nor ``train_seg`` saves them or seeds the generator: such a checkpoint from a
separate ``python -m adaptersis_amd.train`` process cannot be predicted from, and is refused.  What can be predicted from:
checkpoints of ``--train_adapters --train_encoder`` runs (all three modules saved), and runs whose caller seeded torch before
``train_seg`` and passes that ``--seed`` here (modules are built in the same order, ``train.build_modules``; a warning names
what is drawn).

Test-time augmentation (``--tta_flip``, ``--tta_sizes S [S ...]``): every frame is predicted at each size of ``--tta_sizes``
(default: ``--imsize`` alone) and, with ``--tta_flip``, also mirrored at each; ``plan_views`` fixes the order.  The class
probabilities of the views are averaged at native size and the mask is taken from the average, in one fused pass
(``SegEngine.predict_views``, ``ops.predict_mask_views``); ``--confidence`` also writes ``<stem>_conf.png`` (mode ``L``: 255 times
the mean probability of the chosen class, rounded).  Each view is its own forward pass: the encoder's BatchNorm normalises each
view with that view's batch statistics, so the views of a frame differ by more than the resize and the mirror, and a frame's mask
still depends on the batch it is predicted in.  Without any of the three flags the tool calls ``SegEngine.predict`` and writes
exactly the files it wrote before they existed; ``metrics.json`` holds ``"views": [[size, flip], ...]`` only when views were used.

Sliding-window prediction (``--slide_size L`` [``--slide_stride T``] [``--slide_blend ramp|uniform``] [``--slide_context``]): the
frame is resized to L x L (``ops.frame_resize``), the network runs at its own input size S = ``--imsize`` on the S x S windows of
that working frame whose origins ``plan_tiles`` lists (stride T, default 2 S // 3; the last window of a row or column is pulled
back to end at L), and the class probabilities of the windows are blended at native size in one fused pass
(``SegEngine.predict_tiles``, ``ops.predict_mask_tiles``): each window is sampled once, at the native pixel's place in it, and
weighs 1 (``uniform``) or ramps down over S - T working pixels towards its inner edges (``ramp``, the default).
``--slide_context`` adds the whole frame at S x S (the very input of the plain path) as one more tile, ``--tta_flip`` follows every
tile with its mirrored twin, ``--confidence`` works as above; ``--tta_sizes`` cannot be combined with it.  Every tile is its own
forward pass with its own BatchNorm batch statistics, as every view is.  ``metrics.json`` holds ``"tiles": {"size", "stride",
"blend", "context", "flip", "count"}`` only in this mode.

Single process, single GPU: prediction is not sharded over ranks.
"""
from __future__ import annotations

import concurrent.futures as cf
import json
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import train as _t
from .backbones.engines import SegEngine
from .lora import LoRA
from .tools import frame_resize as _fr

IMAGE_EXT = (".png", ".jpg", ".bmp")
DATASETS = ("endovis2017", "endovis2018", "autolapro", "robomis")
MAX_WRITERS = 8
DEFAULT_TOLERANCES = (1.0, 2.0, 5.0)
MAX_VIEWS = 8
MAX_TILES = 32
BLENDS = ("ramp", "uniform")


def get_args_parser():
    p = _t.get_args_parser()
    p.description = ("Native-size masks from a checkpoint (single process, single GPU; prediction is not sharded over ranks: run "
                     "one process per GPU on disjoint --input folders instead)")
    p.add_argument("--head", default="feature", choices=("feature", "mla"), help="decode head the checkpoint was trained with")
    p.add_argument("--num_classes", default=2, type=int)
    p.add_argument("--checkpoint", default=None, type=str, help="default: <output_dir>/checkpoint.pth.tar (what train_seg writes)")
    p.add_argument("--input", required=True, type=str,
                   help="directory walked recursively for .png / .jpg / .bmp frames, or the dataset root with --dataset")
    p.add_argument("--dataset", default=None, choices=DATASETS, help="read --input as this dataset's layout (with --split)")
    p.add_argument("--split", default=None, type=str, help="split of --dataset (default: its validation split)")
    p.add_argument("--task", default=None, choices=("multi", "binary"),
                   help="endovis2017 ground truth: instruments_masks (multi, the default) or binary_masks")
    p.add_argument("--pred_dir", default="pred", type=str)
    p.add_argument("--encode", default="index", choices=sorted(_fr.ENCODINGS),
                   help="pixel value per class: index = c, binary255 = 0 / 255, endovis2017 = 32 c (instruments_masks)")
    p.add_argument("--overlay", action="store_true", help="also write <stem>_overlay.png: the mask drawn over the frame")
    p.add_argument("--alpha", default=0.5, type=float, help="overlay opacity of every class but 0 (reference: .5, green)")
    p.add_argument("--masks", nargs="?", const="dataset", default=None,
                   help="score against native ground truth: with --dataset the dataset's own masks (no value needed), otherwise a "
                        "directory mirroring --input; writes per-class IoU, mean IoU and pixel accuracy to <pred_dir>/metrics.json")
    p.add_argument("--surface", nargs="*", type=float, default=None, metavar="TAU",
                   help="with --masks: per-frame Dice and boundary metrics (normalised surface distance at these tolerances, in "
                        "pixels at native size; Hausdorff; mean surface distance) under 'surface' in metrics.json; no value = "
                        + " ".join(f"{t:g}" for t in DEFAULT_TOLERANCES))
    add_hd_percentile(p)
    p.add_argument("--tta_flip", action="store_true", help="test-time augmentation: also predict every frame mirrored, at every size")
    p.add_argument("--tta_sizes", nargs="+", type=int, default=None, metavar="S",
                   help="test-time augmentation: input sizes of the views (default: --imsize alone); each as --imsize is given to train")
    p.add_argument("--confidence", action="store_true",
                   help="also write <stem>_conf.png (mode L): 255 x the mean probability of the chosen class over the views")
    p.add_argument("--slide_size", default=None, type=int, metavar="L",
                   help="sliding-window prediction: resize every frame to L x L and predict --imsize windows of it, blended at native "
                        "size (L >= --imsize)")
    p.add_argument("--slide_stride", default=None, type=int, metavar="T",
                   help="with --slide_size: distance of the window origins in pixels of the L x L frame (default 2 * imsize // 3)")
    p.add_argument("--slide_blend", default=None, choices=BLENDS,
                   help="with --slide_size: weight of a window at a pixel: ramp (default; falls off over imsize - T pixels towards the "
                        "window's inner edges) or uniform")
    p.add_argument("--slide_context", action="store_true",
                   help="with --slide_size: one more tile, the whole frame at --imsize (the input of the plain prediction)")
    p.add_argument("--ema", action="store_true",
                   help="predict with the averaged weights: the checkpoint's 'ema' entry (a run with --ema_decay) instead of the live "
                        "modules; a checkpoint without that entry is an error")
    p.add_argument("--seed", default=None, type=int,
                   help="torch seed the TRAINING process was given before it built its modules; required when the checkpoint lacks "
                        "cross_vit / cross_cnn / backbone_encoder (the training command lines do not seed, so only a caller that "
                        "seeded train_seg itself has one)")
    return p


# ---- views ------------------------------------------------------------------------------------------------------------------
def plan_views(imsize: int, sizes: Optional[Sequence[int]], flip: bool) -> List[Tuple[int, bool]]:
    """The views of test-time augmentation as (input size, mirrored): ``sizes`` (None = ``imsize`` alone) ascending with duplicates
    removed, at each size the plain view before the mirrored one.  A non-positive size or more than ``MAX_VIEWS`` views raise."""
    chosen = [imsize] if sizes is None else list(sizes)
    for s in chosen:
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or s < 1:
            raise ValueError(f"--tta_sizes / --imsize: {s!r} is not a positive input size")
    if not chosen:
        raise ValueError("--tta_sizes: no size given")
    views = [(int(s), f) for s in sorted(set(int(s) for s in chosen)) for f in ((False, True) if flip else (False,))]
    if len(views) > MAX_VIEWS:
        raise ValueError(f"--tta_sizes / --tta_flip: {len(views)} views, at most {MAX_VIEWS} are supported")
    return views


def views_of(args) -> Optional[List[Tuple[int, bool]]]:
    """None when no ``--tta_*`` flag and no ``--confidence`` is given (the tool then runs ``SegEngine.predict`` as before), else
    ``plan_views`` of the arguments."""
    flip, sizes = getattr(args, "tta_flip", False), getattr(args, "tta_sizes", None)
    if not flip and sizes is None and not getattr(args, "confidence", False):
        return None
    return plan_views(args.imsize, sizes, flip)


# ---- tiles ------------------------------------------------------------------------------------------------------------------
def _is_int(v) -> bool:
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def slide_origins(L: int, S: int, stride: int) -> List[int]:
    """Window origins along one axis: n = max(L - S + stride - 1, 0) // stride + 1 windows at min(i * stride, L - S)."""
    return [min(i * stride, L - S) for i in range(max(L - S + stride - 1, 0) // stride + 1)]


def plan_tiles(L: int, S: int, stride: int, context: bool, flip: bool) -> List[Tuple[int, int, int, int, bool]]:
    """The tiles of sliding-window prediction as (oy, ox, sy, sx, mirrored) on the L x L working frame: the S x S windows at
    ``slide_origins`` in row-major order, then with ``context`` the whole frame (0, 0, L, L); with ``flip`` every tile is followed
    by its mirrored twin.  ``S`` < 1, ``L`` < ``S``, a ``stride`` outside 1..S or more than ``MAX_TILES`` tiles raise."""
    for name, v in (("--imsize", S), ("--slide_size", L), ("--slide_stride", stride)):
        if not _is_int(v):
            raise ValueError(f"{name}: {v!r} is not an integer")
    L, S, stride = int(L), int(S), int(stride)
    if S < 1:
        raise ValueError(f"--imsize: {S} is not a positive input size")
    if L < S:
        raise ValueError(f"--slide_size: {L} is smaller than the network input size --imsize {S}")
    if not 1 <= stride <= S:
        raise ValueError(f"--slide_stride: {stride} must be in 1..{S} (--imsize): a larger stride leaves pixels between the windows")
    org = slide_origins(L, S, stride)
    count = (len(org) ** 2 + bool(context)) * (2 if flip else 1)
    if count > MAX_TILES:
        raise ValueError(f"--slide_size / --slide_stride / --slide_context / --tta_flip: {count} tiles, at most {MAX_TILES} are "
                         "supported")
    rects = [(oy, ox, S, S) for oy in org for ox in org] + ([(0, 0, L, L)] if context else [])
    return [r + (f,) for r in rects for f in ((False, True) if flip else (False,))]


def tiles_of(args) -> Optional[dict]:
    """None without ``--slide_size``, else the checked plan: {"size", "stride", "blend", "context", "flip", "ramp", "tiles"}.
    ``--tta_sizes`` with ``--slide_size``, and the other ``--slide_*`` flags without it, raise."""
    L = getattr(args, "slide_size", None)
    stride, blend, context = (getattr(args, n, None) for n in ("slide_stride", "slide_blend", "slide_context"))
    if L is None:
        for name, given in (("--slide_stride", stride is not None), ("--slide_blend", blend is not None),
                            ("--slide_context", bool(context))):
            if given:
                raise ValueError(f"{name} needs --slide_size")
        return None
    if getattr(args, "tta_sizes", None) is not None:
        raise ValueError("--tta_sizes cannot be combined with --slide_size: the windows are predicted at --imsize")
    S = args.imsize
    stride = 2 * S // 3 if stride is None else stride
    flip = bool(getattr(args, "tta_flip", False))
    tiles = plan_tiles(L, S, stride, bool(context), flip)
    return {"size": int(L), "stride": int(stride), "blend": blend or BLENDS[0], "context": bool(context), "flip": flip,
            "ramp": max(int(S) - int(stride), 1), "tiles": tiles}


# ---- file list and batches ---------------------------------------------------------------------------------------------------
def walk_frames(root: str) -> List[str]:
    """Sorted relative paths of the frames under ``root``."""
    out = []
    for d, _, files in os.walk(root):
        out += [os.path.relpath(os.path.join(d, f), root) for f in files if os.path.splitext(f)[1].lower() in IMAGE_EXT]
    return sorted(out)


def plan_batches(sizes: Sequence[Tuple[int, int]], batch_size: int) -> List[List[int]]:
    """``sizes[i]`` = native (H, W) of the i-th file of the sorted list -> batches of indices: one size per batch, sizes ascending,
    list order inside a size, ``batch_size`` per batch (the last of a size may be short)."""
    if batch_size < 1:
        raise ValueError(f"batch size must be positive, got {batch_size}")
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, s in enumerate(sizes):
        groups.setdefault((int(s[0]), int(s[1])), []).append(i)
    return [g[k:k + batch_size] for _, g in sorted(groups.items()) for k in range(0, len(g), batch_size)]


def _native_size(path: str) -> Tuple[int, int]:
    from PIL import Image
    with Image.open(path) as im:     # header only
        return im.size[1], im.size[0]


class _Frames:
    """The frames to predict: relative paths (outputs mirror them), loaders of the native frame and of its raw mask."""

    def __init__(self, args):
        self.lut = _fr.ENCODINGS[args.encode][1]
        self.ds = None
        if args.dataset is not None:
            from . import train_multi_class as tmc
            from .tools import dataset as D
            split = args.split or tmc.SPLITS[args.dataset][1]
            if args.dataset == "robomis":
                imgs = sorted(os.path.join("images", split, f) for f in os.listdir(os.path.join(args.input, "images", split))
                              if os.path.splitext(f)[1].lower() in IMAGE_EXT)
                self.root, self.rel = args.input, imgs
                self.mask_files = [os.path.join(args.input, "annotations", split, os.path.basename(r)) for r in imgs]
                self.lut = _fr.LUT_BINARY
            elif args.masks is None:
                # frames only: every <sequence>/images/* under the split, no ground truth needed (a test split may ship without)
                self.root = os.path.join(args.input, split)
                self.rel = [r for r in walk_frames(self.root) if os.path.basename(os.path.dirname(r)) == "images"]
                self.mask_files = None
            else:
                kw = dict(transform=None, imsize=args.imsize, resize_on_gpu=True)
                if args.dataset == "endovis2017":
                    kw["task"] = args.task or "multi"
                cls = {"endovis2017": D.EndoVis2017, "endovis2018": D.EndoVis2018, "autolapro": D.Autolapro}[args.dataset]
                self.ds = cls(args.input, split, **kw)
                self.root = os.path.join(args.input, split)
                order = sorted(range(len(self.ds)), key=lambda i: self.ds.img_files[i])
                self.ds_index = order
                self.rel = [os.path.relpath(self.ds.img_files[i], self.root) for i in order]
                self.mask_files = [self.ds.mask_files[i] for i in order]
                self.lut = self.ds.lut
            if args.masks not in (None, "dataset"):
                raise ValueError("--masks takes no directory with --dataset: the dataset's own masks are used")
        else:
            if not os.path.isdir(args.input):
                raise FileNotFoundError(f"--input {args.input}: not a directory")
            self.root, self.rel = args.input, walk_frames(args.input)
            self.mask_files = None
            if args.masks == "dataset":
                raise ValueError("--masks without a directory needs --dataset")
            if args.masks is not None:
                self.mask_files = [self._mirror(args.masks, r) for r in self.rel]
        if not self.rel:
            raise ValueError(f"no frames ({', '.join(IMAGE_EXT)}) under {args.input}")
        self.with_masks = args.masks is not None
        self.sizes = [_native_size(os.path.join(self.root, r)) for r in self.rel]

    @staticmethod
    def _mirror(mask_root, rel):
        stem = os.path.splitext(rel)[0]
        for e in IMAGE_EXT:
            if os.path.isfile(os.path.join(mask_root, stem + e)):
                return os.path.join(mask_root, stem + e)
        raise FileNotFoundError(f"--masks {mask_root}: no mask for frame {rel}")

    def load(self, i: int):
        """-> (uint8 [H,W,3], uint8 [H,W] raw mask or None)."""
        from PIL import Image
        if self.ds is not None and self.with_masks:    # the dataset's own pairing, mask reading and size check
            img, mask, _ = self.ds[self.ds_index[i]]
            return img.numpy(), mask.numpy()
        with open(os.path.join(self.root, self.rel[i]), "rb") as f:
            img = np.array(Image.open(f).convert("RGB"), dtype=np.uint8)
        mask = None
        if self.with_masks:
            with open(self.mask_files[i], "rb") as f:
                mask = np.array(Image.open(f).convert("L"), dtype=np.uint8)
            if mask.shape != img.shape[:2]:
                raise ValueError(f"{self.mask_files[i]}: mask {mask.shape} and frame {img.shape[:2]} differ in size")
        return img, mask

    def load_batch(self, idx: Sequence[int]):
        """-> (uint8 [B,H,W,3], uint8 [B,H,W] or None) on the host."""
        items = [self.load(i) for i in idx]
        frames = torch.from_numpy(np.stack([it[0] for it in items]))
        masks = torch.from_numpy(np.stack([it[1] for it in items])) if self.with_masks else None
        return frames, masks


# ---- model -------------------------------------------------------------------------------------------------------------------
def check_state_dict(ckpt_sd: dict, expected: Dict[str, tuple], path: str, entry: str, hint: str = "") -> dict:
    """The checkpoint entry with DDP's ``module.`` prefix stripped, after checking it against ``expected`` (name -> shape): the
    first key that is unknown to the module, has another shape, or is missing raises with the file and the key named."""
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in ckpt_sd.items()}
    for k, v in sd.items():
        if k not in expected:
            raise ValueError(f"{path}: '{entry}' key '{k}' does not exist in the model built from the arguments{hint}")
        if tuple(v.shape) != tuple(expected[k]):
            raise ValueError(f"{path}: '{entry}' key '{k}' has shape {list(v.shape)}, the model built from the arguments expects "
                             f"{list(expected[k])}{hint}")
    for k in expected:
        if k not in sd:
            raise ValueError(f"{path}: '{entry}' lacks key '{k}' of the model built from the arguments{hint}")
    return sd


def _expected(module) -> Dict[str, tuple]:
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


FROZEN_MODULES = ("backbone_encoder", "cross_vit", "cross_cnn")


def modules_not_in_checkpoint(ck: dict, seed: Optional[int], path: str) -> List[str]:
    """The modules among ``FROZEN_MODULES`` that the checkpoint does not hold.  ``train_seg`` saves them only when they train
    (``--train_adapters`` / ``--train_encoder``); in the reference's flow they keep the random initial values of the training
    process, which no file records.  They can then only be redrawn from a seed the caller vouches for: without ``--seed`` this
    raises, with it the caller is told what is drawn."""
    missing = [n for n in FROZEN_MODULES if n not in ck]
    if missing and seed is None:
        raise ValueError(
            f"{path} holds no {', '.join(repr(n) for n in missing)}: the decoder was trained against the random initial weights of "
            "these modules, which the training process drew and did not save.  Predicting needs exactly those weights.  Either "
            "train with --train_adapters --train_encoder (the checkpoint then holds all three), or, if the training process "
            "called torch.manual_seed(S) before train_seg (the training command lines do not seed), pass --seed S.")
    if missing:
        print(f"WARNING: {path} holds no {', '.join(missing)}; drawing their weights from torch.manual_seed({seed}).  The masks are "
              f"those of the trained model only if the training process was seeded with {seed} before it built its modules.")
    return missing


def read_checkpoint(path: str) -> dict:
    if not os.path.isfile(path):
        raise FileNotFoundError(f"checkpoint {path} does not exist (a prediction from random weights is never made)")
    ck = torch.load(path, map_location="cpu")
    if "state_dict" not in ck:
        raise ValueError(f"{path}: no 'state_dict' entry (expected the file train_seg writes)")
    return ck


def load_checkpoint(path: str, seg_decoder, extra: Dict[str, torch.nn.Module], hint: str = "", ck: Optional[dict] = None) -> dict:
    ck = read_checkpoint(path) if ck is None else ck
    seg_decoder.load_state_dict(check_state_dict(ck["state_dict"], _expected(seg_decoder), path, "state_dict", hint))
    for name, mod in extra.items():
        if name in ck:
            mod.load_state_dict(check_state_dict(ck[name], _expected(mod), path, name))
    return ck


def build_engine(args) -> SegEngine:
    """Modules as ``train_seg`` builds them (``train.build_modules``), the checkpoint loaded into them, one ``SegEngine``."""
    if not torch.cuda.is_available():
        raise RuntimeError("adaptersis_amd.predict needs an MI355X (there is no CPU path)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    path = args.checkpoint or os.path.join(args.output_dir, "checkpoint.pth.tar")
    ck = read_checkpoint(path)
    modules_not_in_checkpoint(ck, args.seed, path)       # before anything is drawn from the generator
    if args.seed is not None:
        torch.manual_seed(args.seed)
    model, enc, cv, cn, dec = _t.build_modules(args, args.head, args.num_classes, dev)
    eng = SegEngine(model, enc, cv, cn, dec, num_classes=args.num_classes)
    # "backbone": the ViT of a run with --optimize_backbone (absent from any other checkpoint: the pretrained weights stay)
    src = ck
    if getattr(args, "ema", False):     # the averaged weights: the same loader, pointed at the entry shaped like the checkpoint
        src = ck.get("ema")
        if not isinstance(src, dict) or "state_dict" not in src:
            raise ValueError(f"{path} holds no 'ema' entry: --ema needs a checkpoint of a run with --ema_decay (the live weights "
                             "are not used in its place)")
    load_checkpoint(path, dec, {"cross_vit": cv, "cross_cnn": cn, "backbone_encoder": enc, "backbone": model},
                    hint=f" (--head {args.head} --num_classes {args.num_classes})", ck=src)
    if "lora" in src:    # a run with --lora_rank: every forward of the engine goes through the merged weights (SegEngine.eval_logits)
        eng.lora = LoRA.from_state(model, src["lora"])
    print(f"loaded {path} (epoch {ck.get('epoch')}, entries {sorted(k for k in ck if isinstance(ck[k], dict))}"
          + (f"; averaged weights after {src.get('updates')} updates" if src is not ck else "") + ")")
    return eng


# ---- the run -----------------------------------------------------------------------------------------------------------------
def _network_input(frames: torch.Tensor, size: int, flip: bool = False) -> torch.Tensor:
    """Native uint8 frames on the device -> the float batch validation feeds the network at ``size`` (mirrored when ``flip``)."""
    from . import ops
    small, _ = ops.frame_resize(frames, None, size)
    return _normalised(small, flip)


def _normalised(small: torch.Tensor, flip: bool = False) -> torch.Tensor:
    """uint8 [B,S,S,3] on the device -> validation's float batch (mirrored when ``flip``)."""
    if flip:
        small = small.flip(2)
    small = small.contiguous()
    inp, _ = _t._to_device_batch(small, torch.zeros(small.shape[:3], dtype=torch.uint8, device=small.device), train=False)
    return inp


def tile_inputs(frames: torch.Tensor, S: int, plan: dict) -> List[torch.Tensor]:
    """Native uint8 frames on the device -> the network input of every tile of ``plan`` (``tiles_of``): S x S windows of the frame
    resized to the working size, and for the context tile the frame resized to S x S (the input of the plain path)."""
    from . import ops
    L = plan["size"]
    work, _ = ops.frame_resize(frames, None, L)
    whole = None
    out = []
    for oy, ox, sy, sx, flip in plan["tiles"]:
        if (sy, sx) == (S, S):
            out.append(_normalised(work[:, oy:oy + S, ox:ox + S], flip))
        else:
            if whole is None:
                whole, _ = ops.frame_resize(frames, None, S)
            out.append(_normalised(whole, flip))
    return out


def predict_batch(engine: SegEngine, frames_u8: torch.Tensor, masks_u8: Optional[torch.Tensor], args, lut, views=None, tiles=None):
    """Native uint8 [B,H,W,3] (host) -> device outputs of ``SegEngine.predict``: mask[, overlay][, counts]; with ``views``
    (``plan_views``) those of ``SegEngine.predict_views``, with ``tiles`` (``tiles_of``) those of ``SegEngine.predict_tiles``:
    mask[, confidence][, overlay][, counts]."""
    C = args.num_classes
    frames = frames_u8.cuda(non_blocking=True).contiguous()
    B, H, W, _ = frames.shape
    if views is None and tiles is None:
        inp = _network_input(frames, args.imsize)
    kw = dict(encode=_fr.encode_table(args.encode, C))
    if args.overlay:
        kw.update(frames=frames, alpha=_fr.default_alpha(C, args.alpha))
    if masks_u8 is not None:
        kw.update(target=masks_u8.cuda(non_blocking=True).contiguous(), lut=lut)
    if tiles is not None:
        out = engine.predict_tiles(tile_inputs(frames, args.imsize, tiles), tiles["tiles"], tiles["size"], (H, W),
                                   blend=tiles["blend"], ramp=tiles["ramp"], confidence=bool(args.confidence), **kw)
    elif views is None:
        out = engine.predict(inp, size=(H, W), **kw)
    else:
        out = engine.predict_views([_network_input(frames, s, f) for s, f in views], [f for _, f in views], (H, W),
                                   confidence=bool(args.confidence), **kw)
    return out if isinstance(out, tuple) else (out,)


def surface_tolerances(args) -> Optional[List[float]]:
    """The tolerances of ``--surface`` (None = not asked for; no value = ``DEFAULT_TOLERANCES``), checked: argument errors are
    raised here, before any file is read or any model is built."""
    if getattr(args, "surface", None) is None:
        return None
    if args.masks is None:
        raise ValueError("--surface needs --masks: boundary metrics are made against the ground truth")
    tol = [float(t) for t in args.surface] or list(DEFAULT_TOLERANCES)
    from . import ops
    ops.surface_thresholds(tol)
    return tol


def add_hd_percentile(p) -> None:
    p.add_argument("--hd_percentile", nargs="*", type=float, default=None, metavar="P",
                   help="with --surface: percentile Hausdorff distances (percents, multiples of 0.01, at most 4) per class under "
                        "'surface' in metrics.json: hd_pct over the pooled boundary distances, hd_pct_sym the larger of the two "
                        "directed percentiles; no value = 95")


def hd_percentiles(args) -> Optional[List[float]]:
    """The percents of ``--hd_percentile`` (None = not asked for; no value = 95), checked like ``surface_tolerances``."""
    if getattr(args, "hd_percentile", None) is None:
        return None
    if getattr(args, "surface", None) is None:
        raise ValueError("--hd_percentile needs --surface: the percentiles are taken over the boundary distances")
    pct = [float(v) for v in args.hd_percentile] or [95.0]
    from . import ops
    ops.surface_percentiles(pct)
    return pct


def surface_batch(meter, mask: torch.Tensor, target: torch.Tensor, args, lut) -> None:
    """Boundary statistics of one batch, on the device: ``mask`` as ``SegEngine.predict`` encoded it (read back through the label
    table that ``--encode`` inverts), ``target`` the raw ground truth with the dataset's table.  Only the statistics come to the
    host, into ``meter``."""
    from . import ops
    out = ops.surface_stats(mask, target, args.num_classes, meter.tol, pred_lut=_fr.ENCODINGS[args.encode][1], lut=lut,
                            percentiles=meter.pct)
    meter.update(*(t.cpu().numpy() for t in out))


def metrics_from_counts(counts: np.ndarray) -> dict:
    """int64 [C,3] = (pred == c and label == c, pred == c, label == c) -> per-class IoU (None where the class occurs in neither),
    their mean over the classes that occur, and pixel accuracy (labels outside 0..C-1 count as wrong)."""
    inter, pred, lab = (counts[:, k].astype(np.int64) for k in range(3))
    union = pred + lab - inter
    iou = [float(i) / float(u) if u > 0 else None for i, u in zip(inter, union)]
    seen = [v for v in iou if v is not None]
    total = int(pred.sum())
    return {"per_class_iou": iou, "mean_iou": float(np.mean(seen)) if seen else None,
            "pixel_accuracy": float(inter.sum()) / total if total else None, "pixels": total, "counts": counts.tolist()}


def surface_line(s: dict) -> str:
    nsd = " ".join(f"{t:g}px " + ("-" if v is None else f"{v:.4f}") for t, v in zip(s["tolerances"], s["mean_nsd"]))
    pct = ""
    if "percentiles" in s:      # the first percentile asked for
        pct = f"  HD{s['percentiles'][0]:g} {s['mean_hd_pct'][0]} (directed maximum {s['mean_hd_pct_sym'][0]})"
    return (f"* boundary (classes 1..): Dice {s['mean_dice']}  NSD [{nsd}]  Hausdorff {s['mean_hd']}{pct}  mean surface distance "
            f"{s['mean_assd']}  unmatched (frame, class) pairs {sum(p['unmatched'] for p in s['per_class'])}")


def _save_png(arr: np.ndarray, mode: str, path: str) -> float:
    from PIL import Image
    t = time.perf_counter()
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    im = Image.fromarray(arr)
    assert im.mode == mode, (im.mode, mode)
    im.save(path, format="PNG")
    return time.perf_counter() - t


def predict_seg(args, engine: Optional[SegEngine] = None) -> dict:
    """-> {"files": mask paths relative to --pred_dir, "metrics": dict or None, "seconds" (wall), "encode_seconds" (summed over
    the writer threads), "drain_seconds" (waiting for the writers after the last batch), "frames_per_second"}."""
    _fr.encode_table(args.encode, args.num_classes)          # argument errors before any model is built
    tolerances = surface_tolerances(args)
    percentiles = hd_percentiles(args)
    tiles = tiles_of(args)
    views = None if tiles is not None else views_of(args)
    with_conf = (views is not None or tiles is not None) and bool(args.confidence)
    meter = None
    if tolerances is not None:
        from .segloss.surface import SurfaceMeter
        meter = SurfaceMeter(args.num_classes, tolerances, percentiles)
    frames = _Frames(args)
    batches = plan_batches(frames.sizes, args.batch_size_per_gpu)
    engine = engine or build_engine(args)
    total = None
    written, jobs = [], []
    t0 = time.perf_counter()
    with cf.ThreadPoolExecutor(max_workers=MAX_WRITERS) as pool:
        for idx in batches:
            fr, mk = frames.load_batch(idx)
            if mk is not None and meter is not None:
                mk = mk.cuda(non_blocking=True).contiguous()     # predict_batch's upload, made here to keep the device copy
            out = list(predict_batch(engine, fr, mk, args, frames.lut, views, tiles))
            if meter is not None:
                surface_batch(meter, out[0], mk, args, frames.lut)
            mask = out.pop(0).cpu().numpy()
            conf = out.pop(0).cpu().numpy() if with_conf else None
            over = out.pop(0).cpu().numpy() if args.overlay else None
            if mk is not None:
                c = out.pop(0)
                total = c if total is None else total + c
            for k, i in enumerate(idx):
                stem = os.path.splitext(frames.rel[i])[0]
                written.append(stem + ".png")
                jobs.append(pool.submit(_save_png, mask[k], "L", os.path.join(args.pred_dir, stem + ".png")))
                if conf is not None:
                    jobs.append(pool.submit(_save_png, conf[k], "L", os.path.join(args.pred_dir, stem + "_conf.png")))
                if over is not None:
                    jobs.append(pool.submit(_save_png, over[k], "RGB", os.path.join(args.pred_dir, stem + "_overlay.png")))
        t_fed = time.perf_counter() - t0                       # read + device + download; the writers ran beside it
        enc_s = sum(j.result() for j in jobs)
    wall = time.perf_counter() - t0
    metrics = None
    if total is not None:
        metrics = metrics_from_counts(total.cpu().numpy())
        metrics["frames"] = len(frames.rel)
        if views is not None:
            metrics["views"] = [[s, f] for s, f in views]
        if tiles is not None:
            metrics["tiles"] = {**{k: tiles[k] for k in ("size", "stride", "blend", "context", "flip")}, "count": len(tiles["tiles"])}
        if meter is not None:
            metrics["surface"] = meter.result()
        os.makedirs(args.pred_dir, exist_ok=True)
        with open(os.path.join(args.pred_dir, "metrics.json"), "w") as f:
            json.dump(metrics, f, indent=1, sort_keys=True)
        iou = " ".join("-" if v is None else f"{v:.4f}" for v in metrics["per_class_iou"])
        print(f"* IoU per class [{iou}]  mean IoU {metrics['mean_iou']}  pixel accuracy {metrics['pixel_accuracy']}")
        if meter is not None:
            print(surface_line(metrics["surface"]))
    n = len(frames.rel)
    print(f"{n} frames in {len(batches)} batches -> {args.pred_dir}: {wall:.2f} s, {n / wall:.2f} frames/s; PNG encoding {enc_s:.2f} "
          f"worker-seconds on {MAX_WRITERS} threads ({100 * enc_s / MAX_WRITERS / wall:.0f} % of the wall time per thread), "
          f"{wall - t_fed:.2f} s of it waiting for the writers after the last batch")
    return {"files": written, "metrics": metrics, "seconds": wall, "encode_seconds": enc_s, "drain_seconds": wall - t_fed,
            "frames_per_second": n / wall}


def main(argv=None):
    return predict_seg(get_args_parser().parse_args(argv))


if __name__ == "__main__":
    main()
