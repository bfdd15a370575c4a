"""`tools/dataset.py:127-167` — ``Robomis``: ``<dir>/images/<split>/*.png`` + ``<dir>/annotations/<split>/<same name>``.

Host side exactly as the reference (PIL decode, RGB, mask ``> 0``, resize to ``imsize`` with BILINEAR / NEAREST); what
differs is where the augmentation runs: with ``transform=None`` the item is the raw uint8 pair (HWC image, HW mask) and the
batch goes through ``tools.augment.TrainAugment`` on the GPU (``collate_u8`` + ``TrainAugment.__call__``); a callable
``transform(image=..., mask=...)`` (albumentations protocol) is still honoured on the host and then the item is the
reference's (float CHW / 255, long mask, index).  ``.npy`` arrays (``images.npy`` uint8 [N,H,W,3] or float [N,3,H,W],
``masks.npy``) are accepted in place of PNG folders: decode-free.

``EndoVis2017`` / ``EndoVis2018`` / ``Autolapro`` (`:7-125,172-222`): sorted, checked image / mask pairs per sequence folder and a
256-entry label table per dataset.  With ``transform=None`` and ``resize_on_gpu=True`` (their default) the item is the native
frame and raw mask and ``collate_frames`` hands the batch to ``ops.frame_resize`` on the device (PIL-exact, ``tools.frame_resize``).
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from .frame_resize import LUT_BINARY, LUT_MULTI


class Robomis(torch.utils.data.Dataset):
    def __init__(self, dir_main, split, transform=None, imsize=None):
        super().__init__()
        self.transform, self.imsize = transform, imsize
        self.arrays = None
        npy = os.path.join(dir_main, split, "images.npy")
        if os.path.isfile(npy):
            self.arrays = (np.load(npy, mmap_mode="r"), np.load(os.path.join(dir_main, split, "masks.npy"), mmap_mode="r"))
            self.img_files = list(range(self.arrays[0].shape[0]))
            self.mask_files = self.img_files
        else:
            self.img_files = sorted(glob.glob(os.path.join(dir_main, "images", split, "*.png")))
            self.mask_files = [os.path.join(dir_main, "annotations", split, os.path.basename(p)) for p in self.img_files]

    def _load(self, index):
        if self.arrays is not None:
            img, mask = np.array(self.arrays[0][index]), np.array(self.arrays[1][index])   # copies out of the memory map
            if img.dtype != np.uint8:                       # float [3,H,W] in [0,1] -> uint8 HWC
                img = np.clip(np.rint(np.moveaxis(img, 0, -1) * 255.0), 0, 255).astype(np.uint8)
            mask = (mask > 0).astype(np.uint8)
            if self.imsize is not None and img.shape[:2] != (self.imsize, self.imsize):
                # same resize as the PNG path (`tools/dataset.py:147-149`): PIL BILINEAR for the image, NEAREST for the mask
                from PIL import Image
                img = np.array(Image.fromarray(img).resize((self.imsize, self.imsize), resample=Image.BILINEAR)).astype(np.uint8)
                mask = np.array(Image.fromarray(mask * 255).resize((self.imsize, self.imsize), resample=Image.NEAREST))
                mask = (mask > 0).astype(np.uint8)
            return img, mask
        from PIL import Image
        with open(self.img_files[index], "rb") as f:
            img = Image.open(f).convert("RGB")
        with open(self.mask_files[index], "rb") as f:
            mask = Image.open(f)
            mask = mask.point(lambda x: 1 if x > 0 else 0, mode="1")
        if self.imsize is not None:
            img = img.resize((self.imsize, self.imsize), resample=Image.BILINEAR)
            mask = mask.resize((self.imsize, self.imsize), resample=Image.NEAREST)
        return np.array(img).astype(np.uint8), np.array(mask).astype(np.uint8)

    def __getitem__(self, index):
        img_np, mask_np = self._load(index)
        if self.transform is not None:
            t = self.transform(image=img_np, mask=mask_np)
            return torch.from_numpy(t["image"].transpose(2, 0, 1).copy()) / 255.0, torch.from_numpy(t["mask"].copy()).long(), index
        return torch.from_numpy(img_np), torch.from_numpy(mask_np), index

    def __len__(self):
        return len(self.img_files)


def collate_u8(items):
    """DataLoader ``collate_fn`` for the GPU-augmented path: -> (uint8 [B,H,W,3], uint8 [B,H,W], int64 [B])."""
    return (torch.stack([i[0] for i in items]), torch.stack([i[1] for i in items]),
            torch.tensor([i[2] for i in items], dtype=torch.int64))


# ---- EndoVis2017 / EndoVis2018 / Autolapro (`tools/dataset.py:7-125,172-222`) -----------------------------------------------------
def _stem(p):
    return os.path.splitext(os.path.basename(p))[0]


def _pair_folder(img_dir, mask_dir):
    """Sorted (images, masks) of one sequence folder, paired by position; the reference pairs two unsorted globs."""
    imgs = sorted(glob.glob(os.path.join(img_dir, "*")))
    masks = sorted(glob.glob(os.path.join(mask_dir, "*")))
    if len(imgs) != len(masks):
        raise ValueError(f"{os.path.dirname(img_dir)}: {len(imgs)} images but {len(masks)} masks in {os.path.basename(mask_dir)}")
    for a, b in zip(imgs, masks):
        if _stem(a) != _stem(b):
            raise ValueError(f"{os.path.dirname(img_dir)}: image {os.path.basename(a)} paired with mask {os.path.basename(b)}")
    return imgs, masks


class FrameBatch:
    """Batch of ``collate_frames``: native-size frames of one size (resized on the device by ``ops.frame_resize``) plus the
    items of another size, already resized on the host by the PIL route.
      frames uint8 [n, H, W, 3], masks uint8 [n, H, W] (raw single-channel), pos int64 [n]: their places in the batch
      host_frames uint8 [m, S, S, 3], host_masks uint8 [m, S, S] (label table applied), host_pos int64 [m]
      size S, lut uint8 [256]: the label table of the dataset."""

    def __init__(self, frames, masks, pos, host_frames, host_masks, host_pos, size, lut):
        self.frames, self.masks, self.pos = frames, masks, pos
        self.host_frames, self.host_masks, self.host_pos = host_frames, host_masks, host_pos
        self.size, self.lut = size, lut

    @property
    def shape(self):
        return (int(self.pos.numel() + self.host_pos.numel()), self.size, self.size, 3)

    def _map(self, fn):
        t = [fn(x) for x in (self.frames, self.masks, self.pos, self.host_frames, self.host_masks, self.host_pos)]
        return FrameBatch(*t, self.size, fn(self.lut))

    def pin_memory(self):
        return self._map(lambda x: x.pin_memory())

    def to(self, device, non_blocking=False):
        return self._map(lambda x: x.to(device, non_blocking=non_blocking))


def collate_frames(items, size, lut):
    """DataLoader ``collate_fn`` of the device-resize route: -> (FrameBatch, uint8 raw masks of the native group, int64 [B]).
    The batch's size is its first frame's; a frame of any other size takes the host route (identical bytes, see
    ``tools.frame_resize``)."""
    from .frame_resize import host_resize_pil
    shp = tuple(items[0][0].shape[:2])
    nat = [k for k, it in enumerate(items) if tuple(it[0].shape[:2]) == shp]
    oth = [k for k, it in enumerate(items) if tuple(it[0].shape[:2]) != shp]
    lut_np = np.asarray(lut, dtype=np.uint8)
    hf, hm = [], []
    for k in oth:
        f, m = host_resize_pil(items[k][0].numpy(), items[k][1].numpy(), size, lut_np)
        hf.append(torch.from_numpy(np.ascontiguousarray(f)))
        hm.append(torch.from_numpy(np.ascontiguousarray(m)))
    frames = torch.stack([items[k][0] for k in nat])
    masks = torch.stack([items[k][1] for k in nat])
    host_frames = torch.stack(hf) if hf else torch.empty((0, size, size, 3), dtype=torch.uint8)
    host_masks = torch.stack(hm) if hm else torch.empty((0, size, size), dtype=torch.uint8)
    fb = FrameBatch(frames, masks, torch.tensor(nat, dtype=torch.int64), host_frames, host_masks,
                    torch.tensor(oth, dtype=torch.int64), int(size), torch.from_numpy(lut_np.copy()))
    return fb, masks, torch.tensor([it[2] for it in items], dtype=torch.int64)


class _EndoFrames(torch.utils.data.Dataset):
    """Common body of the three datasets: sorted, checked pairs over the split's sequence folders; items by route
    (module docstring of ``tools.frame_resize`` and ``collate_frames``):
      transform=None, resize_on_gpu=True (and imsize set): (uint8 HWC native frame, uint8 raw single-channel mask, index)
      transform=None, resize_on_gpu=False: PIL resize on the host (BILINEAR / NEAREST), then the label table -> uint8 pair
      callable transform: host resize + table, then ``transform(image=, mask=)`` -> (float CHW / 255, long mask, index)."""

    lut = LUT_BINARY

    def __init__(self, folders, transform, imsize, resize_on_gpu, where):
        super().__init__()
        self.img_files, self.mask_files = [], []
        for img_dir, mask_dir in folders:
            a, b = _pair_folder(img_dir, mask_dir)
            self.img_files += a
            self.mask_files += b
        if not self.img_files:
            raise ValueError(f"{type(self).__name__}: no images under {where}")
        self.transform, self.imsize, self.resize_on_gpu = transform, imsize, bool(resize_on_gpu)

    def _mask_u8(self, mask, path):
        """The single-channel 8-bit mask the label table applies to."""
        if mask.mode in ("L", "P"):
            return np.array(mask, dtype=np.uint8)
        if mask.mode == "1":
            return np.array(mask.convert("L"), dtype=np.uint8)
        raise ValueError(f"{path}: mask mode {mask.mode}, expected a single-channel 8-bit image")

    @property
    def device_route(self):
        return self.transform is None and self.resize_on_gpu and self.imsize is not None

    @property
    def collate_fn(self):
        """``collate_fn`` for a DataLoader over this dataset."""
        if self.device_route:
            import functools
            return functools.partial(collate_frames, size=int(self.imsize), lut=self.lut)
        return collate_u8 if self.transform is None else None

    def __getitem__(self, index):
        from PIL import Image
        with open(self.img_files[index], "rb") as f:
            img = np.array(Image.open(f).convert("RGB"), dtype=np.uint8)
        with open(self.mask_files[index], "rb") as f:
            mask = self._mask_u8(Image.open(f), self.mask_files[index])
        if img.shape[:2] != mask.shape:
            raise ValueError(f"{self.img_files[index]}: frame {img.shape[:2]} and mask {mask.shape} differ in size")
        if self.device_route:
            return torch.from_numpy(img), torch.from_numpy(mask), index
        if self.imsize is not None:
            from .frame_resize import host_resize_pil
            img, mask = host_resize_pil(img, mask, int(self.imsize), self.lut)
        else:
            mask = self.lut[mask]
        if self.transform is not None:
            t = self.transform(image=img, mask=mask)
            return torch.from_numpy(t["image"].transpose(2, 0, 1).copy()) / 255.0, torch.from_numpy(t["mask"].copy()).long(), index
        return torch.from_numpy(np.ascontiguousarray(img)), torch.from_numpy(np.ascontiguousarray(mask)), index

    def __len__(self):
        return len(self.img_files)


def _split_range(cls, split, ranges):
    if split not in ranges:
        raise ValueError(f"{cls}: split must be one of {sorted(ranges)}, got {split!r}")
    return ranges[split]


class EndoVis2017(_EndoFrames):
    """`tools/dataset.py:7-71`: ``<root>/<split>/instrument_dataset_<i>/images/*`` with ``binary_masks/*`` (task="binary": mask
    ``convert('L')``, x > 0 -> 1) or ``instruments_masks/*`` (task="multi": floor(x / 32), 0, 32, ..., 224 -> classes 0..7);
    Train = 1..8, Test = 1..10."""

    def __init__(self, dir_main, split, transform=None, imsize=None, task="binary", resize_on_gpu=True):
        if task not in ("binary", "multi"):
            raise ValueError(f"EndoVis2017: task must be 'binary' or 'multi', got {task!r}")
        rng = _split_range("EndoVis2017", split, {"Train": range(1, 9), "Test": range(1, 11)})
        sub = "binary_masks" if task == "binary" else "instruments_masks"
        d = [os.path.join(dir_main, split, f"instrument_dataset_{i}") for i in rng]
        self.task = task
        self.lut = LUT_BINARY if task == "binary" else LUT_MULTI
        super().__init__([(os.path.join(p, "images"), os.path.join(p, sub)) for p in d], transform, imsize, resize_on_gpu,
                         os.path.join(dir_main, split))

    def _mask_u8(self, mask, path):
        if self.task == "binary":
            return np.array(mask.convert("L"), dtype=np.uint8)
        if mask.mode in ("L", "P"):
            return np.array(mask, dtype=np.uint8)
        # the reference's expression on any other mode: L of floor(x / 32); kept as label * 32 so the table maps it back
        from PIL import Image
        lab = np.array(Image.fromarray((np.array(mask) / 32.).astype(np.uint8)).convert("L"), dtype=np.uint8)
        if lab.max(initial=0) > 7:
            raise ValueError(f"{path}: mask mode {mask.mode} gives labels above 7")
        return lab << 5


class EndoVis2018(_EndoFrames):
    """`tools/dataset.py:74-125`: ``<root>/<split>/seq_<i>/{images,binary_masks}/*``, x > 0 -> 1 on the mask as read;
    Train = 1..15, Test = 1..4."""

    def __init__(self, dir_main, split, transform=None, imsize=None, resize_on_gpu=True):
        rng = _split_range("EndoVis2018", split, {"Train": range(1, 16), "Test": range(1, 5)})
        d = [os.path.join(dir_main, split, f"seq_{i}") for i in rng]
        super().__init__([(os.path.join(p, "images"), os.path.join(p, "binary_masks")) for p in d], transform, imsize,
                         resize_on_gpu, os.path.join(dir_main, split))


class Autolapro(_EndoFrames):
    """`tools/dataset.py:172-222`: ``<root>/<split>/seq_<i>/{images,binary_masks}/*`` for i in the split's range (Train =
    range(170), Validation = range(170, 227), Test = range(227, 300)); x > 0 -> 1 on the mask as read.  The reference loops
    over an undefined ``dataset_num`` (NameError); the split's range is the only reading consistent with the ranges it
    defines and the folders it globs."""

    def __init__(self, dir_main, split, transform=None, imsize=None, resize_on_gpu=True):
        rng = _split_range("Autolapro", split, {"Train": range(170), "Validation": range(170, 227), "Test": range(227, 300)})
        d = [os.path.join(dir_main, split, f"seq_{i}") for i in rng]
        super().__init__([(os.path.join(p, "images"), os.path.join(p, "binary_masks")) for p in d], transform, imsize,
                         resize_on_gpu, os.path.join(dir_main, split))


# ---- frames without labels (semi-supervised training: --unlabelled_path) ---------------------------------------------------------------
class UnlabelledFrames(torch.utils.data.Dataset):
    """Every ``*.png`` / ``*.jpg`` below ``root`` (sorted by path), decoded to RGB and resized on the host to ``imsize`` with PIL
    BILINEAR as the labelled sets resize theirs.  An item has the form the labelled sets' items have after the device resize:
    (uint8 HWC frame, uint8 mask [imsize, imsize] filled with ``IGNORE`` = 255, index); ``collate_u8`` batches them.  The mask
    carries no information: ``SegEngine.train_step(labelled=)`` fills the rows of unlabelled samples itself.
    ``root == "synthetic"``: ``n_synth`` seeded frames, the images of ``utils.weights.synthetic_batch`` under a seed of their own,
    as ``--data_path synthetic`` makes its labelled ones."""
    IGNORE = 255
    EXTENSIONS = (".png", ".jpg")

    def __init__(self, root, imsize, n_synth=24):
        super().__init__()
        self.imsize, self.frames = int(imsize), None
        if root == "synthetic":
            from ..utils import weights as W
            img, _ = W.synthetic_batch(n_synth, self.imsize, seed=3)
            self.frames = (img.permute(0, 2, 3, 1) * 255.0).round().clamp_(0, 255).to(torch.uint8).contiguous()
            self.files = list(range(n_synth))
            return
        if not os.path.isdir(root):
            raise ValueError(f"{root}: no such directory (the unlabelled frames: a directory, or 'synthetic')")
        self.files = sorted(os.path.join(d, f) for d, _, fs in os.walk(root) for f in fs if f.lower().endswith(self.EXTENSIONS))
        if not self.files:
            raise ValueError(f"{root}: no *.png or *.jpg frame below it")

    def __getitem__(self, index):
        mask = torch.full((self.imsize, self.imsize), self.IGNORE, dtype=torch.uint8)
        if self.frames is not None:
            return self.frames[index], mask, index
        from PIL import Image
        with open(self.files[index], "rb") as f:
            img = Image.open(f).convert("RGB")
        if img.size != (self.imsize, self.imsize):
            img = img.resize((self.imsize, self.imsize), resample=Image.BILINEAR)
        return torch.from_numpy(np.array(img).astype(np.uint8)), mask, index

    def __len__(self):
        return len(self.files)
