"""On-device frame resize, bit-identical to PIL — the ``img.resize((S, S), BILINEAR)`` / ``mask.resize((S, S), NEAREST)`` that
the reference's datasets run on the host for every frame (`tools/dataset.py:51-53`), plus the label mapping of the mask.

Pillow's 8-bit BILINEAR resample (``precompute_coeffs`` + ``normalize_coeffs_8bpc`` of its ``Resample.c``), restated per axis:

    scale = in / out ; fs = max(scale, 1) ; support = fs ; ksize = 2 * ceil(support) + 1
    center = (xx + 0.5) * scale ; xmin = max(int(center - support + 0.5), 0) ; n = min(int(center + support + 0.5), in) - xmin
    w_j = max(0, 1 - |(j + xmin - center + 0.5) / fs|) / sum_j w_j        (float64, summed in order)
    k_j = int(0.5 + w_j * 2^22)                                            (fixed point, 22 fractional bits)
    out = clip8(2^21 + sum_j k_j * px)  with clip8(a) = 255 if a >= 2^30, 0 if a <= 0, else a >> 22

horizontal pass first, rounded to uint8, then the vertical pass on its result; an axis whose size does not change is
skipped.  NEAREST (Pillow's affine nearest transform) accumulates the source coordinate: v = scale / 2, v += scale per output,
index = min(int(v), in - 1) — the multiplied form floor((x + 0.5) * scale) differs from it on some pixels.

The tables are built here in float64 (cached per (in, out) pair); ``csrc/frame_resize.hip`` does the integer arithmetic.
``resize_frame_host`` / ``resize_mask_host`` are the numpy restatement of what the kernel computes (the CPU tests hold it to
PIL), ``host_resize_pil`` is the PIL route a loader takes on the host.
"""
from __future__ import annotations

import math
from functools import lru_cache
from typing import Dict, Tuple

import numpy as np
import torch

PRECISION_BITS = 22

# 256-entry uint8 label tables applied to the single-channel 8-bit mask (tools/dataset.py)
LUT_BINARY = (np.arange(256) > 0).astype(np.uint8)          # x > 0 -> 1
LUT_MULTI = (np.arange(256) >> 5).astype(np.uint8)          # floor(x / 32): instruments_masks 0, 32, ..., 224 -> 0..7
LUT_IDENTITY = np.arange(256, dtype=np.uint8)

# class index -> pixel value of the mask files (``ops.predict_mask``): each the inverse of the label table its dataset reads with
ENCODE_INDEX = np.arange(16, dtype=np.uint8)                        # c
ENCODE_BINARY255 = np.array([0, 255], dtype=np.uint8)               # Robust-MIS, EndoVis 2018, AutoLaparo, EndoVis 2017 binary_masks
ENCODE_ENDOVIS2017 = (np.arange(8) * 32).astype(np.uint8)           # 32 c: instruments_masks (instruments_factor)
# name -> (encode table, the label table it inverts)
ENCODINGS = {"index": (ENCODE_INDEX, LUT_IDENTITY), "binary255": (ENCODE_BINARY255, LUT_BINARY),
             "endovis2017": (ENCODE_ENDOVIS2017, LUT_MULTI)}


def encode_table(name: str, num_classes: int) -> np.ndarray:
    """uint8 [num_classes] of the named encoding; raises when the encoding has fewer classes."""
    if name not in ENCODINGS:
        raise ValueError(f"encode must be one of {sorted(ENCODINGS)}, got {name!r}")
    enc = ENCODINGS[name][0]
    if not 1 <= num_classes <= len(enc):
        raise ValueError(f"encoding {name!r} covers {len(enc)} classes, the model has {num_classes}")
    return enc[:num_classes].copy()


def default_palette(num_classes: int) -> np.ndarray:
    """uint8 [C, 3]: green for every class, the reference's ``draw_segmentation_masks(colors="green")``."""
    return np.tile(np.array([[0, 128, 0]], dtype=np.uint8), (num_classes, 1))


def default_alpha(num_classes: int, alpha: float = 0.5) -> np.ndarray:
    """uint8 [C]: class 0 leaves the frame untouched, every other class blends with round(255 * alpha) (reference: .5)."""
    a = np.full(num_classes, int(round(255 * float(alpha))), dtype=np.uint8)
    a[0] = 0
    return a


@lru_cache(maxsize=64)
def bilinear_tables(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """-> (span int32 [n_out, 2] = (xmin, n), coef int32 [n_out, ksize]; zero past n) for one axis."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"bilinear_tables: sizes must be positive, got {n_in} -> {n_out}")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = 2 * int(math.ceil(support)) + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    n = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), n_in) - xmin
    j = np.arange(ksize, dtype=np.float64)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs((j + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fs)))
    w[np.arange(ksize)[None, :] >= n[:, None]] = 0.0
    ww = np.zeros(n_out, dtype=np.float64)
    for c in range(ksize):                   # summed in Pillow's order (numpy's pairwise sum would reorder it)
        ww = ww + w[:, c]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.trunc(0.5 + w * float(1 << PRECISION_BITS)).astype(np.int32)
    span = np.stack([xmin, n], -1).astype(np.int32)
    span.setflags(write=False)
    k.setflags(write=False)
    return span, k


@lru_cache(maxsize=64)
def nearest_table(n_in: int, n_out: int) -> np.ndarray:
    """Source index per output index of Pillow's NEAREST resize: int32 [n_out]."""
    scale = n_in / n_out
    idx = np.empty(n_out, dtype=np.int32)
    v = scale * 0.5
    for i in range(n_out):
        idx[i] = min(int(v), n_in - 1)
        v += scale
    idx.setflags(write=False)
    return idx


def _clip8(acc: np.ndarray) -> np.ndarray:
    return np.where(acc >= (1 << 30), 255, np.where(acc <= 0, 0, acc >> PRECISION_BITS)).astype(np.uint8)


def _pass(x: np.ndarray, axis: int, n_out: int) -> np.ndarray:
    span, k = bilinear_tables(x.shape[axis], n_out)
    xs = np.moveaxis(x, axis, 0).astype(np.int64)
    acc = np.full((n_out,) + xs.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for j in range(k.shape[1]):
        src = np.minimum(span[:, 0] + j, x.shape[axis] - 1)        # k_j = 0 past n: the clamped index adds nothing
        acc += k[:, j].reshape((-1,) + (1,) * (xs.ndim - 1)).astype(np.int64) * xs[src]
    return np.moveaxis(_clip8(acc), 0, axis)


def resize_frame_host(img: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """numpy restatement of the kernel: uint8 [H, W, C] -> uint8 [out_h, out_w, C] (horizontal pass, then vertical)."""
    x = np.asarray(img, dtype=np.uint8)
    if x.shape[1] != out_w:
        x = _pass(x, 1, out_w)
    if x.shape[0] != out_h:
        x = _pass(x, 0, out_h)
    return x


def resize_mask_host(mask: np.ndarray, out_h: int, out_w: int, lut: np.ndarray = LUT_IDENTITY) -> np.ndarray:
    """uint8 [H, W] -> lut[mask[iy, ix]] uint8 [out_h, out_w]."""
    m = np.asarray(mask, dtype=np.uint8)
    iy, ix = nearest_table(m.shape[0], out_h), nearest_table(m.shape[1], out_w)
    return np.asarray(lut, dtype=np.uint8)[m[iy][:, ix]]


def host_resize_pil(img: np.ndarray, mask: np.ndarray, size: int, lut: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The host route: PIL BILINEAR for the frame, PIL NEAREST for the mask, then the label table."""
    from PIL import Image
    if img.shape[:2] != (size, size):
        img = np.array(Image.fromarray(img).resize((size, size), resample=Image.BILINEAR), dtype=np.uint8)
    if mask.shape != (size, size):
        mask = np.array(Image.fromarray(mask).resize((size, size), resample=Image.NEAREST), dtype=np.uint8)
    return img, np.asarray(lut, dtype=np.uint8)[mask]


_DEVICE_TABLES: Dict[tuple, Dict[str, torch.Tensor]] = {}


def device_tables(h_in: int, w_in: int, size: int, device) -> Dict[str, torch.Tensor]:
    """Cached device copies of the tables for [h_in, w_in] -> [size, size]."""
    key = (h_in, w_in, size, str(device))
    t = _DEVICE_TABLES.get(key)
    if t is None:
        xs, xk = bilinear_tables(w_in, size)
        ys, yk = bilinear_tables(h_in, size)
        arrs = dict(xspan=xs, xcoef=xk, yspan=ys, ycoef=yk, ix=nearest_table(w_in, size), iy=nearest_table(h_in, size))
        t = _DEVICE_TABLES[key] = {k: torch.from_numpy(np.array(v)).to(device) for k, v in arrs.items()}
    return t
