"""CPU oracle of the boundary statistics (helper module of test_surface_host.py / test_gpu_surface.py): the scipy recipe.

Edge pixels: ``M and not binary_erosion(M, cross, border_value=0)``; squared distance to the nearest edge pixel:
``distance_transform_edt(~edges)`` squared and rounded to int64 (exact below 2^52); every comparison on integers."""
import math

import numpy as np
from scipy import ndimage

CROSS = ndimage.generate_binary_structure(2, 1)
NCOL_FIXED = 7    # inter, n_pred, n_lab, e_pred, e_lab, max_pred, max_lab


def edges_of(mask: np.ndarray) -> np.ndarray:
    return mask & ~ndimage.binary_erosion(mask, CROSS, border_value=0)


def d2_of(edges: np.ndarray) -> np.ndarray:
    """int64 [H, W]: squared Euclidean distance to the nearest True pixel of ``edges`` (which must have one)."""
    d = ndimage.distance_transform_edt(~edges)
    return np.rint(d * d).astype(np.int64)


def thresholds(tolerances):
    return [int(math.floor(float(t) * float(t))) for t in tolerances]


def frame_class_stats(P: np.ndarray, G: np.ndarray, tolerances):
    """bool [H, W] masks -> (int64 [7 + 2 T], float64 [2], d2 of E(P) or None, d2 of E(G) or None)."""
    thr = thresholds(tolerances)
    T = len(thr)
    ints = np.zeros(NCOL_FIXED + 2 * T, dtype=np.int64)
    sums = np.zeros(2, dtype=np.float64)
    eP, eG = edges_of(P), edges_of(G)
    ints[:5] = (P & G).sum(), P.sum(), G.sum(), eP.sum(), eG.sum()
    dP = d2_of(eP) if ints[3] else None
    dG = d2_of(eG) if ints[4] else None
    if ints[3] and ints[4]:
        at_p, at_g = dG[eP], dP[eG]          # field of the other side at this side's edge pixels
        ints[5], ints[6] = at_p.max(), at_g.max()
        for j, t in enumerate(thr):
            ints[7 + j] = (at_p <= t).sum()
            ints[7 + T + j] = (at_g <= t).sum()
        sums[0] = np.sqrt(at_p.astype(np.float64)).sum()
        sums[1] = np.sqrt(at_g.astype(np.float64)).sum()
    return ints, sums, dP, dG


def stats(pred: np.ndarray, target: np.ndarray, num_classes: int, tolerances, pred_lut=None, lut=None, want_d2=False):
    """uint8 [B, H, W] raw maps -> ints int64 [B, C, 7 + 2 T], sums float64 [B, C, 2][, d2_pred, d2_target: dicts (b, c) -> field]."""
    ident = np.arange(256, dtype=np.uint8)
    p = np.asarray(ident if pred_lut is None else pred_lut, dtype=np.uint8)[pred]
    g = np.asarray(ident if lut is None else lut, dtype=np.uint8)[target]
    B, C, T = pred.shape[0], num_classes, len(tolerances)
    ints = np.zeros((B, C, NCOL_FIXED + 2 * T), dtype=np.int64)
    sums = np.zeros((B, C, 2), dtype=np.float64)
    d2p, d2g = {}, {}
    for b in range(B):
        for c in range(C):
            P, G = p[b] == c, g[b] == c
            if not P.any() and not G.any():
                continue
            ints[b, c], sums[b, c], dP, dG = frame_class_stats(P, G, tolerances)
            if dP is not None:
                d2p[b, c] = dP
            if dG is not None:
                d2g[b, c] = dG
    return (ints, sums, d2p, d2g) if want_d2 else (ints, sums)
