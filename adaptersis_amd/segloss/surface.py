"""Boundary metrics from the statistics of ``ops.surface_stats`` (host side, numpy only).

Per frame and class c, with P = (prediction == c), G = (label == c), E(.) their edge pixels (mask pixels on the image border or
with a 4-neighbour outside the mask) and d2_G / d2_P the exact squared distances to the nearest edge pixel of the other side:

    dice   = 2 |P and G| / (|P| + |G|)
    nsd[j] = (#{p in E(P): d2_G(p) <= floor(tau_j^2)} + #{g in E(G): d2_P(g) <= floor(tau_j^2)}) / (|E(P)| + |E(G)|)
    hd     = sqrt(max(max over E(P) of d2_G, max over E(G) of d2_P))              (Hausdorff distance of the boundaries)
    assd   = (sum over E(P) of sqrt(d2_G) + sum over E(G) of sqrt(d2_P)) / (|E(P)| + |E(G)|)

Edge PIXELS are counted, each with weight one (no surface-element weighting by boundary length).  A class absent from both
prediction and label of a frame has no value there; a class in exactly one of them scores dice 0 and nsd 0, has no hd / assd,
and is counted under ``unmatched``.  Over a run: per class the mean over the frames that have a value; the headline means run
over the classes 1..C-1 that have a value (class 0, the background, is reported per class only, like ``ch_iou``)."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

NFIXED = 7    # inter, n_pred, n_lab, e_pred, e_lab, max_pred, max_lab; then hit_pred[T], hit_lab[T]


def metrics_from_stats(ints, sums, tolerances: Sequence[float]) -> List[Optional[dict]]:
    """One frame's rows (ints int64 [C, 7 + 2 T], sums float64 [C, 2]) -> per class ``None`` (absent on both sides) or
    ``{"dice", "nsd": [T], "hd", "assd", "unmatched"}`` (hd and assd ``None`` when the class is on one side only)."""
    ints = np.asarray(ints, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    T = len(tolerances)
    if ints.ndim != 2 or ints.shape[1] != NFIXED + 2 * T or sums.shape != (ints.shape[0], 2):
        raise ValueError(f"metrics_from_stats: ints {ints.shape} / sums {sums.shape} do not match {T} tolerances "
                         f"(expected [C, {NFIXED + 2 * T}] and [C, 2])")
    out: List[Optional[dict]] = []
    for row, s in zip(ints, sums):
        inter, n_pred, n_lab, e_pred, e_lab, max_pred, max_lab = (int(v) for v in row[:NFIXED])
        if n_pred == 0 and n_lab == 0:
            out.append(None)
        elif n_pred == 0 or n_lab == 0:
            out.append({"dice": 0.0, "nsd": [0.0] * T, "hd": None, "assd": None, "unmatched": True})
        else:
            e = e_pred + e_lab
            out.append({"dice": 2.0 * inter / (n_pred + n_lab),
                        "nsd": [(int(row[NFIXED + j]) + int(row[NFIXED + T + j])) / e for j in range(T)],
                        "hd": math.sqrt(max(max_pred, max_lab)), "assd": (float(s[0]) + float(s[1])) / e, "unmatched": False})
    return out


def _mean(total: float, n: int) -> Optional[float]:
    return total / n if n else None


class SurfaceMeter:
    """Accumulates the statistics of frames and returns the run's aggregation (module docstring)."""

    def __init__(self, num_classes: int, tolerances: Sequence[float]):
        self.C, self.tol = int(num_classes), [float(t) for t in tolerances]
        T = len(self.tol)
        self.frames = 0
        self.n = np.zeros(self.C, dtype=np.int64)           # frames with a value (dice / nsd)
        self.matched = np.zeros(self.C, dtype=np.int64)     # frames with hd / assd
        self.unmatched = np.zeros(self.C, dtype=np.int64)
        self.dice = np.zeros(self.C, dtype=np.float64)
        self.nsd = np.zeros((self.C, T), dtype=np.float64)
        self.hd = np.zeros(self.C, dtype=np.float64)
        self.assd = np.zeros(self.C, dtype=np.float64)

    def update(self, ints, sums) -> None:
        """ints [B, C, 7 + 2 T] / sums [B, C, 2] of a batch (or one frame's [C, ...] rows), as numpy arrays or host tensors."""
        ints, sums = np.asarray(ints), np.asarray(sums)
        if ints.ndim == 2:
            ints, sums = ints[None], sums[None]
        if ints.ndim != 3 or ints.shape[1] != self.C:
            raise ValueError(f"SurfaceMeter.update: ints {ints.shape}, expected [B, {self.C}, {NFIXED + 2 * len(self.tol)}]")
        for fi, fs in zip(ints, sums):
            self.frames += 1
            for c, m in enumerate(metrics_from_stats(fi, fs, self.tol)):
                if m is None:
                    continue
                self.n[c] += 1
                self.dice[c] += m["dice"]
                self.nsd[c] += np.asarray(m["nsd"], dtype=np.float64)
                if m["unmatched"]:
                    self.unmatched[c] += 1
                else:
                    self.matched[c] += 1
                    self.hd[c] += m["hd"]
                    self.assd[c] += m["assd"]

    def result(self) -> dict:
        T = len(self.tol)
        per_class = []
        for c in range(self.C):
            n, k = int(self.n[c]), int(self.matched[c])
            per_class.append({"dice": _mean(float(self.dice[c]), n),
                              "nsd": [float(self.nsd[c, j]) / n for j in range(T)] if n else None,
                              "hd": _mean(float(self.hd[c]), k), "assd": _mean(float(self.assd[c]), k),
                              "frames": n, "frames_matched": k, "unmatched": int(self.unmatched[c])})

        def over_classes(get):
            vals = [get(p) for p in per_class[1:] if get(p) is not None]
            return float(np.mean(vals)) if vals else None

        mean_nsd = [over_classes(lambda p, j=j: None if p["nsd"] is None else p["nsd"][j]) for j in range(T)]
        return {"tolerances": list(self.tol), "frames": self.frames, "per_class": per_class,
                "mean_dice": over_classes(lambda p: p["dice"]), "mean_nsd": mean_nsd,
                "mean_hd": over_classes(lambda p: p["hd"]), "mean_assd": over_classes(lambda p: p["assd"])}
