"""Boundary metrics from the statistics of ``ops.surface_stats`` (host side, numpy only).

Per frame and class c, with P = (prediction == c), G = (label == c), E(.) their edge pixels (mask pixels on the image border or
with a 4-neighbour outside the mask) and d2_G / d2_P the exact squared distances to the nearest edge pixel of the other side:

    dice   = 2 |P and G| / (|P| + |G|)
    nsd[j] = (#{p in E(P): d2_G(p) <= floor(tau_j^2)} + #{g in E(G): d2_P(g) <= floor(tau_j^2)}) / (|E(P)| + |E(G)|)
    hd     = sqrt(max(max over E(P) of d2_G, max over E(G) of d2_P))              (Hausdorff distance of the boundaries)
    assd   = (sum over E(P) of sqrt(d2_G) + sum over E(G) of sqrt(d2_P)) / (|E(P)| + |E(G)|)

With percentiles (``--hd_percentile``; a percentile is handled as the integer q = hundredths of a percent, 9500 = 95 %), three
multisets of exact integers per frame and class: set 0 = {d2_G(p): p in E(P)} (n = |E(P)|), set 1 = {d2_P(g): g in E(G)}
(n = |E(G)|), set 2 = the two pooled.  With v[0..n-1] a set sorted ascending, r = (n - 1) q, lo = r // 10000, rem = r % 10000,
hi = lo + (rem != 0) (``surface_ranks``), the device returns the integers v[lo], v[hi] and

    pct(set, q) = sqrt(v[lo]) + (rem / 10000) (sqrt(v[hi]) - sqrt(v[lo]))         (``percentile_from_order``, float64)

which is ``numpy.percentile(sqrt(v), q / 100)`` with linear interpolation and the rank taken exactly.

    hd_pct     = pct(set 2, q)                           (the percentile of all boundary distances, both directions pooled)
    hd_pct_sym = max(pct(set 0, q), pct(set 1, q))       (the larger of the two directed percentiles)

q = 10000 gives ``hd`` for both.

Edge PIXELS are counted, each with weight one (no surface-element weighting by boundary length).  A class absent from both
prediction and label of a frame has no value there; a class in exactly one of them scores dice 0 and nsd 0, has no hd / assd,
and is counted under ``unmatched``.  Over a run: per class the mean over the frames that have a value; the headline means run
over the classes 1..C-1 that have a value (class 0, the background, is reported per class only, like ``ch_iou``)."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np

NFIXED = 7    # inter, n_pred, n_lab, e_pred, e_lab, max_pred, max_lab; then hit_pred[T], hit_lab[T]


QSCALE = 10000     # a percentile as an integer: hundredths of a percent
MAX_PERCENTILES = 4


def percentile_q(percent) -> int:
    """A percent in 0..100, a multiple of 0.01 to within 1e-9 -> the integer q in 0..10000."""
    v = float(percent)
    if not (0.0 <= v <= 100.0):       # also refuses nan
        raise ValueError(f"percentile {percent!r} must be in 0..100")
    q = int(round(v * 100.0))
    if abs(v * 100.0 - q) > 1e-7:
        raise ValueError(f"percentile {percent!r} must be a multiple of 0.01")
    return q


def percentile_qs(percentiles) -> List[int]:
    qs = [percentile_q(v) for v in percentiles]
    if not 1 <= len(qs) <= MAX_PERCENTILES:
        raise ValueError(f"{len(qs)} percentiles, supported 1..{MAX_PERCENTILES}")
    return qs


def surface_ranks(n: int, q: int):
    """-> (lo, hi, rem): the ranks of a set of ``n`` >= 1 values between which percentile ``q`` (0..10000) lies and the
    numerator of the interpolation weight rem / 10000, in exact integers."""
    n, q = int(n), int(q)
    if n < 1 or not 0 <= q <= QSCALE:
        raise ValueError(f"surface_ranks: n={n} must be >= 1 and q={q} in 0..{QSCALE}")
    lo, rem = divmod((n - 1) * q, QSCALE)
    return lo, lo + (rem != 0), rem


def percentile_from_order(v_lo: int, v_hi: int, rem: int) -> float:
    """The percentile of the distances from the two order statistics of the SQUARED distances, in float64."""
    a = math.sqrt(int(v_lo))
    return a + (int(rem) / QSCALE) * (math.sqrt(int(v_hi)) - a)


def metrics_from_stats(ints, sums, tolerances: Sequence[float], ord=None, percentiles=None) -> List[Optional[dict]]:
    """One frame's rows (ints int64 [C, 7 + 2 T], sums float64 [C, 2]) -> per class ``None`` (absent on both sides) or
    ``{"dice", "nsd": [T], "hd", "assd", "unmatched"}`` (hd and assd ``None`` when the class is on one side only).
    With ``percentiles`` (percents) and the frame's ``ord`` int64 [C, P, 3, 2] also ``"hd_pct"`` and ``"hd_pct_sym"``: lists of P
    values, ``None`` when the class is on one side only."""
    ints = np.asarray(ints, dtype=np.int64)
    sums = np.asarray(sums, dtype=np.float64)
    T = len(tolerances)
    if ints.ndim != 2 or ints.shape[1] != NFIXED + 2 * T or sums.shape != (ints.shape[0], 2):
        raise ValueError(f"metrics_from_stats: ints {ints.shape} / sums {sums.shape} do not match {T} tolerances "
                         f"(expected [C, {NFIXED + 2 * T}] and [C, 2])")
    if (ord is None) != (percentiles is None):
        raise ValueError("metrics_from_stats: ord and percentiles go together")
    qs = None
    if percentiles is not None:
        qs = percentile_qs(percentiles)
        ord = np.asarray(ord, dtype=np.int64)
        if ord.shape != (ints.shape[0], len(qs), 3, 2):
            raise ValueError(f"metrics_from_stats: ord {ord.shape}, expected [C, {len(qs)}, 3, 2]")
    out: List[Optional[dict]] = []
    for c, (row, s) in enumerate(zip(ints, sums)):
        inter, n_pred, n_lab, e_pred, e_lab, max_pred, max_lab = (int(v) for v in row[:NFIXED])
        if n_pred == 0 and n_lab == 0:
            out.append(None)
            continue
        if n_pred == 0 or n_lab == 0:
            m = {"dice": 0.0, "nsd": [0.0] * T, "hd": None, "assd": None, "unmatched": True}
            if qs is not None:
                m["hd_pct"] = m["hd_pct_sym"] = None
        else:
            e = e_pred + e_lab
            m = {"dice": 2.0 * inter / (n_pred + n_lab),
                 "nsd": [(int(row[NFIXED + j]) + int(row[NFIXED + T + j])) / e for j in range(T)],
                 "hd": math.sqrt(max(max_pred, max_lab)), "assd": (float(s[0]) + float(s[1])) / e, "unmatched": False}
            if qs is not None:
                if int(ord[c].min()) < 0:
                    raise ValueError(f"metrics_from_stats: class {c} is on both sides but its order statistics are missing")
                pct = [[percentile_from_order(int(ord[c, p, k, 0]), int(ord[c, p, k, 1]), surface_ranks(n, q)[2])
                        for k, n in enumerate((e_pred, e_lab, e))] for p, q in enumerate(qs)]
                m["hd_pct"] = [v[2] for v in pct]
                m["hd_pct_sym"] = [max(v[0], v[1]) for v in pct]
        out.append(m)
    return out


def _mean(total: float, n: int) -> Optional[float]:
    return total / n if n else None


class SurfaceMeter:
    """Accumulates the statistics of frames and returns the run's aggregation (module docstring)."""

    def __init__(self, num_classes: int, tolerances: Sequence[float], percentiles: Optional[Sequence[float]] = None):
        self.C, self.tol = int(num_classes), [float(t) for t in tolerances]
        self.pct = None if percentiles is None else [float(v) for v in percentiles]
        if self.pct is not None:
            percentile_qs(self.pct)
        T, P = len(self.tol), len(self.pct or ())
        self.frames = 0
        self.n = np.zeros(self.C, dtype=np.int64)           # frames with a value (dice / nsd)
        self.matched = np.zeros(self.C, dtype=np.int64)     # frames with hd / assd
        self.unmatched = np.zeros(self.C, dtype=np.int64)
        self.dice = np.zeros(self.C, dtype=np.float64)
        self.nsd = np.zeros((self.C, T), dtype=np.float64)
        self.hd = np.zeros(self.C, dtype=np.float64)
        self.assd = np.zeros(self.C, dtype=np.float64)
        self.hd_pct = np.zeros((self.C, P), dtype=np.float64)       # summed over the matched frames, like hd
        self.hd_pct_sym = np.zeros((self.C, P), dtype=np.float64)

    def update(self, ints, sums, ord=None) -> None:
        """ints [B, C, 7 + 2 T] / sums [B, C, 2] of a batch (or one frame's [C, ...] rows), as numpy arrays or host tensors;
        with percentiles also ord [B, C, P, 3, 2]."""
        ints, sums = np.asarray(ints), np.asarray(sums)
        if (ord is None) != (self.pct is None):
            raise ValueError("SurfaceMeter.update: ord is given exactly when the meter has percentiles")
        if ints.ndim == 2:
            ints, sums = ints[None], sums[None]
            ord = None if ord is None else np.asarray(ord)[None]
        if ints.ndim != 3 or ints.shape[1] != self.C:
            raise ValueError(f"SurfaceMeter.update: ints {ints.shape}, expected [B, {self.C}, {NFIXED + 2 * len(self.tol)}]")
        ords = [None] * len(ints) if ord is None else np.asarray(ord)
        if len(ords) != len(ints):
            raise ValueError(f"SurfaceMeter.update: ord of {len(ords)} frames, ints of {len(ints)}")
        for fi, fs, fo in zip(ints, sums, ords):
            self.frames += 1
            for c, m in enumerate(metrics_from_stats(fi, fs, self.tol, fo, self.pct)):
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
                    if self.pct is not None:
                        self.hd_pct[c] += np.asarray(m["hd_pct"], dtype=np.float64)
                        self.hd_pct_sym[c] += np.asarray(m["hd_pct_sym"], dtype=np.float64)

    def result(self) -> dict:
        T = len(self.tol)
        per_class = []
        for c in range(self.C):
            n, k = int(self.n[c]), int(self.matched[c])
            per_class.append({"dice": _mean(float(self.dice[c]), n),
                              "nsd": [float(self.nsd[c, j]) / n for j in range(T)] if n else None,
                              "hd": _mean(float(self.hd[c]), k), "assd": _mean(float(self.assd[c]), k),
                              "frames": n, "frames_matched": k, "unmatched": int(self.unmatched[c])})
            if self.pct is not None:
                for key, tot in (("hd_pct", self.hd_pct), ("hd_pct_sym", self.hd_pct_sym)):
                    per_class[-1][key] = [float(tot[c, p]) / k for p in range(len(self.pct))] if k else None

        def over_classes(get):
            vals = [get(p) for p in per_class[1:] if get(p) is not None]
            return float(np.mean(vals)) if vals else None

        mean_nsd = [over_classes(lambda p, j=j: None if p["nsd"] is None else p["nsd"][j]) for j in range(T)]
        out = {"tolerances": list(self.tol), "frames": self.frames, "per_class": per_class,
               "mean_dice": over_classes(lambda p: p["dice"]), "mean_nsd": mean_nsd,
               "mean_hd": over_classes(lambda p: p["hd"]), "mean_assd": over_classes(lambda p: p["assd"])}
        if self.pct is not None:
            out["percentiles"] = list(self.pct)
            for key in ("hd_pct", "hd_pct_sym"):
                out["mean_" + key] = [over_classes(lambda p, j=j: None if p[key] is None else p[key][j]) for j in range(len(self.pct))]
        return out
