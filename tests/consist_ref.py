"""Restatement of the gated consistency loss of csrc/consist.hip in plain torch, on top of tests/distill_ref.py (float64 by default;
the tests also evaluate it in float32 on the CPU for the yardstick Y of tests/bound_helpers.py):

    z, p, q as in tests/distill_ref.py (``soft_targets`` gives q)
    conf_i = max_c q_c,  m_i = [conf_i >= threshold] (None or <= 0: every pixel),  w_b = sample_weight[b] (None: 1)
    kd_i = sum_c q_c (log q_c - log p_c)
    loss = T^2 sum_i w_b m_i kd_i / N,  N = B H W  (not the kept count)
    kept = sum_i m_i [w_b > 0]
    dz = d loss / d z = (T / N) w_b m_i (p - q)   (autograd), dlow = d loss / d student through the interpolate

Without a threshold and without weights nothing is multiplied in: the value and the gradients are those of ``distill_ref`` bit for bit.
"""
from types import SimpleNamespace

import torch

from tests.distill_ref import _resized, _size, soft_targets


def confidence(teachers, flips, size, T, dtype=torch.float64) -> torch.Tensor:
    """conf [B,H,W] = max_c q_c"""
    flips = [False] * len(teachers) if flips is None else list(flips)
    return soft_targets(teachers, flips, _size(size), T, dtype).amax(dim=1)


def consist_ref(student, teachers, flips, size, T, threshold=None, sample_weight=None, dtype=torch.float64, gate=None):
    """-> namespace(loss 0-dim, dz NHWC [B,H,W,C], dlow NHWC [B,h,w,C], kept int, conf [B,H,W], gate bool [B,H,W] (the gate alone,
    without the weights), kd [B,H,W] (per pixel, neither gated nor weighted), p, q NCHW), all ``dtype`` on the CPU.  ``gate``: a
    bool [B,H,W] to use instead of [conf >= threshold] (the float32 yardstick of a case whose float64 gate has near-threshold
    pixels takes the float64 gate)."""
    size = _size(size)
    flips = [False] * len(teachers) if flips is None else list(flips)
    s = student.detach().cpu().to(dtype).clone().requires_grad_(True)
    z = _resized(s, size)
    z.retain_grad()
    q = soft_targets(teachers, flips, size, T, dtype)
    logp = torch.log_softmax(z / T, dim=1)
    B, _, H, W = z.shape
    N = B * H * W
    conf = q.amax(dim=1)
    if gate is None:
        gate = torch.ones((B, H, W), dtype=torch.bool) if threshold is None or threshold <= 0 else conf >= threshold
    terms = torch.xlogy(q, q) - q * logp
    kd = terms.detach().sum(dim=1)
    wb = None if sample_weight is None else sample_weight.detach().cpu().to(dtype).view(B, 1, 1)
    if not bool(gate.all()):
        terms = terms * gate.to(dtype).unsqueeze(1)
    if wb is not None:
        terms = terms * wb.unsqueeze(1)
    loss = (T * T) * terms.sum() / N
    loss.backward()
    kept = int((gate & (wb > 0)).sum()) if wb is not None else int(gate.sum())
    return SimpleNamespace(loss=loss.detach(), dz=z.grad.permute(0, 2, 3, 1).contiguous(), dlow=s.grad, kept=kept, conf=conf, gate=gate,
                           kd=kd, p=logp.detach().exp(), q=q)


def pick_threshold(conf: torch.Tensor, delta: float = 1e-5):
    """A threshold that no float64 confidence is near: the midpoint of the widest gap between adjacent sorted confidences among the
    gaps that leave 10..90 % of the pixels kept; where that gap is under 2 delta, of the widest gap overall.  Rounded to float32
    (what the device is given).  -> (threshold, note); raises where a confidence lies within ``delta`` of it."""
    c = conf.double().flatten().sort().values
    n = c.numel()
    gaps = c[1:] - c[:-1]
    share = (n - 1 - torch.arange(n - 1, dtype=torch.float64)) / n       # kept share with the threshold in gap j
    mid = (share >= 0.1) & (share <= 0.9)
    j, note = None, "mid-range gap"
    if bool(mid.any()):
        j = int(torch.where(mid, gaps, torch.full_like(gaps, -1.0)).argmax())
    if j is None or float(gaps[j]) < 2 * delta:
        j, note = int(gaps.argmax()), "widest gap overall"
    tau = float(torch.tensor((float(c[j]) + float(c[j + 1])) / 2, dtype=torch.float32))
    nearest = float((conf.double() - tau).abs().min())
    if not nearest > delta:
        raise AssertionError(f"no threshold clear of every confidence by {delta}: the nearest lies {nearest:.3e} from {tau}")
    return tau, f"{note} {float(gaps[j]):.2e}, kept share {float(share[j]):.2f}"
