"""Restatement of the distillation loss of csrc/distill.hip in plain torch (float64 by default; the tests also evaluate it in float32
on the CPU for the yardstick Y of tests/bound_helpers.py):

    z   = F.interpolate(student, (H, W), bilinear, align_corners=False)         maps are NHWC [B,h,w,C] and go through NCHW
    t_k = the same of teacher map k; a mirrored map is ``map.flip(2)`` (its columns) read un-mirrored
    p = softmax(z / T),  q = (1/V) sum_k softmax(t_k / T)   (views in list order)
    kd_i = sum_c q_c (log q_c - log p_c), 0 where q_c = 0  (xlogy; log p from log_softmax, so a saturated p_c costs a finite amount)
    loss = T^2 sum_i kd_i / N,  N = B H W
    dz = d loss / d z = (T / N) (p - q)                     (autograd), dlow = d loss / d student through the interpolate
"""
import torch
import torch.nn.functional as F


def _size(size):
    return (size, size) if isinstance(size, int) else tuple(int(s) for s in size)


def _resized(x_nhwc: torch.Tensor, size):
    return F.interpolate(x_nhwc.permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=False)


def soft_targets(teachers, flips, size, T, dtype=torch.float64) -> torch.Tensor:
    """q, NCHW [B,C,H,W]"""
    q = None
    for t, f in zip(teachers, flips):
        t = t.detach().cpu().to(dtype)
        s = torch.softmax(_resized(t.flip(2) if f else t, size) / T, dim=1)
        q = s if q is None else q + s
    return q / len(teachers)


def distill_ref(student, teachers, flips, size, T, dtype=torch.float64):
    """-> (loss 0-dim, dz NHWC [B,H,W,C], dlow NHWC [B,h,w,C], p NCHW, q NCHW), all ``dtype`` on the CPU"""
    size = _size(size)
    flips = [False] * len(teachers) if flips is None else list(flips)
    s = student.detach().cpu().to(dtype).clone().requires_grad_(True)
    z = _resized(s, size)
    z.retain_grad()
    q = soft_targets(teachers, flips, size, T, dtype)
    logp = torch.log_softmax(z / T, dim=1)
    N = z.shape[0] * z.shape[2] * z.shape[3]
    loss = (T * T) * (torch.xlogy(q, q) - q * logp).sum() / N
    loss.backward()
    return loss.detach(), z.grad.permute(0, 2, 3, 1).contiguous(), s.grad, logp.detach().exp(), q
