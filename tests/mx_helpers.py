"""Host decode of the MX form of a split-precision "lo" plane (two fp8 e4m3 bytes per element in a 16-bit container, one
power-of-two scale per tensor: csrc/asis_common.h), shared by the GPU tests that check a producer's byte image."""
import math

import torch


def e4m3(b: torch.Tensor) -> torch.Tensor:
    b = b.to(torch.int32)
    s, e, m = (b >> 7) & 1, (b >> 3) & 15, b & 7
    v = torch.where(e == 0, m.float() / 8.0 * 2.0 ** -6, (1.0 + m.float() / 8.0) * torch.exp2(e.float() - 7.0))
    return torch.where(s == 1, -v, v)


def mx_bytes(mx: torch.Tensor, wside: bool):
    """MX tensor (16-bit container) -> its (hi8, lo8) byte planes"""
    by = mx.contiguous().view(torch.uint8).view(*mx.shape, 2)
    return (by[..., 1], by[..., 0]) if wside else (by[..., 0], by[..., 1])


def decode(mx: torch.Tensor, amax: float, dt, wside: bool):
    """MX tensor (16-bit container) -> (hi, lo) float tensors"""
    b_hi, b_lo = mx_bytes(mx, wside)
    e = math.floor(math.log2(amax))
    lo_shift = 18 if dt == torch.float16 else 15
    return e4m3(b_hi) * 2.0 ** -(7 - e), e4m3(b_lo) * 2.0 ** -(lo_shift - e)
