"""What tests/test_gpu_distill.py and tests/test_gpu_consist.py share: the small student and teacher maps, the tile sizes of a
side library, the bits of a tensor.  No test collects here."""
import math

import torch

from tests.bound_helpers import _gen

STUDENT = (5, 7)
TEACHER_SETS = {"same": [((5, 7), False)], "other": [((6, 4), False)], "three": [((5, 7), False), ((9, 3), True), ((4, 4), False)]}


def _maps(B, C, hw, views, scale, *key):
    """student NHWC [B,h,w,C], teacher maps and their flip flags, N(0,1) * scale, on the CPU"""
    g = _gen(*key)
    z = torch.randn((B,) + tuple(hw) + (C,), generator=g) * scale
    ts = [torch.randn((B,) + tuple(s) + (C,), generator=g) * scale for s, _ in views]
    return z, ts, [f for _, f in views]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _factor(n):
    a = max(d for d in range(1, int(math.isqrt(n)) + 1) if n % d == 0)
    return a, n // a


def _tile_sizes(lib, op):
    """(tile, cap) of the side library ``lib`` whose symbols are asis_<op>_tile / asis_<op>_nblk"""
    tile, cap = getattr(lib, f"asis_{op}_tile")(), getattr(lib, f"asis_{op}_nblk")((1 << 31) - 1)
    assert cap > 256                                                           # the finalize kernel sums 256 partials a sweep
    return tile, cap
