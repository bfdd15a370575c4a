"""The one cache of derived operands (16-bit, re-laid-out, folded or concatenated copies of parameters).

A cache is a plain dict ``key -> (tag, value)``.  The tag says which state of its sources a value was built from; it is built in
one place, ``tag_of``, so every pack in the package goes stale under the same conditions: a source was written through torch
(``_version``), written by a fused optimizer / a LoRA re-merge that leaves ``_version`` alone (``_asis_gen``), replaced
(``data_ptr``), moved (device), or ``config.operand_dtype`` / a caller's ``extra`` changed.
"""
from __future__ import annotations

from typing import Callable

import torch

from . import config


def tag_of(sources, extra=()) -> tuple:
    """``sources``: a tuple of tensors (None entries skipped), at least one of them a tensor."""
    tag, dev = (), None         # this runs in front of every GEMM launch: tuples only
    for t in sources:
        if t is not None:
            if dev is None:
                dev = t.device
            tag += ((t.data_ptr(), t._version, getattr(t, "_asis_gen", 0)),)
    return tag + (dev, config.operand_dtype) + extra


def derived(cache: dict, key: str, sources, fn: Callable[[], object], extra=()):
    """``fn()`` (run under no_grad), cached under ``key`` until one of ``sources``, the operand dtype or ``extra`` changes"""
    tag = tag_of(sources, extra)
    hit = cache.get(key)
    if hit is None or hit[0] != tag:
        with torch.no_grad():
            hit = cache[key] = (tag, fn())
    return hit[1]
