"""Restatement of csrc/mix.hip in plain torch on the CPU, on top of tests/distill_ref.py and tests/consist_ref.py:

    present[d]   = the classes c in 0..C-1 with some pixel of target[d] equal to c (other labels are never present)
    pasted[b]    = for kind[b] == 2, with P = present[donor[b]] (without class 0 unless ``background``): the first ceil(|P| / 2)
                   members of P in the order order[b]; empty for every other kind
    sel[b,y,x]   = kind 1: (y, x) inside box[b] = (y0, x0, y1, x1), half-open; kind 2: target[donor[b]][y,x] in pasted[b]; else 0
    inp'[b]      = where(sel[b], inp[donor[b]], inp[b]), target' likewise; pasted count[b] = sum sel[b]
    mixed maps   = every teacher map resized as ``distill_ref._resized`` does (a mirrored map un-mirrored first), then gathered per
                   pixel from sample donor[b] where sel; q = the mean of their softmaxes
    mixed loss   = ``consist_ref`` on those maps: a map that already has the size (H, W) passes its resize unchanged (the bilinear
                   weights are exactly 1 and 0), so the student, the gate, the weights, kept and dz are that function's
"""
import torch

from tests.consist_ref import consist_ref
from tests.distill_ref import _resized, _size


def presence(target: torch.Tensor, C: int):
    """-> per sample the set of classes present"""
    return [{c for c in range(C) if bool((t == c).any())} for t in target.cpu()]


def pasted_sets(target, tables, C: int, background: bool = False):
    """-> per sample the set of classes it pastes"""
    present = presence(target, C)
    out = []
    for b in range(target.shape[0]):
        chosen = set()
        if int(tables["kind"][b]) == 2:
            P = {c for c in present[int(tables["donor"][b])] if background or c != 0}
            ranked = [int(c) for c in tables["order"][b] if int(c) in P]
            chosen = set(ranked[:(len(P) + 1) // 2])
        out.append(chosen)
    return out


def sel_ref(target, tables, C: int, background: bool = False) -> torch.Tensor:
    target = target.cpu()
    B, H, W = target.shape
    sel = torch.zeros((B, H, W), dtype=torch.bool)
    sets = pasted_sets(target, tables, C, background)
    for b in range(B):
        k, d = int(tables["kind"][b]), int(tables["donor"][b])
        if k == 1:
            y0, x0, y1, x1 = (int(v) for v in tables["box"][b])
            sel[b, max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
        elif k == 2:
            for c in sets[b]:
                sel[b] |= target[d] == c
    return sel.to(torch.uint8)


def mix_ref(inp, target, tables, C: int, background: bool = False):
    """-> (inp', target', sel uint8 [B,H,W], pasted int32 [B]) on the CPU"""
    inp, target = inp.cpu(), target.cpu()
    sel = sel_ref(target, tables, C, background)
    d = tables["donor"].long()
    m = sel.bool()
    # bits, not values: a NaN payload is copied as it is
    out = torch.where(m.unsqueeze(1), inp.view(torch.int32)[d], inp.view(torch.int32)).view(torch.float32)
    return out, torch.where(m, target[d], target), sel, sel.sum(dim=(1, 2), dtype=torch.int32)


def mixed_maps(teachers, flips, size, sel, donor, dtype=torch.float64):
    """every teacher map at (H, W), un-mirrored, gathered from donor[b] where sel: NHWC [B,H,W,C] in ``dtype``"""
    size = _size(size)
    flips = [False] * len(teachers) if flips is None else list(flips)
    d = torch.as_tensor(donor).long()
    m = sel.cpu().bool().unsqueeze(1)
    out = []
    for t, f in zip(teachers, flips):
        t = t.detach().cpu().to(dtype)
        r = _resized(t.flip(2) if f else t, size)
        out.append(torch.where(m, r[d], r).permute(0, 2, 3, 1).contiguous())
    return out


def mixed_confidence(teachers, flips, size, T, sel, donor, dtype=torch.float64) -> torch.Tensor:
    """conf [B,H,W] = max_c q_c of the mixed soft targets"""
    maps = mixed_maps(teachers, flips, size, sel, donor, dtype)
    q = sum(torch.softmax(m.permute(0, 3, 1, 2) / T, dim=1) for m in maps) / len(maps)
    return q.amax(dim=1)


def mixed_consist_ref(student, teachers, flips, size, T, sel, donor, threshold=None, sample_weight=None, dtype=torch.float64, gate=None):
    """``consist_ref`` over the mixed batch (its namespace)"""
    maps = mixed_maps(teachers, flips, size, sel, donor, dtype)
    return consist_ref(student, maps, [False] * len(maps), size, T, threshold, sample_weight, dtype, gate)
