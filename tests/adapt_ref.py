"""Restatement of the class-adaptive confidence thresholds of csrc/adapt.hip in plain torch and plain Python, on top of
tests/consist_ref.py and tests/distill_ref.py (float64; the loss is also evaluated in float32 on the CPU for the yardstick Y of
tests/bound_helpers.py).  With q the teacher's mean distribution at a pixel (``distill_ref.soft_targets``):

    a_i = argmax_c q_i[c], the lowest index among equal values;  conf_i = q_i[a_i];  m_i = [conf_i >= thr[a_i]]
    loss, kept, dz: those of ``consist_ref`` under that gate
    S_c = sum_i q_i[c],  S_conf = sum_i conf_i,  cnt = the pixels i, over the samples with w_b > 0 (each pixel counts 1)
    state = tau, n_updates, ptilde[C], from tau = ptilde_c = 1 / C;  with cnt > 0:
        tau <- l tau + (1 - l) S_conf / cnt,  ptilde_c <- l ptilde_c + (1 - l) S_c / cnt,  n_updates += 1
        thr_c = fp32(tau ptilde_c / max_c ptilde_c)
    with cnt == 0 nothing changes
"""
import torch

from tests.consist_ref import consist_ref
from tests.distill_ref import _size, soft_targets


def soft_q(teachers, flips, size, T, dtype=torch.float64) -> torch.Tensor:
    """q, NCHW [B,C,H,W]"""
    flips = [False] * len(teachers) if flips is None else list(flips)
    return soft_targets(teachers, flips, _size(size), T, dtype)


def top_class(q: torch.Tensor):
    """-> (a [B,H,W] int64: the lowest index of the largest q_c, conf [B,H,W])"""
    C = q.shape[1]
    conf = q.amax(dim=1)
    idx = torch.arange(C).view(1, C, 1, 1).expand_as(q)
    a = torch.where(q == conf.unsqueeze(1), idx, torch.full_like(idx, C)).amin(dim=1)
    return a, conf


def class_gate(q: torch.Tensor, thr) -> torch.Tensor:
    """m [B,H,W] bool.  ``thr``: C values (the fp32 values the device is given, compared in q's type)"""
    a, conf = top_class(q)
    t = torch.as_tensor(thr).to(q.dtype)
    return conf >= t[a]


def adapt_consist_ref(student, teachers, flips, size, T, thr, sample_weight=None, dtype=torch.float64, gate=None):
    """``consist_ref`` under the class gate (its namespace, plus ``a``: the top class in float64).  ``gate``: a bool [B,H,W] to
    use instead (the float32 yardstick takes the float64 gate)."""
    q64 = soft_q(teachers, flips, size, T)
    a, _ = top_class(q64)
    if gate is None:
        gate = class_gate(q64, thr)
    ref = consist_ref(student, teachers, flips, size, T, None, sample_weight, dtype, gate=gate)
    ref.a = a
    return ref


def stats_ref(teachers, flips, size, T, sample_weight=None, dtype=torch.float64) -> torch.Tensor:
    """sums [C + 2] in ``dtype`` = S_0..S_{C-1}, S_conf, cnt"""
    if sample_weight is None:
        keep = list(range(teachers[0].shape[0]))
    else:
        keep = [b for b, w in enumerate(sample_weight.tolist()) if w > 0]
    C = teachers[0].shape[-1]
    if not keep:
        return torch.zeros(C + 2, dtype=dtype)
    q = soft_q([t[keep] for t in teachers], flips, size, T, dtype)
    conf = q.amax(dim=1)
    return torch.cat([q.sum(dim=(0, 2, 3)), conf.sum().view(1), torch.tensor([float(conf.numel())], dtype=dtype)])


def init_state(C: int):
    """tau, n_updates, ptilde[C] as Python floats"""
    return [1.0 / C, 0.0] + [1.0 / C] * C


def thresholds_of(state):
    """thr [C] fp32 of a state"""
    tau, pt = state[0], state[2:]
    mx = max(pt)
    return torch.tensor([tau * p / mx for p in pt], dtype=torch.float64).to(torch.float32)


def update_ref(state, sums, lam: float = 0.999):
    """one step in Python floats (float64) -> (state, thr fp32 [C]); cnt == 0: the state as it was and None"""
    sums = [float(v) for v in sums]
    C = len(state) - 2
    cnt = sums[C + 1]
    if not cnt > 0:
        return list(state), None
    tau = lam * state[0] + (1.0 - lam) * (sums[C] / cnt)
    pt = [lam * state[2 + c] + (1.0 - lam) * (sums[c] / cnt) for c in range(C)]
    new = [tau, state[1] + 1.0] + pt
    return new, thresholds_of(new)


def _top_two(q: torch.Tensor):
    """-> (v1, v2, a1, a2) [B,H,W]: the two largest q_c and their classes (a1 the lowest index among equal values; C = 1: v2 = 0)"""
    a1, v1 = top_class(q)
    if q.shape[1] == 1:
        return v1, torch.zeros_like(v1), a1, a1
    rest = q.scatter(1, a1.unsqueeze(1), -1.0)
    a2, v2 = top_class(rest)
    return v1, v2, a1, a2


def near_pixels(q: torch.Tensor, thr, delta: float) -> torch.Tensor:
    """bool [B,H,W]: pixels a float32 evaluation may gate either way: the confidence lies within ``delta`` of its class threshold,
    or the top two lie within ``delta`` and their classes decide differently"""
    t = torch.as_tensor(thr).to(q.dtype)
    v1, v2, a1, a2 = _top_two(q)
    close = (v1 - t[a1]).abs() <= delta
    tie = ((v1 - v2) <= delta) & ((v1 >= t[a1]) != (v2 >= t[a2]))
    return close | tie


def pick_class_thresholds(q: torch.Tensor, delta: float = 1e-5):
    """Thresholds no pixel is near.  Classes joined by a pixel whose top two q lie within ``delta`` form a group (union-find); a
    group gets one threshold: the midpoint of the widest gap of at least 4 delta between the sorted confidences of its pixels, with
    0 and 1 as end points, among the gaps that keep 10..90 % of the group where there is one.  Rounded to float32 (what the device
    is given).  -> (thr fp32 [C], note)"""
    C = q.shape[1]
    parent = list(range(C))

    def find(c):
        while parent[c] != c:
            parent[c] = parent[parent[c]]
            c = parent[c]
        return c

    v1, v2, a1, a2 = _top_two(q)
    tied = (v1 - v2) <= delta
    for x, y in set(zip(a1[tied].tolist(), a2[tied].tolist())):
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)
    thr = torch.zeros(C, dtype=torch.float64)
    notes = []
    for root in sorted({find(c) for c in range(C)}):
        members = [c for c in range(C) if find(c) == root]
        inside = torch.zeros_like(a1, dtype=torch.bool)
        for c in members:
            inside |= a1 == c
        conf = v1[inside].flatten().sort().values
        n = conf.numel()
        ext = torch.cat([torch.zeros(1, dtype=torch.float64), conf.double(), torch.ones(1, dtype=torch.float64)])
        gaps = ext[1:] - ext[:-1]                                     # gap j: j pixels lie below it, n - j are kept
        wide = gaps >= 4 * delta
        if not bool(wide.any()):
            raise AssertionError(f"classes {members}: no gap of {4 * delta} between the confidences")
        share = (n - torch.arange(n + 1, dtype=torch.float64)) / max(n, 1)
        mid = wide & (share >= 0.1) & (share <= 0.9)
        pool = mid if bool(mid.any()) else wide
        j = int(torch.where(pool, gaps, torch.full_like(gaps, -1.0)).argmax())
        t = float(torch.tensor((float(ext[j]) + float(ext[j + 1])) / 2, dtype=torch.float32))
        for c in members:
            thr[c] = t
        notes.append(f"{members}: {t:.4f} keeps {float(share[j]):.2f} of {n}")
    return thr.to(torch.float32), "; ".join(notes)


def middle_class_thresholds(q: torch.Tensor):
    """the large cases: per class the midpoint of the two middle confidences of its pixels (0.5 for a class without two pixels),
    rounded to float32"""
    a, conf = top_class(q)
    thr = torch.full((q.shape[1],), 0.5, dtype=torch.float64)
    for c in range(q.shape[1]):
        v = conf[a == c].flatten().sort().values
        if v.numel() >= 2:
            m = v.numel() // 2
            thr[c] = (float(v[m - 1]) + float(v[m])) / 2
    return thr.to(torch.float32)
