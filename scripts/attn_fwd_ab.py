"""Attention forward, speculative order against max-first (ASIS_ATTN_MAXFIRST=1) on peaked scores: python scripts/attn_fwd_ab.py
[--trunk].  The trunk's launch shape (segments (12, 1765) and (12, 1764), 16 heads, folded form), Gaussian q and k scaled so
that the scores have a standard deviation of 0.5, 2, 5 and 10 in log2 units; each form timed with events around 20 calls after
a warm-up, 5 repeats, the two forms alternating.  Beside the times: the share of key tiles that take the fast path, the slow
path without a rescale, and the rescale, from a torch emulation of the kernel's wave-level decision on the same q and k
(``emulate_decision``; tests/test_gpu_attn_fwd_order.py runs it on the CPU).  --trunk: the same shares on the q | k of three
trunk blocks of one bench-shaped step (profiles/attn_fwd_rowmax_ab.txt holds both tables)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

KT, RESCALE_THR = 64, 6.0
SUM_FAST = 0.75 * 2.0 ** RESCALE_THR
C_FOLD = 0.125 * 1.4426950408889634


def emulate_decision(q: torch.Tensor, k: torch.Tensor) -> dict:
    """q, k: float [B, H, N, 64], the 16-bit operands of the folded kernel (q . k is a score in log2 units).  Walks the key
    tiles between the first and the last one as attn_fwd_pipe_kernel does: a wave is 32 consecutive queries, the two lanes of a
    query hold the keys with bit 3 clear / set, the running maximum is the first tile's and moves only in a wave that rescales
    (there by every lane whose tile maximum is above it).  Counts, per wave and tile: ``fast`` (every lane's partial row sum
    below 0.75 * 2^6), ``slow`` (not fast, no row maximum more than 6 above the running one), ``rescale`` (not fast, some
    row maximum is), and ``unsound`` (the sum test passes although the max-first order would rescale: must be 0)."""
    B, H, N, _ = q.shape
    nt, nw = (N + KT - 1) // KT, (N + 31) // 32
    if nw * 32 != N:  # a partial wave repeats the last query
        q = torch.cat([q, q[:, :, -1:].expand(B, H, nw * 32 - N, 64)], 2)
    q, k = q.float(), k.float()
    hi = ((torch.arange(KT, device=q.device) >> 3) & 1).bool()
    m = (q @ k[:, :, :KT].transpose(-1, -2)).amax(-1)
    c = dict(tiles=0, fast=0, slow=0, rescale=0, unsound=0)
    for t in range(1, nt - 1):
        s = q @ k[:, :, t * KT:(t + 1) * KT].transpose(-1, -2) - m[..., None]
        p = torch.exp2(s)
        sums = torch.stack([p[..., ~hi].sum(-1), p[..., hi].sum(-1)], -1)
        fast = (sums < SUM_FAST).reshape(B, H, nw, 64).all(-1)
        mx = s.amax(-1)
        today = (mx > RESCALE_THR).reshape(B, H, nw, 32).any(-1)
        c["tiles"] += fast.numel()
        c["fast"] += int(fast.sum())
        c["slow"] += int((~fast & ~today).sum())
        c["rescale"] += int((~fast & today).sum())
        c["unsound"] += int((fast & today).sum())
        m = torch.where(today.repeat_interleave(32, -1), torch.maximum(m, m + mx), m)
    return c


def shares(c: dict) -> str:
    n = max(c["tiles"], 1)
    return (f"fast {100 * c['fast'] / n:6.2f} %  slow, no rescale {100 * c['slow'] / n:6.2f} %  rescale {100 * c['rescale'] / n:6.2f} %"
            f"  unsound {c['unsound']}")


def add(a: dict, b: dict) -> dict:
    return {k: a[k] + b[k] for k in a}


def time_form(f, maxfirst: bool, calls: int = 20) -> float:
    os.environ["ASIS_ATTN_MAXFIRST"] = "1" if maxfirst else "0"
    for _ in range(3):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3


def gaussian_ab(dev):
    from adaptersis_amd import ops
    H, D, dt = 16, 1024, torch.float16
    segs = [(12, 1765), (12, 1764)]
    (B1, N1), (B2, N2) = segs
    R = B1 * N1 + B2 * N2
    print(f"{'sigma':>5s} | {'max-first us (min med max)':>28s} | {'speculative us (min med max)':>28s} | med ratio | equal | shares of tiles 1 .. nt-2")
    for sigma in (0.5, 2.0, 5.0, 10.0):
        g = torch.Generator(device="cpu").manual_seed(1234)
        a = (sigma / 8.0) ** 0.5  # q . k over 64 unit Gaussians has deviation 8
        qk = (torch.randn(R, 2 * D, generator=g) * a).to(dev).to(dt)
        v = torch.randn(R, D, generator=g).to(dev).to(dt)
        vt = torch.zeros((B1 + B2, D, 1792), device=dev, dtype=dt)
        vt[:B1, :, :N1] = v[:B1 * N1].view(B1, N1, D).transpose(1, 2)
        vt[B1:, :, :N2] = v[B1 * N1:].view(B2, N2, D).transpose(1, 2)
        o, o_lo = torch.empty(R, D, device=dev, dtype=dt), torch.empty(R, D, device=dev, dtype=dt)
        f = lambda: ops.attention_fwd_seg(qk[:, :D], qk[:, D:], vt, B1, N1, B2, N2, H, None, out=o, out_lo=o_lo)
        ts = {True: [], False: []}
        for _ in range(5):
            for mf in (True, False):
                ts[mf].append(time_form(f, mf))
        os.environ["ASIS_ATTN_MAXFIRST"] = "1"
        f()
        ref, ref_lo = o.clone(), o_lo.clone()
        os.environ["ASIS_ATTN_MAXFIRST"] = "0"
        f()
        same = torch.equal(o, ref) and torch.equal(o_lo, ref_lo)
        c = None
        r0 = 0
        for B, N in segs:
            for b in range(B):  # one image at a time: a tile of scores of all of them would not fit beside the rest
                rows = qk[r0 + b * N:r0 + (b + 1) * N]
                ci = emulate_decision(rows[:, :D].view(1, N, H, 64).transpose(1, 2), rows[:, D:].view(1, N, H, 64).transpose(1, 2))
                c = ci if c is None else add(c, ci)
            r0 += B * N
        old, new = sorted(ts[True]), sorted(ts[False])
        print(f"{sigma:5.1f} | {old[0]:8.1f} {old[2]:8.1f} {old[-1]:8.1f}   | {new[0]:8.1f} {new[2]:8.1f} {new[-1]:8.1f}   | {new[2] / old[2]:9.3f} | {str(same):5s} | {shares(c)}")


def trunk_shares(dev):
    """the q | k that three trunk blocks hand to the kernel in one bench-shaped step (ViT-L/14, 12 images of 588^2)"""
    import bench
    from adaptersis_amd import ops
    eng = bench.build_engine("vit_large", dev, lr=0.01)
    img, tgt = bench.synthetic(12, 588, 0, dev)
    seen, launch = [], ops.attention_fwd_seg

    def hook(q, k, vt, B1, N1, B2, N2, H, scale, out, out_lo=None):
        seen.append((q.clone(), k.clone(), (B1, N1), (B2, N2), H, scale))
        return launch(q, k, vt, B1, N1, B2, N2, H, scale, out, out_lo)

    ops.attention_fwd_seg = hook
    try:
        eng.train_step(img, tgt)
        torch.cuda.synchronize()
    finally:
        ops.attention_fwd_seg = launch
    print(f"{len(seen)} stacked attention launches in the step")
    for i in (0, len(seen) // 2, len(seen) - 1):
        q, k, s1, s2, H, scale = seen[i]
        if scale is not None:
            q = q.float() * (scale * 1.4426950408889634)
        c, r0 = None, 0
        for B, N in (s1, s2):
            for b in range(B):
                sl = slice(r0 + b * N, r0 + (b + 1) * N)
                ci = emulate_decision(q[sl].reshape(1, N, H, 64).transpose(1, 2), k[sl].reshape(1, N, H, 64).transpose(1, 2))
                c = ci if c is None else add(c, ci)
            r0 += B * N
        N = s1[1]
        sd = float((q[:N].reshape(N, H, 64).transpose(0, 1).float() @ k[:N].reshape(N, H, 64).transpose(0, 1).float().transpose(1, 2)).std())
        print(f"launch {i:2d}: score deviation {sd:5.2f} (log2 units, first image)  {shares(c)}")


def main():
    dev = torch.device("cuda:0")
    print(torch.cuda.get_device_name(0))
    if "--trunk" in sys.argv[1:]:
        trunk_shares(dev)
    else:
        gaussian_ab(dev)


if __name__ == "__main__":
    main()
