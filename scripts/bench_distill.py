"""The distillation loss (ops.distill_loss, csrc/distill.hip) against the torch composition a user would write without it.
Per shape, number of teacher maps V and form, interleaved in one process:
    fused      ops.distill_loss: loss and dz at the target's size, scratch reused ("acc": added into a given dz)
    composed   per map F.interpolate(bilinear) -> softmax(/T), their mean; F.interpolate of the student -> log_softmax(/T);
               T^2 F.kl_div(reduction="sum") / N; autograd backward to the [B,C,H,W] gradient ("acc": added into a given buffer)
    python scripts/bench_distill.py                # 12 x 588^2 with C = 8 and C = 2, V = 1 and V = 2 (the second map mirrored)
The (h, w) of the logits are read off the heads as in scripts/bench_hardpixel.py.  Medians of --reps timed windows of --iters calls
each (device events), after a warm-up of every form, the forms alternating and their order reversed every window.  The fused
arm's bytes: dz written once (read once more when it is added into) plus the maps read once; the rate next to the float4-copy
rate of this chip that DESIGN.md quotes (6.29 TB/s).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

from bench_hardpixel import head_size, window     # scripts/ is on the path when this file is run

STREAM_TBS = 6.29


def kernel_part(a):
    from adaptersis_amd import ops
    dev = torch.device("cuda:0")
    T = a.temperature
    print(f"us per call, median of {a.reps} windows of {a.iters} calls; T = {T:g}")
    print(f"{'shape':>16s} {'logits':>9s} {'V':>2s} {'dz':>6s} {'fused':>9s} {'composed':>9s} {'ratio':>6s} {'fused GB/s':>11s} {'of stream':>10s}"
          "   fused min..max   |loss diff|")
    for B, S, C in a.shapes:
        h, w = head_size(S, C, dev)
        g = torch.Generator().manual_seed(S + C)
        student = (2.0 * torch.randn((B, h, w, C), generator=g)).to(dev)
        maps = [(2.0 * torch.randn((B, h, w, C), generator=g)).to(dev) for _ in range(2)]
        N = B * S * S
        scratch = torch.empty(ops.distill_scratch_bytes(N), device=dev, dtype=torch.uint8)
        base = torch.randn((B, S, S, C), generator=g).to(dev)
        base_nchw = base.permute(0, 3, 1, 2).contiguous()
        s_nchw = student.permute(0, 3, 1, 2).contiguous()
        for V in (1, 2):
            ts, flips = maps[:V], [False, True][:V]
            t_nchw = [(t.flip(2) if f else t).permute(0, 3, 1, 2).contiguous() for t, f in zip(ts, flips)]
            for acc in (False, True):
                buf_f, buf_c = base.clone(), base_nchw.clone()

                def fused():
                    return ops.distill_loss(student, ts, (S, S), flips=flips, temperature=T, dz=buf_f if acc else None, scratch=scratch)

                def composed():
                    lg = s_nchw.detach().requires_grad_(True)
                    with torch.no_grad():
                        q = sum(torch.softmax(F.interpolate(t, size=(S, S), mode="bilinear", align_corners=False) / T, 1) for t in t_nchw)
                        q = q / V
                    z = F.interpolate(lg, size=(S, S), mode="bilinear", align_corners=False)
                    z.retain_grad()
                    loss = (T * T / N) * F.kl_div(torch.log_softmax(z / T, 1), q, reduction="sum")
                    loss.backward()
                    return loss, (buf_c.add_(z.grad) if acc else z.grad)

                forms = [fused, composed]
                for f in forms:
                    for _ in range(2):
                        f()
                torch.cuda.synchronize()
                times = {f.__name__: [] for f in forms}
                for r in range(a.reps):
                    for f in (forms if r % 2 == 0 else forms[::-1]):
                        times[f.__name__].append(window(f, a.iters))
                med = {k: statistics.median(v) * 1e3 for k, v in times.items()}
                diff = abs(float(fused()[0]) - float(composed()[0].detach()))
                nbytes = 4 * N * C * (2 if acc else 1) + 4 * (1 + V) * student.numel()
                rate = nbytes / (med["fused"] * 1e-6) / 1e9
                tf = [t * 1e3 for t in times["fused"]]
                print(f"{f'{B}x{S}x{S} C={C}':>16s} {h:4d}x{w:<4d} {V:2d} {'acc' if acc else 'fresh':>6s} {med['fused']:9.1f} "
                      f"{med['composed']:9.1f} {med['composed'] / med['fused']:6.1f} {rate:11.0f} {rate / (STREAM_TBS * 1e3):10.2f}   "
                      f"{min(tf):.1f}..{max(tf):.1f}   {diff:.2e}", flush=True)
        del student, maps, scratch, base, base_nchw
        torch.cuda.empty_cache()


def _shape(s):
    b, size, c = (int(x) for x in s.split(","))
    return b, size, c


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--shapes", type=_shape, nargs="+", default=[(12, 588, 8), (12, 588, 2)], help="batch,imsize,classes")
    ap.add_argument("--temperature", type=float, default=2.0)
    kernel_part(ap.parse_args())
