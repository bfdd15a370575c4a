"""Fused AdamW on one flat bucket: byte rates of grad_sumsq (4 B / parameter) and adamw_step (28.25 B: p, m, v read and written, g
read, one group code per 4 parameters) at the decoder, adapter and ViT-L bucket sizes; in the same process the SGD kernel
(20 B) and its guard (4 B) as the yardstick, and torch's AdamW(fused=True) + clip_grad_norm_ on the same flat tensors.
    python scripts/bench_adamw.py [n_params ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from adaptersis_amd import ops
dev = torch.device("cuda:0")
SIZES = {"decoder": 15_700_000, "adapters": 7_800_000, "vit_large": 304_000_000}   # FeatureDecoder / CAViT + CACNN / ViT-L buckets
sizes = {str(int(a)): int(a) for a in sys.argv[1:]} or SIZES


def timed(f, reps=10):
    for _ in range(3):
        f()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        f()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


for name, n in sizes.items():
    n = n // 4 * 4
    p, g, m, v = (torch.rand(n, device=dev) for _ in range(4))
    codes = (torch.arange(n // 4, device=dev) % 3).to(torch.uint8)
    lr_scale = torch.tensor([1.0, 0.5, 0.25], device=dev)
    wd = torch.tensor([0.05, 0.0, 0.1], device=dev)
    partials = torch.zeros(ops.grad_sumsq_blocks(n), device=dev)
    guard3, rec = torch.zeros(3, device=dev, dtype=torch.int32), torch.zeros(4, device=dev)
    guard2 = torch.zeros(2, device=dev, dtype=torch.int32)

    def adamw_all():
        ops.grad_sumsq(g, partials)
        ops.adamw_prepare(partials, guard3, rec, 1.0, 1.0, 0.9, 0.999)
        ops.adamw_step(p, g, m, v, codes, lr_scale, wd, 1e-3, 0.9, 0.999, 1e-8, 1.0, guard3, rec)

    def sgd_all():
        ops.grad_guard(g, guard2, True)
        ops.sgd_momentum(p, g, m, 1e-3, 0.9, 1e-5, 1.0, False, guard2)

    rows = ((lambda: ops.grad_guard(g, guard2, True), "guard", 4.0 * n),
            (lambda: ops.sgd_momentum(p, g, m, 1e-3, 0.9, 1e-5, 1.0, False, guard2), "sgd", 20.0 * n),
            (sgd_all, "guard+sgd", 24.0 * n),
            (lambda: ops.grad_sumsq(g, partials), "grad_sumsq", 4.0 * n),
            (lambda: ops.adamw_prepare(partials, guard3, rec, 1.0, 1.0, 0.9, 0.999), "adamw_prepare", 0.0),
            (lambda: ops.adamw_step(p, g, m, v, codes, lr_scale, wd, 1e-3, 0.9, 0.999, 1e-8, 1.0, guard3, rec), "adamw_step", 28.25 * n),
            (adamw_all, "adamw step, all 3", 32.25 * n))
    for f, what, nbytes in rows:
        us = timed(f)
        print(f"{name:10s} n={n:>11d} {what:18s}: {us:8.1f} us" + (f"  {nbytes / us / 1e6:6.2f} TB/s" if nbytes else ""), flush=True)
    assert int(guard3[1]) == 0 and int(guard2[1]) == 0, "a benchmark step was skipped"
    # torch on the same flat tensors: one parameter = the whole bucket
    tp = torch.nn.Parameter(p.clone())
    tp.grad = g.clone()
    topt = torch.optim.AdamW([tp], lr=1e-3, weight_decay=0.05, fused=True)
    us_clip = timed(lambda: torch.nn.utils.clip_grad_norm_([tp], 1.0))
    us_step = timed(topt.step)
    print(f"{name:10s} n={n:>11d} torch clip_grad_norm_ {us_clip:8.1f} us + AdamW(fused=True) {us_step:8.1f} us = {us_clip + us_step:8.1f} us",
          flush=True)
    del p, g, m, v, tp, topt, codes, partials
    torch.cuda.empty_cache()
