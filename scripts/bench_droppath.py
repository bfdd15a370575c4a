"""Stochastic depth on the config-4 stacking: forward + backward with parameter gradients of the four blocks of vit_large_d4 on
segs = [(12, 1765), (12, 1764)] at uniform rates 0, 0.1, 0.2 and 0.4 — all rates interleaved in one process after warm-up,
fresh draws every round (index tables packed and uploaded inside the timed window), device events around each pass.
Prints ms per block (median over the rounds) and the ratio to rate 0 of the same run, then the four row kernels of
csrc/droppath.hip next to the ops they stand in for, with the bytes each moves.
    python scripts/bench_droppath.py [--rounds 12] [--batch 12]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from adaptersis_amd import config, droppath, ops
from adaptersis_amd.dinov2.models import vision_transformer as vits
from adaptersis_amd.utils import weights as W

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--rates", type=float, nargs="+", default=[0.0, 0.1, 0.2, 0.4])
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_droppath needs an MI355X: there is no CPU path")
dev = torch.device("cuda:0")
config.split_attn_out = True                      # what SegEngine(train_backbone=True) runs
arch = "vit_large_d4"
D, depth, heads, ffn = W.VIT_CONFIGS[arch]
model = vits.__dict__[arch](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0)
model.load_state_dict(W.make_vit_state_dict(arch, layerscale="kernel"))
model = model.to(dev)
B = args.batch
segs = [(B, 1765), (B, 1764)]
R = sum(b * n for b, n in segs)
x = torch.randn((R, D), device=dev)
dres = torch.randn((R, D), device=dev) * 64.0
grads = {f"blocks.{i}.{k}": torch.empty_like(p, dtype=torch.float32) for i, blk in enumerate(model.blocks) for k, p in blk.named_parameters()}
samplers = {r: droppath.DropPathSampler([r] * depth, seed=0) for r in args.rates}


def one_pass(rate):
    keeps = samplers[rate].step(segs, dev) if rate > 0 else [None] * depth
    xx, saved = x, []
    for blk, kp in zip(model.blocks, keeps):
        xx, s = blk.forward_train_rows(xx, segs) if kp is None else blk.forward_train_rows(xx, segs, keep=kp)
        saved.append(s)
    d = dres
    for i in range(depth - 1, -1, -1):
        d = model.blocks[i].backward(saved[i], d, 1.0 / 64.0, grads, f"blocks.{i}")
        saved[i] = None
    return d


with torch.no_grad():
    for _ in range(2):                            # warm-up: every shape of every rate (0.1 draws a new subset size per round)
        for r in args.rates:
            one_pass(r)
    torch.cuda.synchronize()
    times = {r: [] for r in args.rates}
    for _ in range(args.rounds):
        for r in args.rates:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            one_pass(r)
            e.record()
            torch.cuda.synchronize()
            times[r].append(s.elapsed_time(e) / depth)
    base = statistics.median(times[args.rates[0]])
    print(f"{arch} segs {segs} fwd + bwd with gradients, {args.rounds} interleaved rounds, ms per block")
    for r in args.rates:
        t = sorted(times[r])
        med = statistics.median(t)
        print(f"  rate {r:4.2f}: median {med:7.3f}  min {t[0]:7.3f}  max {t[-1]:7.3f}   x{med / base:5.3f} of rate {args.rates[0]:.2f}", flush=True)

    # ---- the row kernels alone, at the subset sizes of each rate -------------------------------------------------------------
    def timed(f, reps=20):
        for _ in range(3):
            f()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            f()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / reps * 1e3

    dt = config.operand_dtype
    w, b = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    print("row kernels (us, GB moved, TB/s); full = the op of the rate-0 path on all R rows")
    rows_full = (("layernorm            full", lambda: ops.layernorm(x, w, b, 1e-6, dt), 6.0 * R * D),
                 ("cast_colsum          full", lambda: ops.cast_colsum(dres, dt), 6.0 * R * D),
                 ("layernorm_bwd        full", lambda: ops.layernorm_bwd(dres, x, w, 1e-6, res=dres), 16.0 * R * D))
    for what, f, nbytes in rows_full:
        us = timed(f)
        print(f"  {what}: {us:8.1f} us  {nbytes / 1e9:5.2f} GB  {nbytes / us / 1e6:5.2f} TB/s", flush=True)
    for r in [r for r in args.rates if r > 0.1]:
        k = droppath.keep_count(B, r)
        spec = [(list(range(k)), B / k)] * 2
        keep = droppath.pack([(spec, spec)], segs, dev)[0][0]
        Rc = keep.rows_c
        y32 = torch.randn((Rc, D), device=dev)
        rows_c = ((f"layernorm_gather      {r:.1f}", lambda: ops.layernorm_gather(x, w, b, 1e-6, dt, keep), 6.0 * Rc * D),
                  (f"scaled_index_add      {r:.1f}", lambda: ops.scaled_index_add(x, y32, keep), (8.0 * R + 4.0 * Rc) * D),
                  (f"gather_cast_colsum    {r:.1f}", lambda: ops.gather_cast_colsum(dres, dt, keep), 6.0 * Rc * D),
                  (f"layernorm_bwd_scatter {r:.1f}", lambda: ops.layernorm_bwd_scatter(y32, x, w, 1e-6, dres, keep), (8.0 * R + 8.0 * Rc) * D))
        for what, f, nbytes in rows_c:
            us = timed(f)
            print(f"  {what} (R' = {Rc} of {R}): {us:8.1f} us  {nbytes / 1e9:5.2f} GB  {nbytes / us / 1e6:5.2f} TB/s", flush=True)
