"""The weight average (optim.EMA, csrc/ema.hip): what the update costs, alone and inside the training step.
    a. kernels   ops.ema_prepare + ops.ema_update on one buffer against torch.Tensor.lerp_ on the same buffers, interleaved: the
                 size of config 3's trainable bucket (15.7 M fp32, 62.8 MB) and of the ViT-L backbone bucket (304 M).  The bytes:
                 12 per element (e and p read, e written); the rate next to the float4-copy rate of this chip that DESIGN.md
                 quotes (6.29 TB/s).  lerp_ has neither the guard nor the device-side schedule: it is the yardstick, not a substitute.
    b. step      SegEngine.train_step at the config-3 geometry (ViT-L/14, 588^2, B = 12, train_adapters) with ema_decay set and
                 unset, two engines alternating in one process; the overhead next to the run-to-run spread of the unset arm.
    python scripts/bench_ema.py [--part a|b|ab]
Medians of --reps timed windows (device events) after a warm-up of every arm, the arms alternating and their order reversed every
window; min and max beside each median.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from bench_hardpixel import window     # scripts/ is on the path when this file is run

STREAM_TBS = 6.29
SIZES = [("config-3 trainable bucket", 15_700_000), ("ViT-L backbone bucket", 304_000_000)]


def _stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def kernel_part(a):
    from adaptersis_amd import ops
    dev = torch.device("cuda:0")
    print(f"a. us per update, median (min..max) of {a.reps} windows of {a.iters} calls")
    print(f"{'buffer':>28s} {'elements':>11s} {'ema':>22s} {'lerp_':>22s} {'ema/lerp_':>9s} {'ema GB/s':>9s} {'of stream':>9s}")
    for name, n in SIZES:
        g = torch.Generator().manual_seed(n % 1000)
        e0 = torch.randn(n, generator=g)
        ed, ld, pd = e0.to(dev), e0.to(dev), torch.randn(n, generator=g).to(dev)
        state = torch.zeros(1, device=dev, dtype=torch.int32)
        rec = torch.zeros(2, device=dev, dtype=torch.float32)
        w = 1.0 - 0.999

        def ema():
            ops.ema_prepare(None, state, rec, 0.999, False)
            ops.ema_update(ed, pd, rec)

        def lerp():
            ld.lerp_(pd, w)

        forms = [ema, lerp]
        for f in forms:
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        times = {f.__name__: [] for f in forms}
        for r in range(a.reps):
            for f in (forms if r % 2 == 0 else forms[::-1]):
                times[f.__name__].append(window(f, a.iters) * 1e3)
        (me, lo_e, hi_e), (ml, lo_l, hi_l) = _stats(times["ema"]), _stats(times["lerp"])
        rate = 12.0 * n / (me * 1e-6) / 1e9
        print(f"{name:>28s} {n:11d} {f'{me:.1f} ({lo_e:.1f}..{hi_e:.1f})':>22s} {f'{ml:.1f} ({lo_l:.1f}..{hi_l:.1f})':>22s} "
              f"{me / ml:9.2f} {rate:9.0f} {rate / (STREAM_TBS * 1e3):9.2f}", flush=True)
        del ed, ld, pd
        torch.cuda.empty_cache()


def step_part(a):
    from adaptersis_amd.backbones.engines import make_ema
    from bench import build_engine, synthetic      # the repository root is on the path
    dev = torch.device("cuda:0")
    img, tgt = synthetic(a.batch, a.imsize, 0, dev)
    arms = {}
    for name in ("unset", "set"):
        eng = build_engine(a.arch, dev, lr=0.01, mode="train_adapters")
        if name == "set":
            eng.ema = make_ema(eng.optimizer, 0.999, True)
        eng.seg_decoder.train()
        arms[name] = eng
    averaged = sum(b.numel for b in arms["set"].ema.buckets)
    for eng in arms.values():
        for _ in range(a.warmup):
            eng.train_step(img, tgt)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    order = list(arms)
    for r in range(a.reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k].append(window(lambda: arms[k].train_step(img, tgt), a.steps))
    (mu, lo_u, hi_u), (ms, lo_s, hi_s) = _stats(times["unset"]), _stats(times["set"])
    print(f"b. ms per train_step, {a.arch} {a.imsize}^2 B={a.batch} train_adapters, median (min..max) of {a.reps} windows of "
          f"{a.steps} steps; {averaged} averaged elements")
    print(f"   ema_decay unset {mu:.2f} ({lo_u:.2f}..{hi_u:.2f})   set {ms:.2f} ({lo_s:.2f}..{hi_s:.2f})   "
          f"overhead {ms - mu:+.3f} ms = {100.0 * (ms - mu) / mu:+.2f} %   spread of the unset arm {hi_u - lo_u:.3f} ms", flush=True)
    assert arms["set"].ema.updates + arms["set"].optimizer.skipped_steps == a.warmup + a.reps * a.steps


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20, help="part a: updates per window")
    ap.add_argument("--steps", type=int, default=3, help="part b: training steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arch", default="vit_large")
    ap.add_argument("--imsize", type=int, default=588)
    ap.add_argument("--batch", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ema.py measures on an MI355X: no device found")
    if "a" in args.part:
        kernel_part(args)
    if "b" in args.part:
        step_part(args)
