"""Class-adaptive confidence thresholds (SegEngine distill_class_thresholds=, ops.consistency_loss(class_threshold=),
ops.confidence_stats, ops.adaptive_threshold_update, csrc/adapt.hip): what the threshold per class and its statistics cost.
    a. op        ops.consistency_loss with class_threshold = full(C, t) against the same call with threshold = t (the yardstick, the
                 same gate decisions) added into dz, at 12 x 588^2 with C = 2 and C = 8, one and two teacher maps; the yardstick is
                 timed as two arms, so that their difference is the run-to-run spread of the same run.  Then ops.confidence_stats +
                 ops.adaptive_threshold_update on the same maps: the time against the loss call's, and the bytes it must move (the
                 teacher maps once) over the time against the 6.29 TB/s the project takes as the stream rate.
    b. step      SegEngine.train_step at the config-3 geometry (ViT-L/14, 588^2, train_adapters) with the EMA teacher: the scalar
                 gate against distill_class_thresholds="adaptive".
    c. default   --plain_only: the default step (no new keyword) alone, every window printed: scripts/bench_mix.py's arm of that
                 name, the form to run alternately in this tree and in the parent commit's, each in its own process.
    python scripts/bench_adapt.py [--part a|b|ab] [--plain_only]
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

from bench_hardpixel import head_size     # scripts/ is on the path when this file is run
from bench_mean_teacher import _engine, _fmt, _interleaved, _shape

STREAM_TBS = 6.29


def op_part(a):
    from adaptersis_amd import ops
    dev = torch.device("cuda:0")
    T = a.temperature
    print(f"a. us per call, median (min..max) of {a.reps} windows of {a.iters} calls; T = {T:g}, threshold {a.threshold:g}; "
          f"GB/s = the teacher maps' bytes / the median")
    print(f"{'shape':>16s} {'logits':>9s} {'V':>2s} {'arm':>22s} {'us':>24s} {'vs scalar':>9s} {'MB':>6s} {'GB/s':>6s} {'of stream':>9s}")
    for B, S, C in a.shapes:
        h, w = head_size(S, C, dev)
        g = torch.Generator().manual_seed(S + C)
        student = (2.0 * torch.randn((B, h, w, C), generator=g)).to(dev)
        maps = [(2.0 * torch.randn((B, h, w, C), generator=g)).to(dev) for _ in range(2)]
        dz = torch.zeros((B, S, S, C), device=dev)
        full = torch.full((C,), a.threshold, device=dev)
        lscr = torch.empty(ops.consistency_scratch_bytes(B * S * S), device=dev, dtype=torch.uint8)
        sscr = torch.empty(ops.confidence_stats_scratch_bytes(B * S * S), device=dev, dtype=torch.uint8)
        sums = torch.empty(C + 2, device=dev, dtype=torch.float64)
        state = torch.tensor([1.0 / C, 0.0] + [1.0 / C] * C, dtype=torch.float64, device=dev)
        thr = torch.empty(C, device=dev)
        for V in (1, 2):
            ts, fl = maps[:V], [False, True][:V]
            kw = dict(flips=fl, temperature=T, dz=dz, scratch=lscr)
            scalar = lambda: ops.consistency_loss(student, ts, (S, S), threshold=a.threshold, **kw)

            def stats():
                ops.confidence_stats(ts, (S, S), flips=fl, temperature=T, out=sums, scratch=sscr)
                ops.adaptive_threshold_update(sums, state, thr, 0.999)

            forms = {"scalar threshold": scalar, "scalar threshold again": scalar,
                     "class thresholds": lambda: ops.consistency_loss(student, ts, (S, S), class_threshold=full, **kw),
                     "stats + update": stats}
            ka, kb = scalar()[1], forms["class thresholds"]()[1]
            assert torch.equal(ka, kb), "equal thresholds: the kept count differs from the scalar gate's"
            times = _interleaved(forms, a.reps, a.iters, scale=1e3)
            med = {k: statistics.median(v) for k, v in times.items()}
            mbytes = V * B * h * w * C * 4
            for k in forms:
                tail = ""
                if k == "stats + update":
                    gbs = mbytes / med[k] / 1e3
                    tail = f" {mbytes / 1e6:6.1f} {gbs:6.0f} {gbs / (STREAM_TBS * 1e3):9.2%}"
                print(f"{f'{B}x{S}x{S} C={C}':>16s} {h:4d}x{w:<4d} {V:2d} {k:>22s} {_fmt(times[k]):>24s} {med[k] / med['scalar threshold']:9.3f}"
                      + tail, flush=True)
            print(f"{'':>16s} kept {int(ka) / (B * S * S):.1%}; thresholds after the updates {[round(v, 4) for v in thr.tolist()]}", flush=True)
        del student, maps, dz
        torch.cuda.empty_cache()


def step_part(a):
    from bench import synthetic
    dev = torch.device("cuda:0")
    img, tgt = synthetic(a.batch, a.imsize, 0, dev)
    ema = dict(teacher="ema", ema_decay=0.999)
    arms = {"scalar threshold": dict(distill_threshold=a.threshold, **ema), "scalar threshold again": dict(distill_threshold=a.threshold, **ema),
            "adaptive thresholds": dict(distill_class_thresholds="adaptive", **ema)}
    print(f"b. ms per train_step, {a.arch} {a.imsize}^2 B={a.batch} train_adapters, EMA teacher, median (min..max) of {a.reps} windows of "
          f"{a.steps} steps")
    engines = {k: _engine(a, dev, **kw) for k, kw in arms.items()}
    forms = {k: (lambda e=e: e.train_step(img, tgt)) for k, e in engines.items()}
    times = _interleaved(forms, a.reps, a.steps, warm=a.warmup)
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, ts in times.items():
        print(f"   {k:>24s} {_fmt(ts, 2):>24s} {med[k] / med['scalar threshold']:7.4f}", flush=True)
    for k, e in engines.items():
        assert e.optimizer.skipped_steps == 0, (k, e.optimizer.skipped_steps)
    ad = engines["adaptive thresholds"]
    print(f"   adaptive: tau {float(ad.adaptive.state[0]):.4f} after {int(ad.adaptive.state[1])} updates, thresholds "
          f"{[round(v, 4) for v in ad.class_thresholds.tolist()]}, kept {int(ad.last_kd_kept) / tgt.numel():.1%} "
          f"(scalar gate: {int(engines['scalar threshold'].last_kd_kept) / tgt.numel():.1%}); synthetic weights: no statement about accuracy")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    ap.add_argument("--plain_only", action="store_true", help="the default step alone (B = --batch), every window printed")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3, help="part a: calls per window")
    ap.add_argument("--steps", type=int, default=3, help="part b: training steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=_shape, nargs="+", default=[(12, 588, 8), (12, 588, 2)], help="part a: batch,imsize,classes")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--threshold", type=float, default=0.6, help="the scalar gate (part a: also every class threshold)")
    ap.add_argument("--arch", default="vit_large")
    ap.add_argument("--imsize", type=int, default=588)
    ap.add_argument("--batch", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_adapt.py measures on an MI355X: no device found")
    if args.plain_only:
        import bench_mix
        bench_mix.step_part(args)
    else:
        if "a" in args.part:
            op_part(args)
        if "b" in args.part:
            step_part(args)
