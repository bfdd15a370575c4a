"""Mean-teacher training (SegEngine teacher=, ops.consistency_loss, csrc/consist.hip): what the gated loss and the teacher cost.
    a. kernel    ops.consistency_loss against ops.distill_loss, both added into a given dz, interleaved: 12 x 588^2 (C = 8 from
                 168^2 logits, C = 2 from 672^2 — read off the heads), V = 1 and 2 teacher maps, ungated and at thresholds that keep
                 about 50 % and 10 % of the pixels (quantiles of the confidence, computed once on the device with torch).
    b. step      SegEngine.train_step at the config-3 geometry (ViT-L/14, 588^2, B = 12, train_adapters): teacher=None without and
                 with an average, the EMA teacher with one view and with two, and the time of one forward under the guard of
                 ``predict`` inside ``ema_weights()`` (what a view costs); --backbone adds the pair average / EMA teacher with
                 --optimize_backbone, where the teacher re-packs the whole averaged ViT every step.
    python scripts/bench_mean_teacher.py [--part a|b|ab] [--backbone]
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

from bench_hardpixel import head_size, window     # scripts/ is on the path when this file is run


def _stats(ts):
    return statistics.median(ts), min(ts), max(ts)


def _fmt(ts, digits=1):
    m, lo, hi = _stats(ts)
    return f"{m:.{digits}f} ({lo:.{digits}f}..{hi:.{digits}f})"


def _interleaved(forms, reps, iters, warm=2, scale=1.0):
    for f in forms.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    order = list(forms)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            times[k].append(window(forms[k], iters) * scale)
    return times


def kernel_part(a):
    from adaptersis_amd import ops
    dev = torch.device("cuda:0")
    T = a.temperature
    print(f"a. us per call added into dz, median (min..max) of {a.reps} windows of {a.iters} calls; T = {T:g}")
    print(f"{'shape':>16s} {'logits':>9s} {'V':>2s} {'distill':>20s} {'ungated':>20s} {'ratio':>6s} {'~50 % kept':>20s} {'~10 % kept':>20s}   kept shares")
    for B, S, C in a.shapes:
        h, w = head_size(S, C, dev)
        g = torch.Generator().manual_seed(S + C)
        student = (2.0 * torch.randn((B, h, w, C), generator=g)).to(dev)
        maps = [(2.0 * torch.randn((B, h, w, C), generator=g)).to(dev) for _ in range(2)]
        N = B * S * S
        sd = torch.empty(ops.distill_scratch_bytes(N), device=dev, dtype=torch.uint8)
        sc = torch.empty(ops.consistency_scratch_bytes(N), device=dev, dtype=torch.uint8)
        base = torch.randn((B, S, S, C), generator=g).to(dev)
        for V in (1, 2):
            ts, flips = maps[:V], [False, True][:V]
            # the confidences the kernel gates on, restated with torch once: their quantiles are the thresholds
            q = sum(torch.softmax(torch.nn.functional.interpolate((t.flip(2) if f else t).permute(0, 3, 1, 2), size=(S, S), mode="bilinear",
                                                                  align_corners=False) / T, 1) for t, f in zip(ts, flips)) / V
            conf = q.amax(1).flatten()
            sample = conf[torch.randint(0, conf.numel(), (1 << 20,), device=dev)]
            thr = {"~50 % kept": float(sample.quantile(0.5)), "~10 % kept": float(sample.quantile(0.9))}
            del q, conf, sample
            bufs = {k: base.clone() for k in ("distill", "ungated", *thr)}
            forms = {"distill": lambda: ops.distill_loss(student, ts, (S, S), flips=flips, temperature=T, dz=bufs["distill"], scratch=sd),
                     "ungated": lambda: ops.consistency_loss(student, ts, (S, S), flips=flips, temperature=T, dz=bufs["ungated"], scratch=sc)}
            for k, t in thr.items():
                forms[k] = lambda k=k, t=t: ops.consistency_loss(student, ts, (S, S), flips=flips, temperature=T, threshold=t,
                                                                 dz=bufs[k], scratch=sc)
            times = _interleaved(forms, a.reps, a.iters, scale=1e3)
            shares = [int(forms[k]()[1]) / N for k in thr]
            med = {k: statistics.median(v) for k, v in times.items()}
            print(f"{f'{B}x{S}x{S} C={C}':>16s} {h:4d}x{w:<4d} {V:2d} {_fmt(times['distill']):>20s} {_fmt(times['ungated']):>20s} "
                  f"{med['ungated'] / med['distill']:6.2f} " + " ".join(f"{_fmt(times[k]):>20s}" for k in thr)
                  + "   " + ", ".join(f"{s:.1%}" for s in shares), flush=True)
        del student, maps, base, bufs
        torch.cuda.empty_cache()


def _engine(a, dev, **kw):
    from adaptersis_amd.backbones.engines import SegEngine
    from bench import build_engine      # the repository root is on the path
    e = build_engine(a.arch, dev, lr=0.01, mode="train_adapters")
    eng = SegEngine(e.model, e.backbone_encoder, e.cross_vit, e.cross_cnn, e.seg_decoder, lr=0.01, mode="train_adapters", **kw)
    eng.seg_decoder.train()
    return eng


def step_part(a):
    from bench import synthetic
    dev = torch.device("cuda:0")
    img, tgt = synthetic(a.batch, a.imsize, 0, dev)
    ema = dict(ema_decay=0.999)
    gate = dict(distill_threshold=a.threshold)
    groups = {"frozen backbone": {"teacher=None": {}, "teacher=None, average kept": ema, "EMA teacher, 1 view": dict(teacher="ema", **ema, **gate),
                                  "EMA teacher, 2 views": dict(teacher="ema", distill_flip=True, **ema, **gate)}}
    if a.backbone:
        bb = dict(train_backbone=True, optimize_backbone=True)
        groups["--optimize_backbone"] = {"teacher=None, average kept": dict(**ema, **bb), "EMA teacher, 1 view": dict(teacher="ema", **ema, **gate, **bb)}
    print(f"b. ms per train_step, {a.arch} {a.imsize}^2 B={a.batch} train_adapters, median (min..max) of {a.reps} windows of {a.steps} steps")
    for gname, arms in groups.items():
        engines = {k: _engine(a, dev, **kw) for k, kw in arms.items()}
        forms = {k: (lambda e=e: e.train_step(img, tgt)) for k, e in engines.items()}
        probe = engines["EMA teacher, 1 view"]

        def guarded_forward():
            with probe.ema_weights():
                probe._guarded_logits([img])

        forms["one guarded forward under ema_weights()"] = guarded_forward
        times = _interleaved(forms, a.reps, a.steps, warm=a.warmup)
        base = statistics.median(times["teacher=None, average kept"])
        print(f"   {gname}: {sum(b.numel for b in probe.ema.buckets)} averaged elements")
        for k, ts in times.items():
            extra = statistics.median(ts) - base
            views = 2 if "2 views" in k else 1
            note = f"   {extra:+.2f} ms over the arm with the average = {extra / views:.2f} ms per view" if "EMA teacher" in k else ""
            print(f"   {k:>42s} {_fmt(ts, 2):>24s}{note}", flush=True)
        if "teacher=None" in times:
            lo, hi = min(times["teacher=None"]), max(times["teacher=None"])
            print(f"   spread of the teacher=None arm {hi - lo:.3f} ms")
        for k, e in engines.items():
            assert e.optimizer.skipped_steps == 0, (k, e.optimizer.skipped_steps)
        del engines, forms, probe
        torch.cuda.empty_cache()


def _shape(s):
    b, size, c = (int(x) for x in s.split(","))
    return b, size, c


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    ap.add_argument("--backbone", action="store_true", help="part b: also the --optimize_backbone pair")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3, help="part a: calls per window")
    ap.add_argument("--steps", type=int, default=3, help="part b: training steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=_shape, nargs="+", default=[(12, 588, 8), (12, 588, 2)], help="part a: batch,imsize,classes")
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--threshold", type=float, default=0.6, help="part b: the gate of the teacher arms")
    ap.add_argument("--arch", default="vit_large")
    ap.add_argument("--imsize", type=int, default=588)
    ap.add_argument("--batch", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mean_teacher.py measures on an MI355X: no device found")
    if "a" in args.part:
        kernel_part(args)
    if "b" in args.part:
        step_part(args)
