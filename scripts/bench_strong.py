"""The strong student view (ops.strong_view, csrc/strongaug.hip): what colour jitter, greyscale and blur cost on the device.
    a. op        ops.strong_view at 12 x 588^2 and (12 + 12) x 588^2, every sample of the batch with the arm's draw: jitter only (all
                 four operations, a drawn order: two launches, the contrast mean first), jitter without contrast (one launch), jitter
                 + grey, blur alone at r = 1 and r = 6, everything (jitter, grey, r = 6).  Each against the torch composition of the
                 same result on the device (the restatement tests/strong_ref.py per sample: elementwise ops and a mean; the blur as
                 two conv2d over a reflect pad), and as a share of the 6.29 TB/s the project takes as the stream rate for the
                 2 x 12 B S^2 bytes the op has to move (one read, one write of three fp32 planes).  The op's windows are device
                 time: a few large matrix products are queued in front of every window, so that the host, which spends tens of
                 microseconds a call on the argument checks, runs ahead of the device; that host time is printed beside it.
    b. step      SegEngine.train_step at the config-3 geometry (ViT-L/14, 588^2, B = 12, train_adapters) with the EMA teacher, without
                 and with the strong view: the second arm draws (TrainAugment's strong generator), uploads the tables, runs
                 ops.strong_view and hands the input itself to the teacher, as train.py --aug_strong does.  A third arm gives the
                 teacher a second tensor with the same pixels: what a separate teacher input alone changes.
    c. default   --plain_only: the default step (no new keyword) alone, every window printed: scripts/bench_mix.py's arm of that
                 name, the form to run alternately in this tree and in the parent commit's, each in its own process.
    python scripts/bench_strong.py [--part a|b|ab] [--plain_only]
Medians of --reps timed windows (device events) after a warm-up of every arm, the arms alternating and their order reversed every
window; min and max beside each median.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from bench_mean_teacher import _engine, _fmt, _interleaved

STREAM_TBS = 6.29
SIGMA = {1: 0.3, 6: 2.0}


def _draws(B, arm, seed):
    """the arm's draw for every sample: the factors and orders of TrainAugment's generator, the members switched by the arm"""
    from adaptersis_amd.tools.augment import ST_CONTRAST, TrainAugment
    jitter, contrast, grey, r = arm
    drawn = [p["strong"] for p in TrainAugment(size=64, seed=seed, strong=dict(jitter_p=1.0)).draw(B)]
    out = []
    for d in drawn:
        order, fac = (d["order"], d["factors"]) if jitter else (None, None)
        if jitter and not contrast:
            keep = [k for k, o in enumerate(order) if o != ST_CONTRAST]
            order, fac = tuple(order[k] for k in keep) + (-1,), tuple(fac[k] for k in keep) + (0.0,)
        out.append({"strong": {"order": order, "factors": fac, "grey": grey, "sigma": SIGMA[r] if r else None}})
    return out


def _ahead_windows(forms, reps, iters, blocker):
    """as ``_interleaved``, with ``blocker`` queued in front of every window: the window is the device's time for ``iters`` calls"""
    import time
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times, host = {k: [] for k in forms}, {k: [] for k in forms}
    for f in forms.values():
        f()
    torch.cuda.synchronize()
    order = list(forms)
    for r in range(reps):
        for k in (order if r % 2 == 0 else order[::-1]):
            blocker()
            s.record()
            t0 = time.perf_counter()
            for _ in range(iters):
                forms[k]()
            host[k].append((time.perf_counter() - t0) / iters * 1e6)
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / iters * 1e3)
    return times, host


def torch_view(x, host):
    """the same result composed from torch ops on the device"""
    from tests import strong_ref as R
    ops_, fac, flags, gauss = (host[k].numpy() for k in ("st_ops", "st_fac", "st_flags", "st_gauss"))
    out = torch.empty_like(x)
    for b in range(x.shape[0]):
        v = R.jitter(x[b], ops_[b], fac[b])
        if flags[b, 0]:
            v = R.to_grey(v)
        r = int(flags[b, 1])
        if r:
            w = torch.from_numpy(gauss[b, 6 - r:7 + r].copy()).to(x.device)
            v = F.conv2d(F.pad(v[:, None], (r, r, 0, 0), mode="reflect"), w.view(1, 1, 1, -1))
            v = F.conv2d(F.pad(v, (0, 0, r, r), mode="reflect"), w.view(1, 1, -1, 1))[:, 0].clamp(0.0, 1.0)
        out[b] = v
    return out


ARMS = {"jitter only": (True, True, False, 0), "jitter, no contrast": (True, False, False, 0), "jitter + grey": (True, True, True, 0),
        "blur r=1": (False, False, False, 1), "blur r=6": (False, False, False, 6), "everything": (True, True, True, 6)}


def op_part(a):
    from adaptersis_amd import ops
    from adaptersis_amd.tools.augment import TrainAugment
    dev = torch.device("cuda:0")
    S = a.imsize
    aug = TrainAugment(size=S, strong={})
    print(f"a. us per call, median (min..max) of {a.reps} windows of {a.iters} calls; GB/s = 2 x 12 B S^2 bytes / the median")
    print(f"{'shape':>12s} {'arm':>20s} {'launches':>8s} {'strong_view us':>24s} {'host us':>7s} {'torch us':>28s} {'torch / op':>10s} {'MB':>5s} {'GB/s':>6s} {'of stream':>9s} {'max diff':>9s}")
    big = torch.randn((4096, 4096), device=dev)

    def blocker():
        for _ in range(4):
            torch.mm(big, big)
    for B in a.batches:
        x = torch.rand((B, 3, S, S), generator=torch.Generator().manual_seed(B)).to(dev)
        out = torch.empty_like(x)
        nbytes = 2 * 12 * B * S * S
        tables = {k: aug.strong_tables(_draws(B, arm, 7), dev) for k, arm in ARMS.items()}
        forms = {k: (lambda t=t: ops.strong_view(x, t, out=out)) for k, t in tables.items()}
        composed = {k + " / torch": (lambda t=t: torch_view(x, t["st_host"])) for k, t in tables.items()}
        diff = {k: float((ops.strong_view(x, t) - torch_view(x, t["st_host"])).abs().max()) for k, t in tables.items()}
        assert max(diff.values()) < 2e-5, diff
        times, host = _ahead_windows(forms, a.reps, a.iters, blocker)
        times.update(_interleaved(composed, max(3, a.reps // 3), 1, warm=1, scale=1e3))
        med = {k: statistics.median(v) for k, v in times.items()}
        for k, t in tables.items():
            gbs = nbytes / med[k] / 1e3
            print(f"{f'{B}x{S}x{S}':>12s} {k:>20s} {1 + int(t['contrast_any']):8d} {_fmt(times[k]):>24s} {statistics.median(host[k]):7.0f} {_fmt(times[k + ' / torch']):>28s} "
                  f"{med[k + ' / torch'] / med[k]:10.1f} {nbytes / 1e6:5.0f} {gbs:6.0f} {gbs / (STREAM_TBS * 1e3):9.1%} {diff[k]:9.1e}", flush=True)
        del x, out, tables, forms, composed
        torch.cuda.empty_cache()


def step_part(a):
    from adaptersis_amd import ops
    from adaptersis_amd.tools.augment import TrainAugment
    from bench import synthetic
    dev = torch.device("cuda:0")
    img, tgt = synthetic(a.batch, a.imsize, 0, dev)
    img = img.clamp(0.0, 1.0).contiguous()
    teacher = dict(teacher="ema", distill_threshold=a.threshold, ema_decay=0.999)
    aug = TrainAugment(size=a.imsize, seed=1000, strong={})
    applied = []

    def strong_step(eng):
        params = aug.draw(a.batch)
        applied.append(sum(p["strong"] is not None for p in params) / a.batch)
        return eng.train_step(ops.strong_view(img, aug.strong_tables(params, dev)), tgt, None, img)

    print(f"b. ms per train_step, {a.arch} {a.imsize}^2 B={a.batch} train_adapters, EMA teacher, median (min..max) of {a.reps} windows of {a.steps} steps")
    twin = img.clone()
    names = ("EMA teacher", "EMA teacher, strong view", "EMA teacher, a second tensor")
    engines = {k: _engine(a, dev, **teacher) for k in names}
    forms = {names[0]: lambda: engines[names[0]].train_step(img, tgt), names[1]: lambda: strong_step(engines[names[1]]),
             names[2]: lambda: engines[names[2]].train_step(twin, tgt, None, img)}
    times = _interleaved(forms, a.reps, a.steps, warm=a.warmup)
    for k, ts in times.items():
        print(f"   {k:>28s} {_fmt(ts, 2):>24s}", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    for base in (names[2], names[0]):
        print(f"   strong view - {base!r}: {med[names[1]] - med[base]:+.2f} ms ({med[names[1]] / med[base]:.4f})")
    print(f"   {np.mean(applied):.1%} of the samples had a strong draw")
    for k, e in engines.items():
        assert e.optimizer.skipped_steps == 0, (k, e.optimizer.skipped_steps)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    ap.add_argument("--plain_only", action="store_true", help="the default step alone (B = --batch), every window printed")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10, help="part a: calls per window")
    ap.add_argument("--steps", type=int, default=3, help="part b: training steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", type=int, nargs="+", default=[12, 24], help="part a: batch sizes")
    ap.add_argument("--threshold", type=float, default=0.6, help="part b: the gate of the teacher")
    ap.add_argument("--arch", default="vit_large")
    ap.add_argument("--imsize", type=int, default=588)
    ap.add_argument("--batch", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_strong.py measures on an MI355X: no device found")
    if args.plain_only:
        import bench_mix
        bench_mix.step_part(args)
    else:
        if "a" in args.part:
            op_part(args)
        if "b" in args.part:
            step_part(args)
