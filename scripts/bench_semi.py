"""Semi-supervised training (SegEngine ignore_index= / train_step(labelled=), ops.seg_loss_ignore, csrc/semi.hip): what the
ignore label and the unlabelled half of a batch cost.
    a. op        ops.seg_loss_ignore against ops.seg_loss_fwd + ops.seg_loss_bwd (the yardstick) on the same input with nothing
                 ignored, at (12 + 12) x 588^2 with C = 2 and C = 8; the yardstick is timed as two arms, so that their difference is
                 the run-to-run spread of the same run.  Then with the second half of the samples unlabelled and with a random
                 30 % of the pixels ignored: the bytes the kernels have to move, computed from the shapes, over the time, against the
                 6.29 TB/s the project takes as the stream rate.
                   all valid        forward: 8 N label bytes + the logits; backward: the same + 4 C N of dz written
                   half unlabelled  the labelled half as above; the unlabelled half its labels once (8 N / 2) and zeros (4 C N / 2)
                   30 % ignored     as all valid: labels and dz are touched for every pixel, the logits through shared taps
    b. step      SegEngine.train_step at the config-3 geometry (ViT-L/14, 588^2, train_adapters) with the EMA teacher: 24 labelled
                 frames against 12 labelled + 12 unlabelled.  The difference is what the hard loss saves.
    c. default   --plain_only: the default step (no new keyword) alone, every window printed: scripts/bench_mix.py's arm of that
                 name, the form to run alternately in this tree and in the parent commit's, each in its own process.
    python scripts/bench_semi.py [--part a|b|ab] [--plain_only]
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
from bench_mix import _labels

STREAM_TBS = 6.29
IGNORE = 255


def op_part(a):
    from adaptersis_amd import ops
    from adaptersis_amd.backbones.engines import SegEngine
    dev = torch.device("cuda:0")
    n_region, mode, eps, n_ce = SegEngine.LOSSES[a.loss]
    print(f"a. us per call (forward + finalize + backward), loss {a.loss}, median (min..max) of {a.reps} windows of {a.iters} calls; "
          f"GB/s = the bytes the kernels must move / the median")
    print(f"{'shape':>16s} {'logits':>9s} {'arm':>18s} {'valid':>7s} {'us':>24s} {'vs parent':>9s} {'MB':>7s} {'GB/s':>6s} {'of stream':>9s}")
    for B, S, C in a.shapes:
        h, w = head_size(S, C, dev)
        g = torch.Generator().manual_seed(S + C)
        lg = (2.0 * torch.randn((B, h, w, C), generator=g)).to(dev)
        tgt = _labels(B, S, C, g)
        half = tgt.clone()
        half[B // 2:] = IGNORE
        rand = tgt.clone()
        rand[torch.rand(tgt.shape, generator=g) < 0.3] = IGNORE
        tgt, half, rand = tgt.to(dev), half.to(dev), rand.to(dev)

        def parent():
            _, coef, _ = ops.seg_loss_fwd(lg, tgt, n_region, mode, eps, n_ce)
            return ops.seg_loss_bwd(lg, tgt, coef, n_region, mode, n_ce)

        forms = {"parent ops": parent, "parent ops again": parent,
                 "ignore, all valid": lambda: ops.seg_loss_ignore(lg, tgt, IGNORE, n_region, mode, eps, n_ce),
                 "half unlabelled": lambda: ops.seg_loss_ignore(lg, half, IGNORE, n_region, mode, eps, n_ce),
                 "30 % ignored": lambda: ops.seg_loss_ignore(lg, rand, IGNORE, n_region, mode, eps, n_ce)}
        assert torch.equal(parent(), forms["ignore, all valid"]()[1]), "nothing ignored: dz differs from the parent ops'"
        N, L = B * S * S, B * h * w * C * 4
        full = 2 * (8 * N + L) + 4 * C * N
        nbytes = {"parent ops": full, "parent ops again": full, "ignore, all valid": full,
                  "half unlabelled": full // 2 + 8 * N // 2 + 4 * C * N // 2, "30 % ignored": full}
        valid = {"parent ops": 1.0, "parent ops again": 1.0, "ignore, all valid": 1.0,
                 "half unlabelled": int(forms["half unlabelled"]()[2].sum()) / N, "30 % ignored": int(forms["30 % ignored"]()[2].sum()) / N}
        times = _interleaved(forms, a.reps, a.iters, scale=1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        for k in forms:
            gbs = nbytes[k] / med[k] / 1e3
            print(f"{f'{B}x{S}x{S} C={C}':>16s} {h:4d}x{w:<4d} {k:>18s} {valid[k]:7.1%} {_fmt(times[k]):>24s} {med[k] / med['parent ops']:9.3f} "
                  f"{nbytes[k] / 1e6:7.0f} {gbs:6.0f} {gbs / (STREAM_TBS * 1e3):9.1%}", flush=True)
        del lg, tgt, half, rand
        torch.cuda.empty_cache()


def step_part(a):
    from bench import synthetic
    dev = torch.device("cuda:0")
    B = 2 * a.batch
    img, tgt = synthetic(B, a.imsize, 0, dev)
    teacher = dict(teacher="ema", distill_threshold=a.threshold, ema_decay=0.999)
    labelled = [True] * a.batch + [False] * a.batch
    print(f"b. ms per train_step, {a.arch} {a.imsize}^2 train_adapters, EMA teacher, median (min..max) of {a.reps} windows of {a.steps} steps")
    engines = {f"{B} labelled": _engine(a, dev, **teacher), f"{a.batch} labelled + {a.batch} unlabelled": _engine(a, dev, **teacher)}
    names = list(engines)
    forms = {names[0]: lambda: engines[names[0]].train_step(img, tgt),
             names[1]: lambda: engines[names[1]].train_step(img, tgt, labelled=labelled)}
    times = _interleaved(forms, a.reps, a.steps, warm=a.warmup)
    for k, ts in times.items():
        print(f"   {k:>32s} {_fmt(ts, 2):>24s}", flush=True)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(f"   difference {med[names[0]] - med[names[1]]:.2f} ms ({med[names[1]] / med[names[0]]:.4f} of the labelled step)")
    for k, e in engines.items():
        assert e.optimizer.skipped_steps == 0, (k, e.optimizer.skipped_steps)
    print(f"   valid pixels per sample of the last semi-supervised step: {engines[names[1]].last_hard_valid.tolist()}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="ab", choices=("a", "b", "ab"))
    ap.add_argument("--plain_only", action="store_true", help="the default step alone (B = --batch), every window printed")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3, help="part a: calls per window")
    ap.add_argument("--steps", type=int, default=3, help="part b: training steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=_shape, nargs="+", default=[(24, 588, 8), (24, 588, 2)], help="part a: batch,imsize,classes")
    ap.add_argument("--loss", default="dice", help="part a: a loss of SegEngine.IGNORE_LOSSES")
    ap.add_argument("--threshold", type=float, default=0.6, help="part b: the gate of the teacher")
    ap.add_argument("--arch", default="vit_large")
    ap.add_argument("--imsize", type=int, default=588)
    ap.add_argument("--batch", type=int, default=12, help="labelled frames a step; part b adds as many unlabelled ones")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_semi.py measures on an MI355X: no device found")
    if args.plain_only:
        import bench_mix
        bench_mix.step_part(args)
    else:
        if "a" in args.part:
            op_part(args)
        if "b" in args.part:
            step_part(args)
