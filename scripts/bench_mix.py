"""Batch mixing (SegEngine mix=, ops.mix_batch, ops.consistency_loss(mix=), csrc/mix.hip): what the mixing costs.
    a. op        ops.mix_batch, cutmix and classmix, against the torch composition of the same result (one-hot presence,
                 index_select, where; checked equal once), at 12 x 588^2 with C = 2 and C = 8; the bytes the kernels have to move
                 (image and labels read and written once, sel written, for classmix the donor's labels read as well) over the time,
                 against the 6.29 TB/s the project takes as the stream rate.
    b. loss      ops.consistency_loss with mix= against without, both added into a given dz at a threshold that keeps about half
                 of the pixels, V = 1 and 2 teacher maps, sel about 50 %.
    c. step      SegEngine.train_step at the config-3 geometry (ViT-L/14, 588^2, B = 12, train_adapters): mix=None and classmix,
                 without a teacher and with the EMA teacher.  --plain_only times the mix=None arm alone and prints every window: the
                 form to run alternately in this tree and in another one (the parent commit's), each in its own process.
    python scripts/bench_mix.py [--part a|b|c|abc] [--plain_only]
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


def _labels(B, S, C, g):
    """blobs of the classes 1..C-1 on background, one sample of background alone (the shape of the project's data)"""
    tgt = torch.zeros((B, S, S), dtype=torch.int64)
    for b in range(B - 1):
        for c in range(1, C):
            y, x = (int(v) for v in torch.randint(0, S - S // 4, (2,), generator=g))
            tgt[b, y:y + S // 4, x:x + S // 6] = c
    return tgt


def torch_mix(img, tgt, t, C, background):
    """the result of ops.mix_batch composed from torch ops, tables ``t`` on the device (inv_order: the rank of each class in order)"""
    B, H, W = tgt.shape
    d = t["donor"].long()
    td = tgt.index_select(0, d)
    valid = (td >= 0) & (td < C)
    present = torch.nn.functional.one_hot(tgt.clamp(0, C - 1), C).flatten(1, 2).any(1)   # the labels measured are all in 0..C-1
    P = present.index_select(0, d)
    if not background:
        P[:, 0] = False
    rank = t["inv_order"][:, :C]
    before = (P.unsqueeze(1) & (rank.unsqueeze(1) < rank.unsqueeze(2))).sum(2)
    chosen = P & (before < (P.sum(1, keepdim=True) + 1) // 2)
    sel2 = chosen.gather(1, td.clamp(0, C - 1).flatten(1)).view(B, H, W) & valid
    ys, xs = torch.arange(H, device=tgt.device).view(1, H, 1), torch.arange(W, device=tgt.device).view(1, 1, W)
    y0, x0, y1, x1 = (t["box"][:, i].view(B, 1, 1) for i in range(4))
    sel1 = (ys >= y0) & (ys < y1) & (xs >= x0) & (xs < x1)
    kind = t["kind"].view(B, 1, 1)
    sel = torch.where(kind == 1, sel1, torch.where(kind == 2, sel2, torch.zeros_like(sel1)))
    return (torch.where(sel.unsqueeze(1), img.index_select(0, d), img), torch.where(sel, td, tgt), sel.to(torch.uint8),
            sel.flatten(1).sum(1, dtype=torch.int32))


def op_part(a):
    from adaptersis_amd import ops
    from adaptersis_amd.tools.mix import MixSampler
    dev = torch.device("cuda:0")
    print(f"a. us per call, median (min..max) of {a.reps} windows of {a.iters} calls; GB/s = the bytes the kernels must move / the median")
    print(f"{'shape':>16s} {'kind':>9s} {'pasted':>7s} {'ops.mix_batch':>22s} {'GB/s':>6s} {'of stream':>9s} {'torch composition':>22s} {'ratio':>6s}")
    for B, S, C in a.shapes:
        g = torch.Generator().manual_seed(S + C)
        img, tgt = torch.randn((B, 3, S, S), generator=g).to(dev), _labels(B, S, C, g).to(dev)
        for kind in ("cutmix", "classmix"):
            t = MixSampler(kind, seed=1, num_classes=C).draw(B, S, S, 0)
            td = {k: v.to(dev) for k, v in t.items()}
            td["inv_order"] = t["order"].long().argsort(1).to(dev)
            forms = {"op": lambda: ops.mix_batch(img, tgt, t, C), "torch": lambda: torch_mix(img, tgt, td, C, False)}
            got, want = forms["op"](), forms["torch"]()
            assert all(torch.equal(x, y) for x, y in zip(got, want)), f"the torch composition differs ({kind}, C={C})"
            times = _interleaved(forms, a.reps, a.iters, scale=1e3)
            med = {k: statistics.median(v) for k, v in times.items()}
            nbytes = B * S * S * (2 * 12 + 2 * 8 + 1 + (16 if kind == "classmix" else 0))   # classmix: two passes over the labels
            gbs = nbytes / med["op"] / 1e3
            print(f"{f'{B}x{S}x{S} C={C}':>16s} {kind:>9s} {int(got[3].sum()) / tgt.numel():7.1%} {_fmt(times['op']):>22s} {gbs:6.0f} "
                  f"{gbs / (STREAM_TBS * 1e3):9.1%} {_fmt(times['torch']):>22s} {med['torch'] / med['op']:6.2f}", flush=True)
        del img, tgt
        torch.cuda.empty_cache()


def loss_part(a):
    from adaptersis_amd import ops
    dev = torch.device("cuda:0")
    T = a.temperature
    print(f"b. us per call added into dz, median (min..max) of {a.reps} windows of {a.iters} calls; T = {T:g}, sel about 50 %")
    print(f"{'shape':>16s} {'logits':>9s} {'V':>2s} {'unmixed':>22s} {'mixed':>22s} {'ratio':>6s}   kept shares")
    for B, S, C in a.shapes:
        h, w = head_size(S, C, dev)
        g = torch.Generator().manual_seed(S + C)
        student = (2.0 * torch.randn((B, h, w, C), generator=g)).to(dev)
        maps = [(2.0 * torch.randn((B, h, w, C), generator=g)).to(dev) for _ in range(2)]
        sel = (torch.rand((B, S, S), generator=g) < 0.5).to(torch.uint8).to(dev)
        donor = [(b + 1) % B for b in range(B)]
        N = B * S * S
        sc = torch.empty(ops.consistency_scratch_bytes(N), device=dev, dtype=torch.uint8)
        base = torch.randn((B, S, S, C), generator=g).to(dev)
        for V in (1, 2):
            ts, flips = maps[:V], [False, True][:V]
            q = sum(torch.softmax(torch.nn.functional.interpolate((t.flip(2) if f else t).permute(0, 3, 1, 2), size=(S, S), mode="bilinear",
                                                                  align_corners=False) / T, 1) for t, f in zip(ts, flips)) / V
            conf = q.amax(1).flatten()
            thr = float(conf[torch.randint(0, conf.numel(), (1 << 20,), device=dev)].quantile(0.5))
            del q, conf
            bufs = {k: base.clone() for k in ("unmixed", "mixed")}
            kw = dict(flips=flips, temperature=T, threshold=thr, scratch=sc)
            forms = {"unmixed": lambda: ops.consistency_loss(student, ts, (S, S), dz=bufs["unmixed"], **kw),
                     "mixed": lambda: ops.consistency_loss(student, ts, (S, S), dz=bufs["mixed"], mix=(sel, donor), **kw)}
            times = _interleaved(forms, a.reps, a.iters, scale=1e3)
            shares = [int(forms[k]()[1]) / N for k in forms]
            med = {k: statistics.median(v) for k, v in times.items()}
            print(f"{f'{B}x{S}x{S} C={C}':>16s} {h:4d}x{w:<4d} {V:2d} {_fmt(times['unmixed']):>22s} {_fmt(times['mixed']):>22s} "
                  f"{med['mixed'] / med['unmixed']:6.2f}   " + ", ".join(f"{s:.1%}" for s in shares), flush=True)
        del student, maps, base, bufs, sel
        torch.cuda.empty_cache()


def step_part(a):
    from bench import synthetic
    dev = torch.device("cuda:0")
    img, tgt = synthetic(a.batch, a.imsize, 0, dev)
    ema = dict(ema_decay=0.999)
    teacher = dict(teacher="ema", distill_threshold=a.threshold, **ema)
    arms = {"mix=None": {}} if a.plain_only else {"mix=None": {}, "classmix": dict(mix="classmix"), "EMA teacher": teacher,
                                                  "EMA teacher, classmix": dict(mix="classmix", **teacher)}
    print(f"c. ms per train_step, {a.arch} {a.imsize}^2 B={a.batch} train_adapters, median (min..max) of {a.reps} windows of {a.steps} steps")
    engines = {k: _engine(a, dev, **kw) for k, kw in arms.items()}
    forms = {k: (lambda e=e: e.train_step(img, tgt)) for k, e in engines.items()}
    times = _interleaved(forms, a.reps, a.steps, warm=a.warmup)
    for k, ts in times.items():
        print(f"   {k:>24s} {_fmt(ts, 2):>24s}" + ("   windows " + " ".join(f"{t:.2f}" for t in ts) if a.plain_only else ""), flush=True)
    for k, e in engines.items():
        assert e.optimizer.skipped_steps == 0, (k, e.optimizer.skipped_steps)
        pasted = getattr(e, "last_mix_pasted", None)
        if pasted is not None:
            print(f"   {k}: {int(pasted.sum()) / tgt.numel():.1%} of the last batch's pixels pasted")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="abc", choices=("a", "b", "c", "ab", "abc"))
    ap.add_argument("--plain_only", action="store_true", help="part c: the mix=None arm alone, every window printed")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3, help="parts a, b: calls per window")
    ap.add_argument("--steps", type=int, default=3, help="part c: training steps per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", type=_shape, nargs="+", default=[(12, 588, 8), (12, 588, 2)], help="parts a, b: batch,imsize,classes")
    ap.add_argument("--temperature", type=float, default=2.0)
    ap.add_argument("--threshold", type=float, default=0.6, help="part c: the gate of the teacher arms")
    ap.add_argument("--arch", default="vit_large")
    ap.add_argument("--imsize", type=int, default=588)
    ap.add_argument("--batch", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix.py measures on an MI355X: no device found")
    if "a" in args.part:
        op_part(args)
    if "b" in args.part:
        loss_part(args)
    if "c" in args.part:
        step_part(args)
