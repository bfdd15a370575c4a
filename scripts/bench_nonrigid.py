"""The non-rigid augmentation block (csrc/nonrigid.hip) inside the augmentation of a training batch: per-batch time of
``TrainAugment.__call__`` (host tables + upload + kernels, wall clock around a synchronize) and of the kernels alone
(``ops.augment`` on tables already on the device, device events), at B = 12, S = 588, for
    p0        drawn with non_rigid_p = 0: the launches of the pipeline without the block
    elastic   every sample elastic     grid   every sample grid-distorted     optical   every sample optically distorted
    drawn     drawn with non_rigid_p = 0.8 (a different batch of draws every call)
Every form carries the same drawn crop / flip / rot90 / CLAHE / table parameters, so the forms differ by the block alone.
Yardstick: the host time of ``scipy.ndimage.gaussian_filter`` over the 24 noise fields of an all-elastic batch, i.e. the blur
alone of the albumentations form, one loader worker.
    python scripts/bench_nonrigid.py [--only p0] [--out profiles/nonrigid_bench.txt]
Medians of --reps timed windows of --iters calls each after a warm-up of every form, the forms alternating and their order
reversed every window.  ``--only p0`` needs nothing of the block: it runs on a tree without it (the parent-commit comparison)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def main(a):
    from adaptersis_amd import ops
    from adaptersis_amd.tools.augment import TrainAugment
    dev = torch.device("cuda:0")
    B, S = a.batch, a.size
    r = np.random.RandomState(0)
    img = torch.from_numpy(r.randint(0, 256, (B, S, S, 3)).astype(np.uint8)).to(dev)
    mask = torch.from_numpy((r.random_sample((B, S, S)) > 0.7).astype(np.uint8)).to(dev)
    aug = TrainAugment(size=S, seed=7)
    base = [aug.draw(B) for _ in range(8)]                       # 8 batches of draws, cycled
    forms = {"p0": base}
    if a.only != "p0":
        nr = TrainAugment(size=S, seed=8, non_rigid_p=1.0)
        kinds = {"elastic": [], "grid": [], "optical": []}
        while min(len(v) for v in kinds.values()) < 8 * B:        # drawn members, sorted by kind
            d = nr._draw_nonrigid()
            kinds[d["kind"]].append(d)
        for k, ds in kinds.items():
            forms[k] = [[dict(p, nonrigid=ds[i * B + b]) for b, p in enumerate(ps)] for i, ps in enumerate(base)]
        p8 = TrainAugment(size=S, seed=9, non_rigid_p=0.8)
        forms["drawn"] = [[dict(p, nonrigid=p8._draw_nonrigid()) for p in ps] for ps in base]
        aug = nr
    names = list(forms)
    count = {n: 0 for n in names}

    def call(n):                                                 # what the training loop pays per batch
        ps = forms[n][count[n] % 8]
        count[n] += 1
        t0 = time.perf_counter()
        aug(img, mask, ps)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    tabs = {n: aug.tables(forms[n][0], dev) for n in names}

    def kernels(n, iters):                                       # the launches alone
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            ops.augment(img, mask, tabs[n])
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / iters

    for n in names:
        for _ in range(3):
            call(n)
            kernels(n, 1)
    wall, kern = {n: [] for n in names}, {n: [] for n in names}
    for rep in range(a.reps):
        for n in (names if rep % 2 == 0 else names[::-1]):
            wall[n].append(statistics.median(call(n) for _ in range(a.iters)))
            kern[n].append(kernels(n, a.iters))
    lines = [f"TrainAugment at B = {B}, S = {S}: ms per batch, median of {a.reps} windows of {a.iters} calls (min..max of the windows)",
             f"{'form':>8s} {'__call__ (wall)':>24s} {'kernels (device)':>24s}"]
    for n in names:
        w, k = wall[n], kern[n]
        lines.append(f"{n:>8s} {statistics.median(w):8.3f} ({min(w):.3f}..{max(w):.3f}) {statistics.median(k):8.3f} ({min(k):.3f}..{max(k):.3f})")
    if a.only != "p0":
        from scipy.ndimage import gaussian_filter
        fields = np.random.RandomState(1).uniform(-1, 1, (2 * B, S, S)).astype(np.float32)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            for f in fields:
                gaussian_filter(f, aug.elastic[1], mode="reflect")
            ts.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"yardstick: scipy.ndimage.gaussian_filter(sigma = {aug.elastic[1]:g}) over {2 * B} fp32 fields of {S} x {S} on the host: "
                     f"{statistics.median(ts):.1f} ms (one thread)")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--size", type=int, default=588)
    ap.add_argument("--only", choices=("all", "p0"), default="all")
    ap.add_argument("--out", default=None)
    main(ap.parse_args())
