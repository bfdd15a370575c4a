"""Boundary statistics on the device (ops.surface_stats, csrc/surface.hip) against the scipy recipe on the host's 16 CPUs.
    python scripts/bench_surface.py                  # 540x960, 1024x1280, 1080x1920; C in {2, 8}; B in {1, 12}; near and far
    python scripts/bench_surface.py --script DIR     # + the predict entry point with and without --surface, interleaved
Device: median / min / max over --reps timed windows of --iters calls (device events) after warm-up, per frame.  Host: the same
inputs, one task per (frame, class present on either side) spread over a 16-worker process pool (binary_erosion with the cross,
distance_transform_edt of both edge images, the comparisons), wall time of the batch per frame, median of --host-reps.
"near": blobs whose boundaries differ by a few pixels (what a trained model gives); "far": the prediction in one corner, the label
in the opposite one (the long search).  Both have C classes present in every frame."""
import argparse
import multiprocessing as mp
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

WORKERS = 16
TOL = (1.0, 2.0, 5.0)


def host_task(job):
    """One (frame, class): the scipy recipe.  -> a few numbers so that nothing is optimised away."""
    from scipy import ndimage
    P, G = job
    cross = ndimage.generate_binary_structure(2, 1)
    eP = P & ~ndimage.binary_erosion(P, cross, border_value=0)
    eG = G & ~ndimage.binary_erosion(G, cross, border_value=0)
    if not eP.any() or not eG.any():
        return (int(eP.sum()), int(eG.sum()), 0, 0.0)
    dG = ndimage.distance_transform_edt(~eG)
    dP = ndimage.distance_transform_edt(~eP)
    a, b = np.rint(dG[eP] ** 2).astype(np.int64), np.rint(dP[eG] ** 2).astype(np.int64)
    hits = sum(int((a <= int(t * t)).sum()) + int((b <= int(t * t)).sum()) for t in TOL)
    return (int(eP.sum()), int(eG.sum()), hits + int(max(a.max(), b.max())), float(np.sqrt(a).sum() + np.sqrt(b).sum()))


def make_maps(kind, B, H, W, C, seed):
    """-> pred, target uint8 [B,H,W], classes 0..C-1 all present: class 0 the background, one blob per other class."""
    rng = np.random.default_rng(seed)
    pred = np.zeros((B, H, W), dtype=np.uint8)
    tgt = np.zeros((B, H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for b in range(B):
        for c in range(1, C):
            ry, rx = rng.integers(H // 16, H // 6), rng.integers(W // 16, W // 6)
            if kind == "near":
                cy, cx = rng.integers(0, H), rng.integers(0, W)
                dy, dx = rng.integers(-4, 5), rng.integers(-4, 5)
            else:                                           # far: opposite corners
                cy, cx = rng.integers(0, H // 8), rng.integers(0, W // 8)
                dy, dx = H - 1 - 2 * cy, W - 1 - 2 * cx
            pred[b][((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = c
            tgt[b][((yy - cy - dy) / ry) ** 2 + ((xx - cx - dx) / rx) ** 2 <= 1.0] = c
    return pred, tgt


def window(f, iters):
    import torch
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def kernel(pool, reps, iters, host_reps, sizes, classes, batches):
    import torch
    from adaptersis_amd import ops
    dev = torch.device("cuda:0")
    print(f"{'case':38s} {'device ms/frame':>16s} {'(min':>8s} {'max)':>8s} {'host ms/frame':>14s} {'host/device':>12s}")
    for H, W in sizes:
        for C in classes:
            for B in batches:
                for kind in ("near", "far"):
                    pred, tgt = make_maps(kind, B, H, W, C, seed=H + C + B)
                    p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
                    f = lambda: ops.surface_stats(p, t, C, TOL)
                    for _ in range(3):
                        f()
                    torch.cuda.synchronize()
                    td = [window(f, iters) / B for _ in range(reps)]
                    jobs = [(pred[b] == c, tgt[b] == c) for b in range(B) for c in range(C)]
                    th = []
                    for _ in range(host_reps):
                        t0 = time.perf_counter()
                        pool.map(host_task, jobs, chunksize=1)
                        th.append((time.perf_counter() - t0) * 1e3 / B)
                    md, mh = statistics.median(td), statistics.median(th)
                    print(f"{kind:5s} {H}x{W} C={C:<2d} B={B:<3d}            {md:16.3f} {min(td):8.3f} {max(td):8.3f} {mh:14.1f} {mh / md:12.1f}",
                          flush=True)


def script(root, out, rounds):
    """``predict --masks`` with and without ``--surface`` on bench_predict's tree (12 frames of 1280x1024, 8 classes), one engine,
    runs interleaved, median of ``rounds``."""
    import torch
    import bench_predict as BP
    from adaptersis_amd import predict as P
    from adaptersis_amd import train as T
    BP.make_frames(root)
    base = ["--imsize", "588", "--batch_size_per_gpu", "12", "--output_dir", out, "--head", "mla", "--num_classes", "8", "--seed", "0",
            "--input", root, "--dataset", "endovis2017", "--split", "Test", "--encode", "endovis2017", "--masks"]
    args = P.get_args_parser().parse_args(base + ["--pred_dir", os.path.join(out, "pred")])
    os.makedirs(out, exist_ok=True)
    torch.manual_seed(0)
    _, _, _, _, dec = T.build_modules(args, "mla", 8, torch.device("cuda", 0))
    torch.save({"epoch": 0, "state_dict": {"module." + k: v.cpu() for k, v in dec.state_dict().items()}},
               os.path.join(out, "checkpoint.pth.tar"))
    del dec
    eng = P.build_engine(args)
    forms = {"masks+metrics": [], "masks+metrics+surface": ["--surface"]}
    parsed = {k: P.get_args_parser().parse_args(base + ["--pred_dir", os.path.join(out, "pred_" + k)] + v) for k, v in forms.items()}
    fps = {k: [] for k in forms}
    for a in parsed.values():
        P.predict_seg(a, engine=eng)          # warm-up: code objects, tables
    for r in range(rounds):
        order = list(forms) if r % 2 == 0 else list(forms)[::-1]
        for k in order:
            fps[k].append(P.predict_seg(parsed[k], engine=eng)["frames_per_second"])
    med = {k: statistics.median(v) for k, v in fps.items()}
    for k, v in fps.items():
        print(f"predict entry point, 12 x 1280x1024, {k}: median {med[k]:.2f} frames/s of {rounds} (min {min(v):.2f}, max {max(v):.2f})")
    print(f"with --surface / without: {med['masks+metrics+surface'] / med['masks+metrics']:.3f}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--size", default=None, help="HxW: this size only")
    ap.add_argument("--no-kernel", action="store_true", help="the entry point only (with --script)")
    ap.add_argument("--script", default=None, help="directory for the generated frames and the outputs of the entry point")
    a = ap.parse_args()
    sizes = (tuple(int(v) for v in a.size.split("x")),) if a.size else ((540, 960), (1024, 1280), (1080, 1920))
    # the workers are forked before this process touches the GPU: they run numpy / scipy only
    with mp.get_context("fork").Pool(WORKERS) as pool:
        if not a.no_kernel:
            kernel(pool, a.reps, a.iters, a.host_reps, sizes, (2, 8), (1, 12))
    if a.script:
        script(os.path.join(a.script, "tree"), os.path.join(a.script, "out"), a.rounds)
