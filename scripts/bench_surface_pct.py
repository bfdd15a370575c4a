"""Percentile Hausdorff on the device (ops.surface_stats(..., percentiles=[95]), asis_surface_quantiles) against the same call
without percentiles and against the host route it replaces.
    python scripts/bench_surface_pct.py              # 12 x 1080x1920 x 8 classes and 12 x 588x588 x 2 classes
Three times per case, per batch, in ms:
  with      ops.surface_stats(pred, target, C, TOL, percentiles=[95]) and the download of ints, sums, ord
  without   the same call without percentiles and the download of ints, sums (what the parent commit runs)
  host      what a user had to do for HD95 before: two calls with return_d2 ("pred", "target"), both int32 [B,C,H,W] fields
            copied to the host, the edge pixels of a side read off its own field (d2 == 0), numpy.percentile of the square roots
            of the pooled distances per (frame, class)
Device routes: median / min / max over --reps windows of --iters calls after warm-up, wall time around a synchronize (the
download is part of the route).  Host route: median of --host-reps.  The maps are those of scripts/bench_surface.py ("near")."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

TOL = (1.0, 2.0, 5.0)
CASES = ((12, 1080, 1920, 8), (12, 588, 588, 2))


def wall(f, iters):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def host_route(p, t, C):
    """-> hd95 [B, C] (nan where a class is not on both sides)."""
    import torch
    from adaptersis_amd import ops
    ints, _, d2p = ops.surface_stats(p, t, C, TOL, return_d2="pred")
    _, _, d2g = ops.surface_stats(p, t, C, TOL, return_d2="target")
    ints, d2p, d2g = ints.cpu().numpy(), d2p.cpu().numpy(), d2g.cpu().numpy()
    out = np.full(ints.shape[:2], np.nan)
    for b in range(ints.shape[0]):
        for c in range(C):
            if ints[b, c, 3] and ints[b, c, 4]:
                d = np.concatenate([d2g[b, c][d2p[b, c] == 0], d2p[b, c][d2g[b, c] == 0]])
                out[b, c] = np.percentile(np.sqrt(d.astype(np.float64)), 95)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    import bench_surface as BS
    from adaptersis_amd import ops
    from adaptersis_amd.segloss.surface import metrics_from_stats
    dev = torch.device("cuda:0")
    print(f"{'case':30s} {'with ms':>9s} {'(min':>8s} {'max)':>8s} {'without ms':>11s} {'(min':>8s} {'max)':>8s} {'added ms':>9s} "
          f"{'host ms':>9s} {'host/with':>10s}")
    for B, H, W, C in CASES:
        pred, tgt = BS.make_maps("near", B, H, W, C, seed=H + C + B)
        p, t = torch.from_numpy(pred).to(dev), torch.from_numpy(tgt).to(dev)
        routes = {"with": lambda: [v.cpu() for v in ops.surface_stats(p, t, C, TOL, percentiles=[95])],
                  "without": lambda: [v.cpu() for v in ops.surface_stats(p, t, C, TOL)]}
        for f in routes.values():
            for _ in range(3):
                f()
        times = {k: [] for k in routes}
        for r in range(a.reps):                                  # interleaved
            for k in (list(routes) if r % 2 == 0 else list(routes)[::-1]):
                times[k].append(wall(routes[k], a.iters))
        ref = host_route(p, t, C)                                # warm-up of the host route, and the check of the device route
        ints, sums, ord_ = routes["with"]()
        for b in range(B):
            for c, m in enumerate(metrics_from_stats(ints[b].numpy(), sums[b].numpy(), TOL, ord_[b].numpy(), [95])):
                if m is not None and not m["unmatched"]:
                    assert abs(m["hd_pct"][0] - ref[b, c]) <= 1e-9 * max(ref[b, c], 1.0), (b, c, m["hd_pct"], ref[b, c])
        th = [wall(lambda: host_route(p, t, C), 1) for _ in range(a.host_reps)]
        mw, mo, mh = statistics.median(times["with"]), statistics.median(times["without"]), statistics.median(th)
        print(f"{B:2d} x {H}x{W} C={C:<2d}              {mw:9.3f} {min(times['with']):8.3f} {max(times['with']):8.3f} {mo:11.3f} "
              f"{min(times['without']):8.3f} {max(times['without']):8.3f} {mw - mo:9.3f} {mh:9.1f} {mh / mw:10.1f}", flush=True)


if __name__ == "__main__":
    main()
