"""Fused test-time augmentation (ops.predict_mask_views, csrc/predict.hip) against the composition of the older ops a user would
write without it, interleaved in one process:
    per view  r = ops.resize_bilinear_fwd(v.flip(2) if mirrored else v, H, W);  acc (+)= torch.softmax(r, -1)
    at the end  encode[acc.argmax(-1)]
    python scripts/bench_predict_views.py            # B = 12, 1080x1920, logits 147x147 and 168x168, C in {2, 8}, K in {2, 6}
Views: K / 2 sizes (the listed logit size and, for K = 6, two more around it), each plain and mirrored.  Medians of --reps timed
windows of --iters calls each (device events), after a warm-up of every form at every shape, fused and composed alternating and
the order swapped every window.  Bytes written, from the shapes: fused 1 B/px; composed per view 4 C (resize) + 4 C (softmax)
+ 4 C (the add into the accumulator; none for the first view, whose softmax is the accumulator), then 8 (int64 argmax) + 1 (table)
per pixel.  The logit maps are not counted: they are read from cache.  The share of pixels on which the two forms differ is
printed (near-ties: the two round differently); it is not a timing."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def window(f, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def view_sizes(h, K):
    """K / 2 logit sizes around h (a multiple of 21 = 588 / 28 apart, as input sizes 14 * 6 apart give with a stride-4 head)."""
    n = K // 2
    return [h + 21 * (i - n // 2) for i in range(n)]


def main(a):
    from adaptersis_amd import ops
    from adaptersis_amd.tools import frame_resize as F
    dev = torch.device("cuda:0")
    B, H, W = a.batch, a.height, a.width
    px = B * H * W
    print(f"B={B} -> {H}x{W}; ms per call, median of {a.reps} windows of {a.iters} calls")
    print(f"{'logits':>9s} {'C':>3s} {'K':>3s} {'fused ms':>9s} {'composed ms':>12s} {'ratio':>6s} {'fused MB':>9s} {'composed MB':>12s} "
          f"{'differ %':>9s}   fused min..max")
    slower = 0
    for h in a.logits:
        for C in a.classes:
            for K in a.views:
                g = torch.Generator().manual_seed(C * 100 + K)
                sizes = view_sizes(h, K)
                views = [(3 * torch.randn((B, s, s, C), generator=g)).to(dev) for s in sizes for _ in (0, 1)]
                flips = [False, True] * len(sizes)
                enc = torch.from_numpy(F.ENCODE_ENDOVIS2017[:C].copy()).to(dev)

                def fused():
                    return ops.predict_mask_views(views, (H, W), enc, flips=flips)

                def composed():
                    acc = None
                    for v, f in zip(views, flips):
                        p = torch.softmax(ops.resize_bilinear_fwd(v.flip(2).contiguous() if f else v, H, W), -1)
                        acc = p if acc is None else acc.add_(p)
                    return enc[acc.argmax(-1)]
                for f in (fused, composed):
                    for _ in range(3):
                        f()
                torch.cuda.synchronize()
                differ = float((fused() != composed()).double().mean())
                tf, tc = [], []
                for r in range(a.reps):
                    order = ((fused, tf), (composed, tc))
                    for f, acc in (order if r % 2 == 0 else order[::-1]):
                        acc.append(window(f, a.iters))
                mf, mc = statistics.median(tf), statistics.median(tc)
                slower += mf > mc
                by_f, by_c = px, px * (4 * C * (3 * K - 1) + 9)
                print(f"{h:4d}x{h:<4d} {C:3d} {K:3d} {mf:9.3f} {mc:12.3f} {mc / mf:6.1f} {by_f / 1e6:9.1f} {by_c / 1e6:12.1f} "
                      f"{100 * differ:9.4f}   {min(tf):.3f}..{max(tf):.3f}", flush=True)
                del views
                torch.cuda.empty_cache()
    print(f"fused slower than composed at {slower} shapes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--logits", type=int, nargs="+", default=[147, 168])
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 8])
    ap.add_argument("--views", type=int, nargs="+", default=[2, 6], help="even view counts: each size plain and mirrored")
    main(ap.parse_args())
