"""Fused sliding-window blend (ops.predict_mask_tiles, csrc/predict.hip) against the straightforward torch composition on the device,
interleaved in one process:
    per tile  s = F.grid_sample(map_k, grid_k, "bilinear", padding_mode="border", align_corners=False)   # at the native pixel centres
              acc (+)= weight_k * torch.softmax(s, 1)
    at the end  encode[(acc / wsum).argmax(1)]
    python scripts/bench_predict_tiles.py      # B = 4, 1024x1280 and 1080x1920, tile maps 147x147, C in {2, 8, 11}
Tile sets: the 3 x 3 windows of --slide_size 1176 at --imsize 588 (stride 392 = 2 * 588 // 3, the tool's default), and the same plus the context tile, every tile also
mirrored (20 tiles); ramp blend of width 196.  The composition is given every advantage that does not change what it computes: the
maps already NCHW, the sampling grids, the weight maps and 1 / wsum made once outside the timed region (a mirrored map is flipped
inside it, as the views bench does).  Medians of --reps timed windows of --iters calls each (device events), after a warm-up of both
forms at every shape, fused and composed alternating and the order swapped every window.  Bytes written, from the shapes: fused
1 B/px; composed per tile 4 C (sample) + 4 C (softmax) + 4 C (weighting) + 4 C (the add; none for the first tile), then 4 C (the
division) + 8 (int64 argmax) + 1 (table) per pixel.  The share of pixels on which the two forms differ is printed (near-ties and
pixel centres within rounding of a tile edge); it is not a timing."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F


def window(f, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def axis(n, L, o, s, R, dev):
    """One axis of one tile at the n native pixel centres -> (grid_sample coordinate, weight incl. coverage), fp32 on the device."""
    u = (torch.arange(n, dtype=torch.float64) + 0.5) * L / n
    inf = torch.full_like(u, float("inf"))
    g = torch.minimum(torch.minimum(inf if o == 0 else u - o, inf if o + s == L else (o + s) - u), torch.full_like(u, float(R))) / R
    g = g * ((u >= o) & (u < o + s))
    return (2.0 * (u - o) / s - 1.0).float().to(dev), g.float().to(dev)


def main(a):
    from adaptersis_amd import ops
    from adaptersis_amd import predict as P
    dev = torch.device("cuda:0")
    B, S, L, T, h = a.batch, a.imsize, a.slide_size, a.slide_stride, a.logits
    R = max(S - T, 1)
    print(f"B={B}, --imsize {S} --slide_size {L} --slide_stride {T}, tile maps {h}x{h}, ramp {R}; ms per call, median of {a.reps} windows "
          f"of {a.iters} calls")
    print(f"{'native':>10s} {'C':>3s} {'K':>3s} {'fused ms':>9s} {'composed ms':>12s} {'ratio':>6s} {'fused MB':>9s} {'composed MB':>12s} "
          f"{'differ %':>9s}   fused min..max")
    slower = 0
    for H, W in a.native:
        for C in a.classes:
            for context, flip in ((False, False), (True, True)):
                tiles = P.plan_tiles(L, S, T, context, flip)
                K = len(tiles)
                g = torch.Generator().manual_seed(C * 100 + K)
                maps = [(3 * torch.randn((B, h, h, C), generator=g)).to(dev) for _ in tiles]
                enc = (torch.arange(C, dtype=torch.uint8) * 23).to(dev)
                nchw = [m.permute(0, 3, 1, 2).contiguous() for m in maps]
                grids, weights = [], []
                for oy, ox, sy, sx, _ in tiles:
                    cy, gy = axis(H, L, oy, sy, R, dev)
                    cx, gx = axis(W, L, ox, sx, R, dev)
                    grids.append(torch.stack((cx[None, :].expand(H, W), cy[:, None].expand(H, W)), -1)[None].expand(B, H, W, 2).contiguous())
                    weights.append((gy[:, None] * gx[None, :])[None, None].contiguous())
                inv = 1.0 / torch.stack(weights).sum(0)

                def fused():
                    return ops.predict_mask_tiles(maps, tiles, L, (H, W), enc, blend="ramp", ramp=R)

                def composed():
                    acc = None
                    for m, grid, wt, t in zip(nchw, grids, weights, tiles):
                        s = F.grid_sample(m.flip(3) if t[4] else m, grid, mode="bilinear", padding_mode="border", align_corners=False)
                        p = torch.softmax(s, 1).mul_(wt)
                        acc = p if acc is None else acc.add_(p)
                    return enc[acc.mul_(inv).argmax(1)]
                for f in (fused, composed):
                    for _ in range(2):
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
                px = B * H * W
                by_f, by_c = px, px * (4 * C * (4 * K - 1) + 4 * C + 9)
                print(f"{H:5d}x{W:<4d} {C:3d} {K:3d} {mf:9.3f} {mc:12.3f} {mc / mf:6.1f} {by_f / 1e6:9.1f} {by_c / 1e6:12.1f} "
                      f"{100 * differ:9.4f}   {min(tf):.3f}..{max(tf):.3f}", flush=True)
                del maps, nchw, grids, weights, inv
                torch.cuda.empty_cache()
    print(f"fused slower than composed at {slower} shapes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--native", type=lambda s: tuple(int(v) for v in s.split("x")), nargs="+", default=[(1024, 1280), (1080, 1920)],
                    metavar="HxW")
    ap.add_argument("--imsize", type=int, default=588)
    ap.add_argument("--slide_size", type=int, default=1176)
    ap.add_argument("--slide_stride", type=int, default=392)
    ap.add_argument("--logits", type=int, default=147, help="side of a tile's logit map (147 = 588 / 4)")
    ap.add_argument("--classes", type=int, nargs="+", default=[2, 8, 11])
    main(ap.parse_args())
