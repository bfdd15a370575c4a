"""The hard-pixel loss stages (ops.hardpixel_loss, csrc/hardpixel.hip) against the torch compositions a user would write without
them and against the fused cross-entropy + Dice loss stage of today, interleaved in one process.  Per shape and form:
    fused      ops.hardpixel_loss: loss and dz at the target's size, scratch reused
    +resize^T  the same followed by ops.resize_bilinear_bwd (float32): the gradient back at the head's (h, w), what the
               composition's backward delivers
    composed   top-k: F.interpolate(bilinear) -> F.cross_entropy(reduction="none") -> torch.topk(K, sorted=False) -> mean;
               focal: F.interpolate -> softmax(1) -> the formula of segloss/focal_loss.py:70-88 written in torch on the device
               (one-hot by scatter_, clamp, pt, log, pow; without its target.cpu()); .backward() to the logits
    ce_dc      ops.seg_loss_fwd + ops.seg_loss_bwd of SegEngine.LOSSES["ce_dc"]: a plain fused loss stage as a yardstick
    python scripts/bench_hardpixel.py              # 12 x 588^2 with C = 8 and C = 2; top-k at k = 10 and 100, focal
The (h, w) of the logits are read off the heads: a SegEngine with the tiny test backbone and the MLA head (C = 8) or the
FeatureDecoder (C = 2) evaluates one frame of the size; the head's geometry does not depend on the backbone's width.
Medians of --reps timed windows of --iters calls each (device events), after a warm-up of every form, the forms alternating and
their order reversed every window.  Peak memory: torch's allocator high-water mark of one call on top of the inputs.
--only fused runs that form alone (for a kernel trace: the per-pass breakdown)."""
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


def head_size(imsize, C, dev):
    from adaptersis_amd import train as T
    from adaptersis_amd.backbones.engines import SegEngine
    args = T.get_args_parser().parse_args(["--arch", "vit_tiny_test", "--imsize", str(imsize)])
    model, enc, cv, cn, dec = T.build_modules(args, "mla" if C > 2 else "feature", C, dev)
    eng = SegEngine(model, enc, cv, cn, dec, num_classes=C)
    dec.eval()
    with torch.no_grad():
        lg = eng.eval_logits(torch.zeros((1, 3, imsize, imsize), device=dev))
    return int(lg.shape[1]), int(lg.shape[2])


def peak_mb(f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def main(a):
    from adaptersis_amd import ops
    from adaptersis_amd.backbones.engines import SegEngine
    dev = torch.device("cuda:0")
    print(f"ms per call, median of {a.reps} windows of {a.iters} calls; peak MB of one call")
    print(f"{'shape':>16s} {'loss':>10s} {'logits':>9s} {'fused':>8s} {'+resize^T':>10s} {'composed':>9s} {'ratio':>6s} {'ce_dc':>7s} "
          f"{'fused MB':>9s} {'composed MB':>12s}   fused min..max   |loss diff|")
    for B, S, C in a.shapes:
        h, w = head_size(S, C, dev)
        g = torch.Generator().manual_seed(S + C)
        logits = (2.0 * torch.randn((B, h, w, C), generator=g)).to(dev)
        target = torch.randint(0, C, (B, S, S), generator=g).to(dev)
        nchw = logits.permute(0, 3, 1, 2).contiguous()
        N = B * S * S
        scratch = torch.empty(ops.hardpixel_scratch_bytes(N), device=dev, dtype=torch.uint8)
        n_region, mode, eps, n_ce = SegEngine.LOSSES["ce_dc"]
        for name in a.losses:
            focal = name == "focal"
            K = N if focal else int(N * int(name[4:]) / 100)
            kind = ops.HARDPIXEL_FOCAL if focal else ops.HARDPIXEL_CE
            cfg = dict(n_softmax=1, gamma=2.0, smooth=1e-5) if focal else {}

            def fused():
                return ops.hardpixel_loss(logits, target, kind, K, scratch=scratch, **cfg)

            def fused_rt():
                loss, dz = ops.hardpixel_loss(logits, target, kind, K, scratch=scratch, **cfg)
                return loss, ops.resize_bilinear_bwd(dz, h, w, torch.float32)[0]

            def fused_fresh():   # allocates its scratch: the memory a single call holds
                return ops.hardpixel_loss(logits, target, kind, K, **cfg)

            def composed():
                lg = nchw.detach().requires_grad_(True)
                z = F.interpolate(lg, size=(S, S), mode="bilinear", align_corners=False)
                if focal:
                    q = torch.softmax(z, 1).permute(0, 2, 3, 1).reshape(-1, C)
                    key = torch.zeros((N, C), device=dev).scatter_(1, target.view(-1, 1), 1.0)
                    key = torch.clamp(key, 1e-5 / (C - 1), 1.0 - 1e-5)
                    pt = (key * q).sum(1) + 1e-5
                    loss = (-1 * torch.pow(1 - pt, 2.0) * pt.log()).mean()
                else:
                    ce = F.cross_entropy(z, target, reduction="none")
                    loss = torch.topk(ce.view(-1), K, sorted=False)[0].mean()
                loss.backward()
                return loss, lg.grad

            def ce_dc():
                loss, coef, _ = ops.seg_loss_fwd(logits, target, n_region, mode, eps, n_ce, None, 1.0)
                return loss, ops.seg_loss_bwd(logits, target, coef, n_region, mode, n_ce, None)

            forms = [fused] if a.only == "fused" else [fused, fused_rt, composed, ce_dc]
            for f in forms:
                for _ in range(2):
                    f()
            torch.cuda.synchronize()
            times = {f.__name__: [] for f in forms}
            for r in range(a.reps):
                for f in (forms if r % 2 == 0 else forms[::-1]):
                    times[f.__name__].append(window(f, a.iters))
            med = {k: statistics.median(v) for k, v in times.items()}
            shape = f"{B}x{S}x{S} C={C}"
            if a.only == "fused":
                print(f"{shape:>16s} {name:>10s} {h:4d}x{w:<4d} {med['fused']:8.3f}", flush=True)
                continue
            diff = abs(float(fused()[0]) - float(composed()[0].detach()))
            mb_f, mb_c = peak_mb(fused_fresh), peak_mb(composed)
            tf = times["fused"]
            print(f"{shape:>16s} {name:>10s} {h:4d}x{w:<4d} {med['fused']:8.3f} {med['fused_rt']:10.3f} {med['composed']:9.3f} "
                  f"{med['composed'] / med['fused_rt']:6.1f} {med['ce_dc']:7.3f} {mb_f:9.1f} {mb_c:12.1f}   {min(tf):.3f}..{max(tf):.3f}   "
                  f"{diff:.2e}", flush=True)
        del scratch, logits, target, nchw
        torch.cuda.empty_cache()


def _shape(s):
    b, size, c = (int(x) for x in s.split(","))
    return b, size, c


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--shapes", type=_shape, nargs="+", default=[(12, 588, 8), (12, 588, 2)], help="batch,imsize,classes")
    ap.add_argument("--losses", nargs="+", default=["topk10", "topk100", "focal"], help="topk<percent> or focal")
    ap.add_argument("--only", choices=("all", "fused"), default="all")
    main(ap.parse_args())
