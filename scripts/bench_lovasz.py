"""The Lovasz-Softmax loss stage (ops.lovasz_softmax, csrc/lovasz.hip) against the torch composition a user would write without
it and against the soft-IoU loss stage of today, interleaved in one process:
    lovasz     ops.lovasz_softmax(logits, target, n_softmax=1): loss and dz at the target's size, scratch reused
    +resize^T  the same followed by ops.resize_bilinear_bwd (float32): the gradient back at the head's (h, w), what the
               composition's backward delivers
    composed   F.interpolate(bilinear) -> softmax(1) -> per class |t - q|, torch.sort(descending), the reference formula of
               lovasz_grad (cumulative sums and differences, float32), dot -> mean; .backward() to the logits (written here)
    iou        ops.seg_loss_fwd + ops.seg_loss_bwd of SegEngine.LOSSES["iou"]: the scale of the loss stage today
    python scripts/bench_lovasz.py                 # 12 x 588^2 with C = 8 and C = 2, 12 x 672^2 with C = 2
The (h, w) of the logits are read off the heads: a SegEngine with the tiny test backbone and the MLA head (C = 8) or the
FeatureDecoder (C = 2) evaluates one frame of the size; the head's geometry does not depend on the backbone's width.
Medians of --reps timed windows of --iters calls each (device events), after a warm-up of every form, the forms alternating and
their order reversed every window.  Peak memory: torch's allocator high-water mark of one call on top of the inputs.
--only lovasz runs that form alone (for a kernel trace: the per-pass breakdown)."""
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


def reference_lovasz_grad(gt_sorted):
    gts = gt_sorted.sum()
    inter = gts - gt_sorted.cumsum(0)
    union = gts + (1.0 - gt_sorted).cumsum(0)
    jac = 1.0 - inter / union
    return torch.cat([jac[:1], jac[1:] - jac[:-1]])


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
    print(f"{'shape':>16s} {'logits':>9s} {'lovasz':>8s} {'+resize^T':>10s} {'composed':>9s} {'ratio':>6s} {'iou':>7s} "
          f"{'lovasz MB':>10s} {'composed MB':>12s}   lovasz min..max   |loss diff|")
    for B, S, C in a.shapes:
        h, w = head_size(S, C, dev)
        g = torch.Generator().manual_seed(S + C)
        logits = (2.0 * torch.randn((B, h, w, C), generator=g)).to(dev)
        target = torch.randint(0, C, (B, S, S), generator=g).to(dev)
        nchw = logits.permute(0, 3, 1, 2).contiguous()
        scratch = torch.empty(ops.lovasz_scratch_bytes(B * S * S, C), device=dev, dtype=torch.uint8)
        n_region, mode, eps, n_ce = SegEngine.LOSSES["iou"]

        def lovasz():
            return ops.lovasz_softmax(logits, target, 1, "mean", 1.0, scratch=scratch)

        def lovasz_rt():
            loss, _, dz = ops.lovasz_softmax(logits, target, 1, "mean", 1.0, scratch=scratch)
            return loss, ops.resize_bilinear_bwd(dz, h, w, torch.float32)[0]

        def lovasz_fresh():   # allocates its scratch: the memory a single call holds
            return ops.lovasz_softmax(logits, target, 1, "mean", 1.0)

        def composed():
            lg = nchw.detach().requires_grad_(True)
            q = torch.softmax(F.interpolate(lg, size=(S, S), mode="bilinear", align_corners=False), 1)
            q = q.permute(0, 2, 3, 1).reshape(-1, C)
            t = target.view(-1)
            losses = []
            for c in range(C):
                tc = (t == c).float()
                e, idx = torch.sort((tc - q[:, c]).abs(), 0, descending=True)
                losses.append(torch.dot(e, reference_lovasz_grad(tc[idx])))
            loss = torch.stack(losses).mean()
            loss.backward()
            return loss, lg.grad

        def iou():
            loss, coef, _ = ops.seg_loss_fwd(logits, target, n_region, mode, eps, n_ce, None, 1.0)
            return loss, ops.seg_loss_bwd(logits, target, coef, n_region, mode, n_ce, None)

        forms = [lovasz] if a.only == "lovasz" else [lovasz, lovasz_rt, composed, iou]
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
        if a.only == "lovasz":
            print(f"{shape:>16s} {h:4d}x{w:<4d} {med['lovasz']:8.3f}", flush=True)
            continue
        diff = abs(float(lovasz()[0]) - float(composed()[0].detach()))
        mb_l, mb_c = peak_mb(lovasz_fresh), peak_mb(composed)
        tl = times["lovasz"]
        print(f"{shape:>16s} {h:4d}x{w:<4d} {med['lovasz']:8.3f} {med['lovasz_rt']:10.3f} {med['composed']:9.3f} "
              f"{med['composed'] / med['lovasz_rt']:6.1f} {med['iou']:7.3f} {mb_l:10.1f} {mb_c:12.1f}   {min(tl):.3f}..{max(tl):.3f}   "
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
    ap.add_argument("--shapes", type=_shape, nargs="+", default=[(12, 588, 8), (12, 588, 2), (12, 672, 2)],
                    help="batch,imsize,classes")
    ap.add_argument("--only", choices=("all", "lovasz"), default="all")
    main(ap.parse_args())
