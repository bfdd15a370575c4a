"""Fused prediction (ops.predict_mask, csrc/predict.hip) against the unfused composition of the older ops
(ops.resize_bilinear_fwd -> lowest-index argmax -> table lookup), interleaved in one process.
    python scripts/bench_predict.py                  # kernel: B = 12, 168x168 -> 1024x1280 and 1080x1920, C in {2, 8}
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_predict.py --fused-only --size 1024x1280 --classes 8 --only mask
                                                     # kernel time of one variant (one process per variant)
    python scripts/bench_predict.py --script DIR     # + the predict entry point on 12 generated 1280x1024 frames: frames/s, PNG share
Medians of --reps timed windows of --iters calls each (device events), fused and unfused alternating and the order swapped every
window.  Output bytes: 1 B/px for the mask, + 3 B/px for the overlay; "moved" adds the frame (3 B/px) and the raw mask (1 B/px)
the optional outputs read.  The logit map is not counted: it is read from cache."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def lowest_argmax(r):
    C = r.shape[-1]
    idx = torch.arange(C, device=r.device).expand(r.shape)
    return torch.where(r == r.max(-1, keepdim=True).values, idx, torch.full_like(idx, C)).min(-1).values


def window(f, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def kernel(dev, reps, iters, B=12, h=168, sizes=((1024, 1280), (1080, 1920)), classes=(2, 8), only=None, fused_only=False):
    from adaptersis_amd import ops
    from adaptersis_amd.tools import frame_resize as F
    print(f"{'shape':34s} {'outputs':10s} {'fused us':>9s} {'out GB/s':>9s} {'moved GB/s':>10s} {'unfused us':>11s} {'argmax=torch us':>16s} {'ratio':>6s}")
    for H, W in sizes:
        for C in classes:
            g = torch.Generator().manual_seed(C)
            lg = (3 * torch.randn((B, h, h, C), generator=g)).to(dev)
            enc = torch.from_numpy(F.ENCODE_ENDOVIS2017[:C].copy()).to(dev)
            frames = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
            raw = (torch.randint(0, C, (B, H, W), generator=g, dtype=torch.uint8) * 32).to(dev)
            lut = torch.from_numpy(F.LUT_MULTI.copy()).to(dev)
            px = B * H * W

            def unfused():
                return enc[lowest_argmax(ops.resize_bilinear_fwd(lg, H, W))]

            def unfused_torch():          # torch.argmax in place of the spelled-out lowest index: the cheapest unfused form
                return enc[ops.resize_bilinear_fwd(lg, H, W).argmax(-1)]
            assert torch.equal(ops.predict_mask(lg, (H, W), enc), unfused())
            forms = (("mask", lambda: ops.predict_mask(lg, (H, W), enc), 1, 1),
                     ("+overlay", lambda: ops.predict_mask(lg, (H, W), enc, frames=frames), 4, 7),
                     ("+counts", lambda: ops.predict_mask(lg, (H, W), enc, target=raw, lut=lut), 1, 2))
            for what, fused, out_b, moved_b in forms:
                if only is not None and what != only:
                    continue
                if fused_only:                 # one variant alone under a kernel trace: its kernel time is the trace's average
                    for _ in range(reps * iters):
                        fused()
                    torch.cuda.synchronize()
                    print(f"B={B} {h}x{h} -> {H}x{W} C={C} {what}: {reps * iters} fused calls", flush=True)
                    continue
                for f in (fused, unfused, unfused_torch):
                    for _ in range(3):
                        f()
                torch.cuda.synchronize()
                tf, tu, tt = [], [], []
                for r in range(reps):
                    order = ((fused, tf), (unfused, tu), (unfused_torch, tt))
                    for f, acc in (order if r % 2 == 0 else order[::-1]):
                        acc.append(window(f, iters))
                mf, mu, mt = statistics.median(tf), statistics.median(tu), statistics.median(tt)
                print(f"B={B} {h}x{h} -> {H}x{W} C={C:<2d}       {what:10s} {mf:9.1f} {px * out_b / mf / 1e3:9.1f} {px * moved_b / mf / 1e3:10.1f} "
                      f"{mu:11.1f} {mt:16.1f} {mu / mf:6.1f}   (fused min {min(tf):.1f} max {max(tf):.1f})", flush=True)


def make_frames(root, n=12, hw=(1024, 1280)):
    from PIL import Image
    rng = np.random.default_rng(0)
    d = os.path.join(root, "Test", "instrument_dataset_1")
    if os.path.isdir(os.path.join(d, "images")) and len(os.listdir(os.path.join(d, "images"))) == n:
        return
    os.makedirs(os.path.join(d, "images"), exist_ok=True)
    os.makedirs(os.path.join(d, "instruments_masks"), exist_ok=True)
    for k in range(n):
        lab = rng.integers(0, 8, (hw[0] // 64, hw[1] // 64)).repeat(64, 0).repeat(64, 1)
        img = np.clip(lab[..., None] * np.array([29, 71, 113]) % 256 + rng.integers(-20, 21, hw + (3,)), 0, 255)
        Image.fromarray(img.astype(np.uint8)).save(os.path.join(d, "images", f"frame{k:03d}.png"))
        Image.fromarray((lab * 32).astype(np.uint8)).save(os.path.join(d, "instruments_masks", f"frame{k:03d}.png"))


def script(root, out):
    """The entry point end to end on 12 frames of 1280x1024 (vit_large, 588, MLA head, 8 classes; the checkpoint is a freshly
    initialised decoder, which costs what a trained one costs)."""
    from adaptersis_amd import predict as P
    from adaptersis_amd import train as T
    base = ["--imsize", "588", "--batch_size_per_gpu", "12", "--output_dir", out, "--head", "mla", "--num_classes", "8", "--seed", "0"]
    args = P.get_args_parser().parse_args(base + ["--input", root, "--dataset", "endovis2017", "--split", "Test", "--encode",
                                                  "endovis2017", "--pred_dir", os.path.join(out, "pred"), "--masks"])
    os.makedirs(out, exist_ok=True)
    torch.manual_seed(0)
    _, _, _, _, dec = T.build_modules(args, "mla", 8, torch.device("cuda", 0))
    torch.save({"epoch": 0, "state_dict": {"module." + k: v.cpu() for k, v in dec.state_dict().items()}},
               os.path.join(out, "checkpoint.pth.tar"))
    del dec
    eng = P.build_engine(args)
    for tag, extra in (("masks+metrics", []), ("masks+metrics+overlay", ["--overlay"])):
        a = P.get_args_parser().parse_args(base + ["--input", root, "--dataset", "endovis2017", "--split", "Test", "--encode",
                                                   "endovis2017", "--pred_dir", os.path.join(out, "pred_" + tag), "--masks"] + extra)
        P.predict_seg(a, engine=eng)          # warm-up: code objects, tables
        r = P.predict_seg(a, engine=eng)
        print(f"predict entry point, 12 x 1280x1024, {tag}: {r['frames_per_second']:.2f} frames/s ({r['seconds']:.2f} s); PNG encoding "
              f"{r['encode_seconds']:.2f} worker-s on {P.MAX_WRITERS} threads = {100 * r['encode_seconds'] / P.MAX_WRITERS / r['seconds']:.0f} % "
              f"of the wall per thread; {r['drain_seconds']:.2f} s waiting for the writers after the last batch", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--size", default=None, help="HxW: this output size only")
    ap.add_argument("--classes", type=int, default=None, help="this class count only")
    ap.add_argument("--only", default=None, choices=("mask", "+overlay", "+counts"), help="this output form only")
    ap.add_argument("--fused-only", action="store_true",
                    help="launch only the fused op (with --size / --classes / --only: one variant per process, for "
                         "rocprofv3 --kernel-trace --stats, whose statistics are per kernel name)")
    ap.add_argument("--script", default=None, help="directory for the generated frames and the outputs of the entry point")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    kw = {}
    if a.size:
        kw["sizes"] = (tuple(int(v) for v in a.size.split("x")),)
    if a.classes:
        kw["classes"] = (a.classes,)
    kernel(dev, a.reps, a.iters, only=a.only, fused_only=a.fused_only, **kw)
    if a.script:
        make_frames(os.path.join(a.script, "tree"))
        script(os.path.join(a.script, "tree"), os.path.join(a.script, "out"))
