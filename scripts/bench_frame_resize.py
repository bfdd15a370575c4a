"""On-device frame resize (ops.frame_resize, csrc/frame_resize.hip) and the two loader routes of the EndoVis datasets.
    python scripts/bench_frame_resize.py                 # kernel: B = 12, 1280x1024 and 960x540 -> 588, us and GB/s
    python scripts/bench_frame_resize.py --loader DIR    # + loader CPU ms per item per route on a generated 1280x1024 PNG tree
    python scripts/bench_frame_resize.py --script DIR    # + train_multi_class img/s per route (vit_large, 588, B = 12)
Bytes counted: frames and masks read once, the horizontal pass's uint8 intermediate written and read once, outputs written."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def kernel(dev, B=12, S=588):
    from adaptersis_amd import ops
    from adaptersis_amd.tools import frame_resize as F
    for H, W in ((1024, 1280), (540, 960)):
        g = torch.Generator().manual_seed(0)
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        msk = (torch.randint(0, 8, (B, H, W), generator=g, dtype=torch.uint8) * 32).to(dev)
        nbytes = B * (H * W * 4 + 2 * H * S * 3 + S * S * 4)
        for what, f in (("frames+masks", lambda: ops.frame_resize(img, msk, S, F.LUT_MULTI)),
                        ("frames", lambda: ops.frame_resize(img, None, S)),
                        ("masks", lambda: ops.frame_resize(None, msk, S, F.LUT_MULTI))):
            for _ in range(5):
                f()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(50):
                f()
            e.record(); torch.cuda.synchronize()
            us = s.elapsed_time(e) / 50 * 1e3
            nb = nbytes if what == "frames+masks" else (B * (H * W * 3 + 2 * H * S * 3 + S * S * 3) if what == "frames"
                                                        else B * (S * W + S * S))
            print(f"B={B} {W}x{H} -> {S}: {what:13s} {us:8.1f} us  {nb / us / 1e3:7.1f} GB/s (counted {nb / 1e6:.1f} MB)")


def make_tree(root, n_train=48, n_test=12, hw=(1024, 1280)):
    from PIL import Image
    rng = np.random.default_rng(0)
    for split, n in (("Train", n_train), ("Test", n_test)):
        d = os.path.join(root, split, "instrument_dataset_1")
        if os.path.isdir(os.path.join(d, "images")) and len(os.listdir(os.path.join(d, "images"))) == n:
            continue
        os.makedirs(os.path.join(d, "images"), exist_ok=True)
        os.makedirs(os.path.join(d, "instruments_masks"), exist_ok=True)
        for k in range(n):
            lab = rng.integers(0, 8, (hw[0] // 64, hw[1] // 64)).repeat(64, 0).repeat(64, 1)
            img = np.clip(lab[..., None] * np.array([29, 71, 113]) % 256 + rng.integers(-20, 21, hw + (3,)), 0, 255)
            Image.fromarray(img.astype(np.uint8)).save(os.path.join(d, "images", f"frame{k:03d}.png"))
            Image.fromarray((lab * 32).astype(np.uint8)).save(os.path.join(d, "instruments_masks", f"frame{k:03d}.png"))


def loader(root, S=588, n=24):
    from adaptersis_amd.tools import dataset as D
    for route in ("host", "gpu"):
        ds = D.EndoVis2017(root, "Train", imsize=S, task="multi", resize_on_gpu=route == "gpu")
        ds[0]
        t = time.process_time()
        items = [ds[i % len(ds)] for i in range(n)]
        t_items = time.process_time() - t
        t = time.process_time()
        for k in range(0, n, 12):
            ds.collate_fn(items[k:k + 12])
        t_col = time.process_time() - t
        print(f"loader {route:4s}: {(t_items + t_col) / n * 1e3:6.1f} CPU ms per item (decode + resize + table + collate)")


def script(root, out, S=588, B=12):
    from adaptersis_amd import train as T
    from adaptersis_amd import train_multi_class as TMC
    inner = T.train
    for route in ("host", "gpu"):
        times = []

        def timed(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            r = inner(*a, **k)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t)
            return r
        T.train = timed
        args = TMC.get_args_parser().parse_args(["--imsize", str(S), "--batch_size_per_gpu", str(B), "--epochs", "2",
                                                 "--data_path", root, "--num_workers", "10", "--val_freq", "100",
                                                 "--output_dir", os.path.join(out, route), "--resize_on", route])
        T._ENGINES.clear()
        n = len(TMC.open_datasets(args)[0])
        TMC.train_seg(args)
        T.train = inner
        print(f"train_multi_class --resize_on {route}: {n / times[-1]:.1f} img/s (second epoch, {n} images, B={B}, {S}x{S})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--loader", default=None, help="directory for the generated PNG tree")
    ap.add_argument("--script", default=None, help="directory for the generated PNG tree (+ outputs)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    kernel(dev)
    for d in (a.loader, a.script):
        if d:
            make_tree(os.path.join(d, "tree"))
    if a.loader:
        loader(os.path.join(a.loader, "tree"))
    if a.script:
        script(os.path.join(a.script, "tree"), os.path.join(a.script, "out"))
