"""Score mask PNGs that ``adaptersis_amd.predict`` (or anything else) wrote: no model, no checkpoint.

    python -m adaptersis_amd.score --pred_dir /tmp/pred --input /data/endovis2017 --dataset endovis2017 --split Test \
        --encode endovis2017 --num_classes 8 --surface 1 2 5
    python -m adaptersis_amd.score --pred_dir pred/ --masks labels/ --encode binary255 --num_classes 2

The ground truth is paired with the predictions as ``predict`` pairs it with the frames (``predict._Frames``): the dataset's own
masks with ``--dataset --input --split``, otherwise a directory ``--masks`` mirroring ``--pred_dir``.  The PNGs are batched by size
(``predict.plan_batches``), uploaded as uint8, and everything is counted on the device by ``ops.surface_stats``: the region
counts of ``metrics.json`` (per-class IoU, mean IoU, pixel accuracy) are its inter / n_pred / n_lab columns summed over the
frames, and with ``--surface`` the boundary metrics are added under ``"surface"``, exactly as ``predict --masks --surface`` writes
them.  ``<pred_dir>/metrics.json`` is (over)written."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np
import torch

from . import predict as _p
from .tools import frame_resize as _fr


def get_args_parser():
    p = argparse.ArgumentParser("adaptersis_amd.score", description=__doc__.split("\n\n")[0])
    p.add_argument("--pred_dir", required=True, type=str, help="mask PNGs (<stem>.png; <stem>_overlay.png files are ignored)")
    p.add_argument("--masks", nargs="?", const="dataset", default=None,
                   help="directory mirroring --pred_dir; with --dataset the dataset's own masks are used (no value needed)")
    p.add_argument("--input", default=None, type=str, help="the dataset root, with --dataset")
    p.add_argument("--dataset", default=None, choices=_p.DATASETS)
    p.add_argument("--split", default=None, type=str)
    p.add_argument("--task", default=None, choices=("multi", "binary"))
    p.add_argument("--encode", default="index", choices=sorted(_fr.ENCODINGS), help="how the prediction PNGs encode the class")
    p.add_argument("--num_classes", default=2, type=int)
    p.add_argument("--imsize", default=224, type=int, help="unused by the scores (the datasets' constructors ask for one)")
    p.add_argument("--batch_size_per_gpu", default=12, type=int)
    p.add_argument("--surface", nargs="*", type=float, default=None, metavar="TAU",
                   help="boundary metrics at these tolerances (pixels); no value = "
                        + " ".join(f"{t:g}" for t in _p.DEFAULT_TOLERANCES))
    _p.add_hd_percentile(p)
    return p


class _Pairs:
    """(prediction PNG, raw ground truth) pairs: ``predict._Frames``' pairing with the predictions in the frames' place."""

    def __init__(self, args):
        from PIL import Image
        self._open = Image.open
        self.pred_dir = args.pred_dir
        if args.dataset is not None:
            if args.input is None:
                raise ValueError("--dataset needs --input (the dataset root)")
            args.masks = args.masks or "dataset"
            self.frames = _p._Frames(args)            # the dataset's frames, masks and label table
            self.stems = [os.path.splitext(r)[0] for r in self.frames.rel]
            self.lut = self.frames.lut
            self.sizes = self.frames.sizes
        else:
            if args.masks in (None, "dataset"):
                raise ValueError("--masks DIR (mirroring --pred_dir) or --dataset/--input/--split is required")
            if not os.path.isdir(args.pred_dir):
                raise FileNotFoundError(f"--pred_dir {args.pred_dir}: not a directory")
            self.frames = None
            rel = [r for r in _p.walk_frames(args.pred_dir) if not os.path.splitext(r)[0].endswith("_overlay")]
            if not rel:
                raise ValueError(f"no mask PNGs under {args.pred_dir}")
            self.stems = [os.path.splitext(r)[0] for r in rel]
            self.mask_files = [_p._Frames._mirror(args.masks, r) for r in rel]
            self.lut = _fr.ENCODINGS[args.encode][1]
            self.sizes = [_p._native_size(os.path.join(args.pred_dir, r)) for r in rel]

    def load(self, i: int):
        """-> (prediction uint8 [H,W], raw ground truth uint8 [H,W])."""
        path = os.path.join(self.pred_dir, self.stems[i] + ".png")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"--pred_dir {self.pred_dir}: no prediction {self.stems[i]}.png")
        with open(path, "rb") as f:
            pred = np.array(self._open(f).convert("L"), dtype=np.uint8)
        if self.frames is not None:
            mask = self.frames.load(i)[1]
        else:
            with open(self.mask_files[i], "rb") as f:
                mask = np.array(self._open(f).convert("L"), dtype=np.uint8)
        if mask.shape != pred.shape:
            raise ValueError(f"{path}: prediction {pred.shape} and ground truth {mask.shape} differ in size")
        return pred, np.ascontiguousarray(mask)


def score(args) -> dict:
    from . import ops
    from .segloss.surface import SurfaceMeter
    C = args.num_classes
    _fr.encode_table(args.encode, C)
    tol = [] if args.surface is None else ([float(t) for t in args.surface] or list(_p.DEFAULT_TOLERANCES))
    ops.surface_thresholds(tol)
    pct = _p.hd_percentiles(args)
    if not torch.cuda.is_available():
        raise RuntimeError("adaptersis_amd.score needs an MI355X (there is no CPU path)")
    pairs = _Pairs(args)
    meter = SurfaceMeter(C, tol, pct) if args.surface is not None else None
    pred_lut = _fr.ENCODINGS[args.encode][1]
    counts = np.zeros((C, 3), dtype=np.int64)
    for idx in _p.plan_batches(pairs.sizes, args.batch_size_per_gpu):
        items = [pairs.load(i) for i in idx]
        pred = torch.from_numpy(np.stack([it[0] for it in items])).cuda().contiguous()
        target = torch.from_numpy(np.stack([it[1] for it in items])).cuda().contiguous()
        out = [t.cpu().numpy() for t in ops.surface_stats(pred, target, C, tol, pred_lut=pred_lut, lut=pairs.lut, percentiles=pct)]
        counts += out[0][:, :, :3].sum(0)
        if meter is not None:
            meter.update(*out)
    metrics = _p.metrics_from_counts(counts)
    metrics["frames"] = len(pairs.stems)
    if meter is not None:
        metrics["surface"] = meter.result()
    with open(os.path.join(args.pred_dir, "metrics.json"), "w") as f:
        json.dump(metrics, f, indent=1, sort_keys=True)
    iou = " ".join("-" if v is None else f"{v:.4f}" for v in metrics["per_class_iou"])
    print(f"* IoU per class [{iou}]  mean IoU {metrics['mean_iou']}  pixel accuracy {metrics['pixel_accuracy']}")
    if meter is not None:
        print(_p.surface_line(metrics["surface"]))
    return metrics


def main(argv=None):
    return score(get_args_parser().parse_args(argv))


if __name__ == "__main__":
    main()
