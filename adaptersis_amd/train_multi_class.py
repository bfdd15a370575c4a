"""Drop-in for the reference's `train_multi_class.py`: the `train_mla.py` pipeline (DecoderMLA, lr * batch * world / 16,
momentum 0.9, no weight decay) on ``EndoVis2017(task="multi")`` with the soft-IoU loss (`:393`, engine loss "iou") and
``ch_iou`` / ``isi_iou`` in validation (`:583-597`, from the validation kernel's per-class pixel counts).

    python -m adaptersis_amd.train_multi_class --arch vit_large --imsize 588 --batch_size_per_gpu 12 \
        --data_path /data/endovis2017 --num_classes 8 --output_dir /tmp/out

Where the reference cannot run as written: its encoder ``SpatialPriorModule`` is undefined (``FeatureEncoder``
here, as in `train_mla.py`); it builds ``DecoderMLA(num_classes=2)`` but calls ``iou_loss`` with its default of 8 classes
(``--num_classes``, default 8, feeds both); ``--cross_test_path`` is used but never declared (default: ``--data_path``); its
validation cross-entropy weight ``[0.1, 10]`` raises for C != 2 (kept for C = 2, no weight otherwise).
Added: ``--dataset``, ``--task``, ``--problem_type`` (of ``isi_iou``) and ``--resize_on`` (frame resize on the device, the
default, or PIL on the host: identical bytes).  ``--data_path synthetic`` trains on ``W.synthetic_batch(..., num_classes)``.
"""
from __future__ import annotations

import contextlib
import functools

import torch

from . import parallel
from . import train as _t
from . import train_mla as _mla
from .segloss import iou_multi
from .utils import misc as utils

train = _t.train

DATASETS = ("endovis2017", "endovis2018", "autolapro", "robomis")
# (train split, validation split) per dataset: the reference validates EndoVis2017 on "Test" (`train_multi_class.py:129`)
SPLITS = {"endovis2017": ("Train", "Test"), "endovis2018": ("Train", "Test"), "autolapro": ("Train", "Validation"),
          "robomis": ("training", "validation")}


def _task(args) -> str:
    task = args.task or ("multi" if args.dataset == "endovis2017" else "binary")
    if task == "multi" and args.dataset != "endovis2017":
        raise ValueError(f"--task multi: {args.dataset} has binary masks only (only endovis2017 has instruments_masks)")
    return task


def open_datasets(args):
    """-> (train set, val set, collate_fn) for ``--dataset`` (validation on ``--cross_test_path``), or the synthetic set."""
    if args.data_path == "synthetic":
        C = args.num_classes
        return (_t._SegData(args.data_path, "train", args.imsize, num_classes=C),
                _t._SegData(args.data_path, "validation", args.imsize, num_classes=C), None)
    from .tools import dataset as D
    test_path = args.cross_test_path or args.data_path
    tr, va = SPLITS[args.dataset]
    if args.dataset == "robomis":
        return (D.Robomis(args.data_path, tr, transform=None, imsize=args.imsize),
                D.Robomis(test_path, va, transform=None, imsize=args.imsize), D.collate_u8)
    kw = dict(transform=None, imsize=args.imsize, resize_on_gpu=args.resize_on == "gpu")
    if args.dataset == "endovis2017":
        kw["task"] = _task(args)
    cls = {"endovis2017": D.EndoVis2017, "endovis2018": D.EndoVis2018, "autolapro": D.Autolapro}[args.dataset]
    ds_train, ds_val = cls(args.data_path, tr, **kw), cls(test_path, va, **kw)
    return ds_train, ds_val, ds_train.collate_fn


def _val_meters():
    """``train._val_meters`` plus ch_iou / isi_iou: all five created up front on every rank (the ``--shard_val`` hang fix)."""
    ml = utils.MetricLogger(delimiter="  ")
    for name in ("loss", "acc1", "dice", "ch_iou", "isi_iou"):
        ml.meters[name]
    return ml


def _val_summary(ml) -> str:
    return ("* Acc@1 {top1.global_avg:.3f} loss {losses.global_avg:.3f} Dice {dice.global_avg:.3f} Ch_iou {ch_iou.global_avg:.3f} "
            "ISI_iou {isi_iou.global_avg:.3f}").format(top1=ml.acc1, losses=ml.loss, dice=ml.meters["dice"],
                                                        ch_iou=ml.meters["ch_iou"], isi_iou=ml.meters["isi_iou"])


@torch.no_grad()
def validate_network(val_loader, model, feature_model, backbone_encoder, cross_vit, cross_cnn, seg_decoder, n, avgpool,
                     problem_type="instruments"):
    """`train_multi_class.py:410-602`: `train.validate_network` + per-batch ch_iou / isi_iou of argmax(logits) against the
    labels (from the per-class counts of ``ops.ce_acc``); CE weight [0.1, 10] for C = 2, none otherwise."""
    engine = _t._engine_for(model, backbone_encoder, cross_vit, cross_cnn, seg_decoder)
    metric_logger = _val_meters()
    dev = next(seg_decoder.parameters()).device
    wt = torch.tensor([0.1, 10.0], device=dev) if engine.num_classes == 2 else None
    sharded = isinstance(getattr(val_loader, "batch_sampler", None), _t.BatchShardSampler)
    with (parallel.local_batchnorm() if sharded else contextlib.nullcontext()):
        for (inp, target, idx) in metric_logger.log_every(val_loader, 20, "Test:"):
            inp, target = _t._to_device_batch(inp, target, train=False)
            m, dloss, counts = engine.validate_step(inp, target, wt, with_counts=True)
            m, counts = m.cpu(), counts.cpu()
            bs = inp.shape[0]
            metric_logger.update(loss=float(m[0] / m[1]))
            metric_logger.meters["acc1"].update(float(m[2]) / target.numel(), n=bs)
            metric_logger.meters["dice"].update(1.0 - float(dloss), n=bs)
            metric_logger.meters["ch_iou"].update(float(iou_multi.ch_iou_from_counts(counts)), n=bs)
            metric_logger.meters["isi_iou"].update(float(iou_multi.isi_iou_from_counts(counts, problem_type)), n=bs)
    if sharded:
        metric_logger.synchronize_between_processes()
    print(_val_summary(metric_logger))
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def train_seg(args):
    if args.cross_test_path is None:
        args.cross_test_path = args.data_path
    if args.data_path != "synthetic":
        _task(args)   # argument errors before any model is built
    return _t.train_seg(args, head="mla", num_classes=args.num_classes, loss=getattr(args, "loss", "iou"), open_datasets=open_datasets,
                        validate=functools.partial(validate_network, problem_type=args.problem_type))


def get_args_parser():
    p = _mla.get_args_parser()
    p.description = "Multi-class segmentation on EndoVis2017 (train_multi_class.py)"
    p.set_defaults(loss="iou")   # train_multi_class.py:390-393
    p.add_argument("--num_classes", default=8, type=int, help="classes of the MLA head and of the soft-IoU loss")
    p.add_argument("--cross_test_path", default=None, type=str, help="root of the validation split (default: --data_path)")
    p.add_argument("--dataset", default="endovis2017", choices=DATASETS)
    p.add_argument("--task", default=None, choices=("multi", "binary"),
                   help="endovis2017 masks: instruments_masks (multi, the default) or binary_masks; the others are binary")
    p.add_argument("--problem_type", default="instruments", choices=("instruments", "parts", "binary"), help="of isi_iou")
    p.add_argument("--resize_on", default="gpu", choices=("gpu", "host"),
                   help="frame resize to --imsize on the device (ops.frame_resize) or with PIL in the loader: identical bytes")
    return p


if __name__ == "__main__":
    train_seg(get_args_parser().parse_args())
