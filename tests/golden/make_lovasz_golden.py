"""Writes tests/golden/lovasz_ref.pt: inputs, losses and gradients of the reference project's own ``LovaszSoftmax``
(`segloss/lovasz_loss.py`) on the CPU, in float32 (the reference's ``torch.dot`` mixes dtypes in any other precision).

    python tests/golden/make_lovasz_golden.py --reference /path/to/the/reference/checkout

The reference is imported from that path only while this script runs; none of its text is copied.

Per shape (B, h, w, C) the logits are ``randn`` (std 1) and the labels uniform from a seeded ``torch.Generator``; the seed is the
first one for which the minimal gap between the sorted keys |t - q| of every class is >= 1e-5 in float64 AND in float32.  With
gaps that wide the order is the same in every precision and the gradient unique, so the reference's unstable ``torch.sort``
cannot matter.  Recorded per case: seed, logits [B,h,w,C], target [B,h,w], probs [B,C,h,w] (float32 softmax, the reference's
input), loss_mean / loss_sum / loss_none, grad_mean / grad_sum = d loss / d probs [B,C,h,w]."""
import argparse
import os
import sys

import torch

SHAPES = [(2, 12, 10, 3), (1, 9, 7, 8), (2, 16, 16, 2)]
MIN_GAP = 1e-5


def min_key_gap(probs_nchw: torch.Tensor, target: torch.Tensor) -> float:
    """smallest difference between neighbouring sorted keys over all classes, in the dtype of ``probs``"""
    C = probs_nchw.shape[1]
    q = probs_nchw.permute(0, 2, 3, 1).reshape(-1, C)
    t = (target.reshape(-1, 1) == torch.arange(C).view(1, C)).to(q.dtype)
    keys = (t - q).abs().t()
    s = torch.sort(keys, dim=1).values
    return float((s[:, 1:] - s[:, :-1]).min())


def draw(shape, seed):
    B, h, w, C = shape
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, h, w, C), generator=gen, dtype=torch.float32)
    target = torch.randint(0, C, (B, h, w), generator=gen, dtype=torch.int64)
    return logits, target


def find_seed(shape, limit=10000):
    for seed in range(limit):
        logits, target = draw(shape, seed)
        z = logits.permute(0, 3, 1, 2)
        if min(min_key_gap(torch.softmax(z.double(), 1), target), min_key_gap(torch.softmax(z, 1), target)) >= MIN_GAP:
            return seed
    raise RuntimeError(f"no seed below {limit} for {shape}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds segloss/lovasz_loss.py)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "lovasz_ref.pt"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from segloss.lovasz_loss import LovaszSoftmax  # the reference's

    cases = []
    for shape in SHAPES:
        seed = find_seed(shape)
        logits, target = draw(shape, seed)
        probs = torch.softmax(logits.permute(0, 3, 1, 2), 1).contiguous()
        rec = {"shape": shape, "seed": seed, "logits": logits, "target": target, "probs": probs}
        for red in ("mean", "sum", "none"):
            p = probs.clone().requires_grad_(True)
            loss = LovaszSoftmax(reduction=red)(p, target)
            rec["loss_" + red] = loss.detach().clone()
            if red != "none":
                loss.backward()
                rec["grad_" + red] = p.grad.detach().clone()
        cases.append(rec)
        print(shape, "seed", seed, "loss_mean", float(rec["loss_mean"]))
    torch.save({"cases": cases}, a.out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
