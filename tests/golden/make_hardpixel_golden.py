"""Writes tests/golden/hardpixel_ref.pt: inputs, losses and gradients of the reference project's own ``TopKLoss``
(`segloss/ND_Crossentropy.py`), ``DC_and_topk_loss`` (`segloss/dice_loss.py`) and ``FocalLoss`` (`segloss/focal_loss.py`) on the
CPU, in float32.

    python tests/golden/make_hardpixel_golden.py --reference /path/to/the/reference/checkout

The reference is imported from that path only while this script runs; none of its text is copied.

Per shape (B, h, w, C) the logits are ``randn`` (std 1) and the labels uniform from a seeded ``torch.Generator``; the seed is the
first one for which the gap between the K-th and the (K+1)-th largest per-pixel cross entropy at k = 10 (K = int(N * 10 / 100))
is >= 1e-4 in float64 AND in float32: the selected set is then the same in every precision and ``torch.topk``'s arbitrary
choice among ties cannot matter.  Recorded per case: seed, K, logits [B,h,w,C], target [B,h,w], probs [B,C,h,w] (float32 softmax,
the focal loss's input), weight [C] (the class weights of "topk_w"), alpha_list (of "focal_list"), and per configuration of
CONFIGS ``loss_<name>`` and ``grad_<name>`` = d loss / d input [B,C,h,w]."""
import argparse
import os
import sys

import torch

SHAPES = [(2, 12, 10, 3), (1, 9, 7, 8), (2, 16, 16, 2)]
MIN_GAP = 1e-4
K_PERCENT = 10
# name -> (class, constructor arguments as written below, input: "logits" or "probs")
CONFIGS = ["topk", "topk_w", "dc_and_topk", "focal", "focal_float", "focal_list"]
FOCAL_FLOAT = dict(alpha=0.25, balance_index=1, gamma=1.5, size_average=False)


def kth_gap(logits_nhwc: torch.Tensor, target: torch.Tensor, K: int) -> float:
    """difference between the K-th and the (K+1)-th largest per-pixel cross entropy, in the dtype of ``logits``"""
    C = logits_nhwc.shape[-1]
    ce = torch.nn.functional.cross_entropy(logits_nhwc.reshape(-1, C), target.reshape(-1), reduction="none")
    s = torch.sort(ce, descending=True).values
    return float(s[K - 1] - s[K])


def draw(shape, seed):
    B, h, w, C = shape
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn((B, h, w, C), generator=gen, dtype=torch.float32)
    target = torch.randint(0, C, (B, h, w), generator=gen, dtype=torch.int64)
    weight = torch.rand((C,), generator=gen, dtype=torch.float32) + 0.5
    return logits, target, weight


def find_seed(shape, limit=10000):
    B, h, w, C = shape
    K = int(B * h * w * K_PERCENT / 100)
    for seed in range(limit):
        logits, target, _ = draw(shape, seed)
        if min(kth_gap(logits, target, K), kth_gap(logits.double(), target, K)) >= MIN_GAP:
            return seed
    raise RuntimeError(f"no seed below {limit} for {shape}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference checkout (holds segloss/)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "hardpixel_ref.pt"))
    a = ap.parse_args()
    sys.path.insert(0, a.reference)
    from segloss.ND_Crossentropy import TopKLoss  # the reference's
    from segloss.dice_loss import DC_and_topk_loss
    from segloss.focal_loss import FocalLoss

    cases = []
    for shape in SHAPES:
        B, h, w, C = shape
        seed = find_seed(shape)
        logits, target, weight = draw(shape, seed)
        z = logits.permute(0, 3, 1, 2).contiguous()
        probs = torch.softmax(z, 1).contiguous()
        alpha_list = [float(i + 1) for i in range(C)]
        rec = {"shape": shape, "seed": seed, "K": int(B * h * w * K_PERCENT / 100), "logits": logits, "target": target, "probs": probs,
               "weight": weight, "alpha_list": alpha_list}
        runs = {
            "topk": (TopKLoss(k=K_PERCENT), z),
            "topk_w": (TopKLoss(k=K_PERCENT, weight=weight), z),
            "dc_and_topk": (DC_and_topk_loss({}, {"k": K_PERCENT}), z),
            "focal": (FocalLoss(), probs),
            "focal_float": (FocalLoss(**FOCAL_FLOAT), probs),
            "focal_list": (FocalLoss(alpha=alpha_list, smooth=0), probs),
        }
        assert list(runs) == CONFIGS
        for name, (module, inp) in runs.items():
            x = inp.clone().requires_grad_(True)
            loss = module(x, target.unsqueeze(1))
            loss.backward()
            rec["loss_" + name], rec["grad_" + name] = loss.detach().clone(), x.grad.detach().clone()
            print(shape, "seed", seed, name, float(loss))
        cases.append(rec)
    torch.save({"cases": cases}, a.out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
