"""Float64 reference of the Lovasz-Softmax loss for the tests (CPU, plain torch; nothing of adaptersis_amd is used here).

``closed_form`` evaluates loss and gradient from a GIVEN order of GIVEN keys, so a test can hand it the device's own keys and
check the combinatorics exactly; ``reference_g`` is the reference formula (cumulative sums and differences of 1 - I/U)."""
import torch
import torch.nn.functional as F

ULP24 = 2.0 ** -24   # one rounding to float32, relative


def reference_g(flags_sorted: torch.Tensor) -> torch.Tensor:
    """`segloss/lovasz_loss.py:7-19` in float64."""
    gt = flags_sorted.double()
    gts = gt.sum()
    inter = gts - gt.cumsum(0)
    union = gts + (1.0 - gt).cumsum(0)
    jac = 1.0 - inter / union
    if gt.numel() > 1:
        jac[1:] = jac[1:] - jac[:-1]
    return jac


def closed_g(flags_sorted: torch.Tensor) -> torch.Tensor:
    """g from integer counts: class pixel 1/U, other I/(U(U-1)); no class pixel: g_0 = 1."""
    f = flags_sorted.to(torch.int64)
    G = int(f.sum())
    g = torch.zeros(f.numel(), dtype=torch.float64)
    if G == 0:
        g[0] = 1.0
        return g
    fk = f.cumsum(0)
    k1 = torch.arange(1, f.numel() + 1, dtype=torch.int64)
    I, U = (G - fk).double(), (G + (k1 - fk)).double()
    cls = f > 0
    g[cls] = 1.0 / U[cls]
    g[~cls] = I[~cls] / (U[~cls] * (U[~cls] - 1.0))
    return g


def stable_order(keys: torch.Tensor) -> torch.Tensor:
    """[C, N] -> int64 [C, N]: descending, ties by ascending index."""
    return torch.sort(keys, dim=1, descending=True, stable=True).indices


def closed_form(keys: torch.Tensor, labels: torch.Tensor, order: torch.Tensor):
    """keys float64 [C, N] (pixel order), labels int64 [N], order int64 [C, N] -> (per_class float64 [C],
    d float64 [N, C] = d loss_c / d q_c: -g class pixel, +g other, 0 where the key is 0)."""
    C, N = keys.shape
    per_class = torch.zeros(C, dtype=torch.float64)
    d = torch.zeros(N, C, dtype=torch.float64)
    for c in range(C):
        o = order[c]
        flags = (labels == c)[o]
        g = closed_g(flags)
        e = keys[c][o]
        per_class[c] = (e * g).sum()
        s = torch.where(flags, -1.0, 1.0).double()
        s[e == 0] = 0.0
        d[o, c] = s * g
    return per_class, d


def reduce(per_class: torch.Tensor, reduction: str):
    """-> (loss, gradient factor)"""
    C = per_class.numel()
    return (per_class.mean(), 1.0 / C) if reduction == "mean" else (per_class.sum(), 1.0)


def resized64(logits_nhwc: torch.Tensor, H: int, W: int, dtype=torch.float64) -> torch.Tensor:
    """NHWC logits -> resized NHWC in ``dtype`` (F.interpolate bilinear, align_corners=False)."""
    z = logits_nhwc.to(dtype).permute(0, 3, 1, 2)
    if tuple(z.shape[-2:]) != (H, W):
        z = F.interpolate(z, size=(H, W), mode="bilinear", align_corners=False)
    return z.permute(0, 2, 3, 1).contiguous()


def keys_of(q_nhwc: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """probabilities [B,H,W,C], labels [B,H,W] -> keys [C, N] = |t - q| in the dtype of q."""
    C = q_nhwc.shape[-1]
    q = q_nhwc.reshape(-1, C)
    t = (labels.reshape(-1, 1) == torch.arange(C).view(1, C)).to(q.dtype)
    return (t - q).abs().t().contiguous()


def softmax_ulps(D: float, C: int) -> float:
    """E(D, C) of tests/test_gpu_loss_kernels.py: the error of the kernels' softmax in ulps (2^-23) of a probability."""
    return 2.0 * (D + 1.0) + (C - 1) / 2.0 + 2.0


def prob_bound(logits_nhwc: torch.Tensor, H: int, W: int) -> float:
    """Absolute bound on |q_device - q_float64| for q = softmax(resize(logits)).  The resize: delta_z = max(4 Y, 4 ulp max|z|)
    as in test_gpu_loss_kernels (Y = torch's float32 resize against float64: the float32 source coordinate both share); a shift
    of the logits by at most delta_z moves a probability by at most exp(2 delta_z) - 1 ~ 2 delta_z of itself; then E(D, C)."""
    z64 = resized64(logits_nhwc, H, W)
    z32 = resized64(logits_nhwc, H, W, torch.float32).double()
    dz = max(4.0 * float((z32 - z64).abs().max()), 4.0 * 2.0 ** -23 * float(z64.abs().max()))
    if tuple(logits_nhwc.shape[1:3]) == (H, W):
        dz = 0.0   # identity resize: weights 1 and 0, exact
    D = float((z64.max(-1).values - z64.min(-1).values).max())
    return 2.0 * dz + softmax_ulps(D, logits_nhwc.shape[-1]) * 2.0 ** -23
