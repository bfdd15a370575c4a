"""Float64 reference of the hard-pixel losses for the tests (CPU, plain torch; nothing of adaptersis_amd is used here): the
per-pixel values v_i of the top-k cross entropy and of the focal loss in closed form, their gradients, the stable top-K, the
loss and dz — and the error bounds the tests of both precisions share (u = 2^-24, one rounding to float32).

Bounds, for ANY float32 evaluation whose exp / log / pow are good to 1 ulp = 2 u (torch on the CPU and csrc/hardpixel.hip alike):
  cross entropy  nll = log(sum_c exp(z_c - m)) - (z_t - m), A = max |z|: the two differences move by 2 A u each, a term of the
                 sum by (2 A + 2) u of itself, the chain of C - 1 adds by (C - 1) u, the log by 2 u ln C, the last difference
                 by u |nll|:  |nll - nll64| <= ce_bound = u (4 A + 2 C + 4 + 2 |nll|)  (3 ln C <= C + 3); times |w|, plus u |v|
                 for that product (inside the 2 |nll|).  Inputs off by dz in the sup norm (the resize): 2 dz more (logsumexp
                 and z_t are 1-Lipschitz).
  focal          pt = sum_c o_c q_c + smooth, o >= 0: C products, C adds: (C + 2) u pt, plus the error dq of q itself times
                 sum o <= 1 + smooth, plus u for the rounding of 1 - pt:  dpt = (C + 2) u pt + u + (1 + smooth) dq.
                 v(pt) = -w max(1 - pt, 0)^gamma log pt and its derivative c(pt) = w (gamma b^(gamma-1) log pt - b^gamma / pt) are
                 monotone in pt on (0, 1] for gamma = 0 and gamma >= 1 (every factor's magnitude falls as pt grows), so an
                 argument off by dpt moves them by at most the larger of the two end-point differences, `interval`; the
                 operations on top (pow 2 u (+ gamma u through b), log 2 u, three products, a difference) add
                 (gamma + 8) u times the sum of the magnitudes of the terms.  pt - dpt <= 0: no bound (infinity).
  softmax        a probability is off by E(D, C) ulps (lovasz_ref.softmax_ulps, derived in test_gpu_loss_kernels for the
                 kernels' __expf; torch's is tighter), plus 2 dz of itself for inputs off by dz.
  sums           a float32 sum of n terms in any order: n u sum |terms|; the kernels sum in double: 2 u |result| for the one
                 rounding at the end.
  soft dice      (2 I + s) / (Sp + St + s) per (b, c), -mean: I and Sp are sums of n = H W probabilities, each off by E_q u
                 relative, summed with n u: a ratio <= 1 moves by 2 (E_q + n + 2) u, the mean of B C of them by B C u more:
                 dice_bound = (2 E_q + 2 n + 4 + B C) u, E_q = 2 softmax_ulps.  Its gradient at z: the coefficient d loss / d q_c
                 of a (b, c) is relative 3 (E_q + n + 2) u off (numerator once, denominator twice), the softmax transpose
                 q_c (g_c - <g, q>) carries q three times and a dot product over C: per element
                 (3 (E_q + n + 2) + 3 E_q + C + 4) u * 2 * sum_j |coef_j|."""
import math

import torch
import torch.nn.functional as F

from tests.lovasz_ref import ULP24, prob_bound, resized64, softmax_ulps  # noqa: F401  (re-exported for the tests)

U = ULP24
CE, FOCAL = 0, 1


def onehot_row(C: int, smooth: float):
    """(o_hit, o_miss): the one-hot row after torch.clamp(., smooth / (C - 1), 1 - smooth), evaluated in float32"""
    if not smooth:
        return 1.0, 0.0
    s = torch.tensor(smooth, dtype=torch.float32)
    lo, hi = s / torch.tensor(float(C - 1), dtype=torch.float32), torch.tensor(1.0, dtype=torch.float32) - s
    one, zero = torch.tensor(1.0), torch.tensor(0.0)
    return float(torch.minimum(torch.maximum(one, lo), hi)), float(torch.minimum(torch.maximum(zero, lo), hi))


def alpha_vector(alpha, C: int, balance_index: int = 0):
    """`focal_loss.py:51-63` in float32 on the host (the same operations: the same bits); None = ones"""
    if alpha is None:
        return torch.ones(C)
    if isinstance(alpha, float):
        a = torch.ones(C) * (1 - alpha)
        a[balance_index] = alpha
        return a
    a = torch.tensor(list(alpha), dtype=torch.float32)
    return a / a.sum()


def _focal_terms(pt, gamma):
    """pt float64 -> (b^gamma, d b^gamma / d b, log pt) with b = max(1 - pt, 0); the derivative is 0 where gamma = 0 or b = 0"""
    b = (1.0 - pt).clamp_min(0.0)
    pw = torch.ones_like(pt) if gamma == 0 else b ** gamma
    dpw = torch.zeros_like(pt) if gamma == 0 else torch.where(b > 0, gamma * b.clamp_min(1e-300) ** (gamma - 1.0), torch.zeros_like(pt))
    return pw, dpw, pt.log()


def focal_v(pt, gamma):
    pw, _, lg = _focal_terms(pt, gamma)
    return -pw * lg


def focal_c(pt, gamma):
    pw, dpw, lg = _focal_terms(pt, gamma)
    return dpw * lg - pw / pt


def pixel_values(z, labels, kind, *, n_softmax=0, gamma=2.0, smooth=1e-5, weight=None):
    """z float64 [N, C] (the resized logits or probabilities), labels int64 [N] -> (v float64 [N], dv float64 [N, C] = d v_i / d z_i,
    aux dict for the bounds).  A label outside 0..C-1: v = 0, dv = 0."""
    N, C = z.shape
    ok = (labels >= 0) & (labels < C)
    t = labels.clamp(0, C - 1)
    w = (torch.ones(C, dtype=torch.float64) if weight is None else weight.double())[t]
    hot = F.one_hot(t, C).double()
    if kind == CE:
        nll = torch.logsumexp(z, -1) - z.gather(1, t.view(-1, 1)).squeeze(1)
        v = w * nll
        dv = w.view(-1, 1) * (torch.softmax(z, -1) - hot)
        aux = {"nll": nll, "w": w}
    else:
        q = torch.softmax(z, -1) if n_softmax else z
        hit, miss = onehot_row(C, smooth)
        o = hot * hit + (1.0 - hot) * miss
        pt = (o * q).sum(-1) + float(torch.tensor(smooth or 0.0, dtype=torch.float32))
        v = w * focal_v(pt, gamma)
        c = w * focal_c(pt, gamma)
        g = c.view(-1, 1) * o
        dv = q * (g - (g * q).sum(-1, keepdim=True)) if n_softmax else g
        aux = {"pt": pt, "w": w, "o": o, "q": q}
    v = torch.where(ok, v, torch.zeros_like(v))
    dv = torch.where(ok.view(-1, 1), dv, torch.zeros_like(dv))
    aux["ok"] = ok
    return v, dv, aux


def stable_topk(values: torch.Tensor, K: int) -> torch.Tensor:
    """bool [N]: the K largest, ties by ascending index (-0 == +0)"""
    idx = torch.sort(values, descending=True, stable=True).indices[:K]
    sel = torch.zeros(values.numel(), dtype=torch.bool)
    sel[idx] = True
    return sel


def loss_and_dz(v, dv, sel, K, size_average=True, grad_scale=1.0):
    """-> (loss, dz [N, C]) of the selected set"""
    f = 1.0 / K if size_average else 1.0
    return v[sel].sum() * f, dv * sel.view(-1, 1).double() * (f * grad_scale)


def ce_bound(A: float, C: int, nll: torch.Tensor) -> torch.Tensor:
    return U * (4.0 * A + 2.0 * C + 4.0 + 2.0 * nll.abs())


def interval(f, pt, dpt, gamma):
    """max |f(pt +- dpt) - f(pt)| for monotone f; infinity where pt - dpt <= 0"""
    lo, hi = pt - dpt, pt + dpt
    safe = lo > 0
    lo = torch.where(safe, lo, pt)
    d = torch.maximum((f(lo, gamma) - f(pt, gamma)).abs(), (f(hi, gamma) - f(pt, gamma)).abs())
    return torch.where(safe, d, torch.full_like(d, math.inf))


def focal_bounds(aux, gamma, smooth, C, dq=0.0):
    """-> (bound of v [N], bound of the coefficient w c(pt) [N]) for a float32 evaluation whose q is off by <= dq"""
    pt, w = aux["pt"], aux["w"].abs()
    dpt = (C + 2) * U * pt.abs() + U + (1.0 + (smooth or 0.0)) * dq
    pw, dpw, lg = _focal_terms(pt, gamma)
    bv = w * (interval(focal_v, pt, dpt, gamma) + (gamma + 8) * U * (pw * lg).abs())
    bc = w * (interval(focal_c, pt, dpt, gamma) + (gamma + 8) * U * ((dpw * lg).abs() + (pw / pt).abs()))
    zero = ~aux["ok"]
    return torch.where(zero, torch.zeros_like(bv), bv), torch.where(zero, torch.zeros_like(bc), bc)


def soft_dice(z_nhwc, labels, smooth=1.0):
    """SoftDiceLoss(apply_nonlin=softmax, smooth) of float64 logits [B,H,W,C]: -> (loss, d loss / d z [B,H,W,C], coef [B,H,W,C] =
    d loss / d q)"""
    z = z_nhwc.detach().clone().requires_grad_(True)
    q = torch.softmax(z, -1)
    q.retain_grad()
    B, H, W, C = z.shape
    hot = F.one_hot(labels.clamp(0, C - 1), C).double() * ((labels >= 0) & (labels < C)).unsqueeze(-1)
    I, Sp, St = (q * hot).sum((1, 2)), q.sum((1, 2)), hot.sum((1, 2))
    loss = -((2 * I + smooth) / (Sp + St + smooth)).mean()
    loss.backward()
    return loss.detach(), z.grad.detach(), q.grad.detach()


def dice_bounds(z_nhwc, coef):
    """-> (bound of the loss, bound of d loss / d z per element [B,H,W,C])"""
    B, H, W, C = z_nhwc.shape
    D = float((z_nhwc.max(-1).values - z_nhwc.min(-1).values).max())
    Eq, n = 2.0 * softmax_ulps(D, C), H * W
    d1 = coef.abs().sum(-1, keepdim=True).expand_as(coef)
    return (2 * Eq + 2 * n + 4 + B * C) * U, (3 * (Eq + n + 2) + 3 * Eq + C + 4) * U * 2.0 * d1
