"""Plain-torch restatement of the fused segmentation loss with an ignore label (include/asis_semi.h), written for the tests of
libasis_semi.so; float64 is the reference, float32 the yardstick of the bounds (tests/test_gpu_loss_kernels.py's scheme).

With g the ignore value: v_i = [t_i != g], n_b = sum_{i in b} v_i, sample b present when n_b > 0, P = the present samples.
  sums      I = sum v q t, Sp = sum v q, St = sum v t per (b, c), q = softmax^{n_region}(resize(logits))
  region    the five formulas of loss.hip per (b, c), the mean over the P*C pairs of the present samples; P = 0: exactly 0
  CE        sum v w_t nll / sum v w_t on level n_ce - 1; a denominator of 0: exactly 0
  dz        d loss / d resized logits times ``gs`` by autograd: 0 on every ignored pixel, nothing is NaN
Labels other than g must lie in 0..C-1 here (the kernels' treatment of other labels is the parent kernels' and is not restated)."""
import torch
import torch.nn.functional as F


def semi_ref(lg, tg, g, n_region, mode, eps, n_ce, wts, dtype, gs=1024.0):
    """-> dict of loss, sums [B, C, 3], valid [B], dz [B, H, W, C] (times gs), and what the bounds need: D, A (over the valid
    pixels), kappa, rho, rho_ce, mean |term| over the present pairs, |CE|"""
    B, h, w, C = lg.shape
    H, W = tg.shape[1:]
    v = tg != g
    tcl = torch.where(v, tg, torch.zeros_like(tg))
    assert int(tcl.min()) >= 0 and int(tcl.max()) < C
    x0 = F.interpolate(lg.to(dtype).permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False).requires_grad_()
    x1 = torch.softmax(x0, 1)
    lv = [x0, x1, torch.softmax(x1, 1)]
    vq = v.unsqueeze(1).to(dtype)
    t = F.one_hot(tcl, C).permute(0, 3, 1, 2).to(dtype) * vq
    q = lv[n_region]
    I, Sp, St = (q * t).sum((2, 3)), (q * vq).sum((2, 3)), t.sum((2, 3))
    valid = v.sum((1, 2))
    present = valid > 0
    P = int(present.sum())
    e = float(torch.tensor(eps, dtype=torch.float32))
    zero = x0.sum() * 0
    Ip, Spp, Stp = I[present], Sp[present], St[present]          # [P, C]: an absent sample has no term
    if mode == 0:
        term = 2 * Ip / (Spp + Stp + e)
    elif mode == 1:
        term = (Ip + e) / (Spp + Stp - Ip + e)
    elif mode == 2:
        term = (2 * Ip + e) / (Spp + Stp + e)
    elif mode == 3:
        term = (Ip + e) / (Ip + 0.3 * (Spp - Ip) + 0.7 * (Stp - Ip) + e)
    else:
        term = Ip * 0
    if P == 0 or mode == 4:
        region = zero
    elif mode in (0, 1):
        region = 1 - term.sum() / (P * C)
    else:
        region = -term.sum() / (P * C)
    wv = torch.ones(C, dtype=dtype) if wts is None else wts.to(dtype)
    wpix = wv[tcl] * v.to(dtype)
    ce = zero
    if n_ce and float(wpix.sum()) > 0:
        nll = F.cross_entropy(lv[n_ce - 1], tcl, reduction="none")
        ce = (wpix * nll).sum() / wpix.sum()
    loss = region + ce
    (loss * gs).backward()
    d, qd = x0.detach(), q.detach()
    kap, rho = 1.0, 0.0
    for s, a, a2 in ((I, (qd.abs() * t).sum((2, 3)), (qd * qd * t).sum((2, 3))),
                     (Sp, (qd.abs() * vq).sum((2, 3)), (qd * qd * vq).sum((2, 3)))):
        nz = s.detach() != 0
        if bool(nz.any()):
            rho = max(rho, float((a2[nz].sqrt() / a[nz]).max()))
            if n_region == 0:
                kap = max(kap, float((a[nz] / s.detach()[nz].abs()).max()))
    dv = d.permute(0, 2, 3, 1)[v]                                  # [valid pixels, C]
    w64 = wpix.double()
    return dict(loss=loss.detach(), sums=torch.stack([I, Sp, St], -1).detach(), valid=valid, dz=x0.grad.permute(0, 2, 3, 1),
                D=float((dv.amax(1) - dv.amin(1)).max()) if dv.numel() else 0.0, A=float(dv.abs().max()) if dv.numel() else 0.0,
                kappa=kap, rho=rho, rho_ce=float(w64.pow(2).sum().sqrt() / w64.sum()) if float(w64.sum()) > 0 else 0.0,
                term=float(term.detach().abs().mean()) if P else 0.0, ce=abs(float(ce.detach())), P=P)


PATTERNS = ("none", "rand30", "sample0", "all", "onepix", "oneclass", "zero_w")


def ignore_pattern(tg, pattern, g, gen):
    """the target of a case: ``tg`` (labels in 0..C-1) with the pixels of ``pattern`` set to ``g``.
    none: nothing; rand30: a random 30 % of the pixels; sample0: sample 0 wholly; all: every pixel; onepix: all but one pixel of the
    batch (in the last sample); oneclass: all but the pixels of class 0; zero_w: all but the pixels of class 1 (the class
    ``_loss_inputs`` gives the CE weight 0)."""
    out = tg.clone()
    if pattern == "none":
        return out
    if pattern == "rand30":
        out[torch.rand(tg.shape, generator=gen) < 0.3] = g
    elif pattern == "sample0":
        out[0] = g
    elif pattern == "all":
        out[:] = g
    elif pattern == "onepix":
        y, x = int(torch.randint(0, tg.shape[1], (1,), generator=gen)), int(torch.randint(0, tg.shape[2], (1,), generator=gen))
        keep = out[-1, y, x].clone()
        out[:] = g
        out[-1, y, x] = keep
    elif pattern in ("oneclass", "zero_w"):
        out[tg != (0 if pattern == "oneclass" else 1)] = g
    else:
        raise ValueError(pattern)
    return out.contiguous()
