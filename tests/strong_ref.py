"""The strong student view restated in plain torch: colour jitter (brightness, contrast, saturation, hue in a drawn order),
random greyscale, Gaussian blur — the yardstick of tests/test_strong_host.py and tests/test_gpu_strong.py.  It acts on the output of
``ops.augment`` (``[B,3,H,W]`` in [0,1]) and reads the tables of ``tools.augment.TrainAugment.strong_tables``.

The formulas are torchvision's tensor semantics as published (``adjust_brightness`` / ``_contrast`` / ``_saturation`` / ``_hue`` with
``_rgb2hsv`` / ``_hsv2rgb`` in the max / min form and its ``where`` guards, ``rgb_to_grayscale``, ``gaussian_blur`` with a reflect
border).  torchvision cannot be run here, so parity with it is unpinned, as for CLAHE and the non-rigid block.  Stated deviation:
the blurred value is clamped to [0,1] as well (the fp32 weights sum to 1 only within their roundings).

Every function takes ``dtype``: float64 is the reference; the same code in float32 measures what the number format alone costs."""
import numpy as np
import torch

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3
GREY = (0.2989, 0.587, 0.114)
RMAX = 6


def grey(x):
    """[...,3,H,W] -> [...,H,W]"""
    return GREY[0] * x[..., 0, :, :] + GREY[1] * x[..., 1, :, :] + GREY[2] * x[..., 2, :, :]


def brightness(x, f):
    return (x * f).clamp(0.0, 1.0)


def contrast(x, f, mean=None):
    """``mean``: the mean grey value of the sample as it stands (computed here when None)"""
    m = grey(x).mean() if mean is None else mean
    return (f * x + (1.0 - f) * m).clamp(0.0, 1.0)


def saturation(x, f):
    return (f * x + (1.0 - f) * grey(x).unsqueeze(-3)).clamp(0.0, 1.0)


def rgb2hsv(x):
    r, g, b = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    maxc, minc = x.max(dim=-3).values, x.min(dim=-3).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    hr = (maxc == r) * (bc - gc)
    hg = ((maxc == g) & (maxc != r)) * (2.0 + rc - bc)
    hb = ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = torch.fmod((hr + hg + hb) / 6.0 + 1.0, 1.0)
    return h, s, maxc


def hsv2rgb(h, s, v):
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int64) % 6
    p = (v * (1.0 - s)).clamp(0.0, 1.0)
    q = (v * (1.0 - s * f)).clamp(0.0, 1.0)
    t = (v * (1.0 - s * (1.0 - f))).clamp(0.0, 1.0)
    table = (((v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)))
    out = []
    for c in range(3):
        ch = torch.zeros_like(v)
        for k in range(6):
            ch = torch.where(i == k, table[k][c], ch)
        out.append(ch)
    return torch.stack(out, dim=-3)


def hue(x, f):
    h, s, v = rgb2hsv(x)
    return hsv2rgb(torch.remainder(h + f, 1.0), s, v)


def to_grey(x):
    return grey(x).unsqueeze(-3).expand_as(x).clone()


def reflect_index(n: int, r: int) -> np.ndarray:
    """source index of every position of an axis of ``n`` padded by ``r`` on both sides, reflect border (no edge repeat; r < n)"""
    i = np.arange(-r, n + r)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur(x, w, r: int):
    """separable correlation of ``x`` [...,H,W] with the taps ``w`` [2 r + 1] along both axes, reflect border"""
    H, W = x.shape[-2:]
    if r >= min(H, W):
        raise ValueError(f"blur: radius {r} needs an image larger than {r} on both axes")
    w = torch.as_tensor(w, dtype=x.dtype)
    xp = x[..., :, torch.from_numpy(reflect_index(W, r))]
    x = sum(w[k] * xp[..., :, k:k + W] for k in range(2 * r + 1))
    xp = x[..., torch.from_numpy(reflect_index(H, r)), :]
    return sum(w[k] * xp[..., k:k + H, :] for k in range(2 * r + 1))


def jitter(x, ops, fac, upto_contrast: bool = False):
    """one sample [3,H,W] through the operations ``ops`` (codes; -1 = none) with the factors ``fac``, in order.
    ``upto_contrast``: stop in front of the contrast operation (the image whose grey mean contrast uses)."""
    for op, f in zip(ops, fac):
        op, f = int(op), float(f)
        if op == OP_CONTRAST and upto_contrast:
            break
        if op == OP_BRIGHTNESS:
            x = brightness(x, f)
        elif op == OP_CONTRAST:
            x = contrast(x, f)
        elif op == OP_SATURATION:
            x = saturation(x, f)
        elif op == OP_HUE:
            x = hue(x, f)
    return x


def _host(tables, name):
    return tables[name].detach().cpu().numpy()


def strong_view(x, tables, apply=None, dtype=torch.float64):
    """``x`` [B,3,H,W] -> the strong view, evaluated in ``dtype`` on the CPU"""
    ops, fac, flags, gauss = (_host(tables, k) for k in ("st_ops", "st_fac", "st_flags", "st_gauss"))
    out = x.detach().cpu().to(dtype).clone()
    for b in range(out.shape[0]):
        if apply is not None and not int(apply[b]):
            continue
        v = jitter(out[b], ops[b], fac[b])
        if flags[b, 0]:
            v = to_grey(v)
        r = int(flags[b, 1])
        if r > 0:
            v = blur(v, gauss[b, RMAX - r:RMAX + r + 1].astype(np.float64), r).clamp(0.0, 1.0)
        out[b] = v
    return out


def contrast_mean(x, tables, b: int, dtype=torch.float64):
    """the mean grey value contrast uses for sample ``b`` (None without a contrast operation)"""
    ops, fac = _host(tables, "st_ops")[b], _host(tables, "st_fac")[b]
    if OP_CONTRAST not in ops.tolist():
        return None
    return float(grey(jitter(x[b].detach().cpu().to(dtype), ops, fac, upto_contrast=True)).mean())
