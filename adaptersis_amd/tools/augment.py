"""Training-time augmentation on the GPU — the albumentations pipeline of `train.py:139-163`, which the reference runs on
uint8 numpy images inside its DataLoader workers (`tools/dataset.py:150-161`), as ONE HIP kernel per batch
(`csrc/augment.hip`) behind a host-side parameter sampler.  At ~70 ms per 12-image step a CPU pipeline (PIL decode +
albumentations ≈ 15-25 ms per 588x588 image per worker) is the next bottleneck.

What the reference composes (albumentations, version unpinned in `README.md:12`; semantics restated from its 1.x sources):

    OneOf([RandomSizedCrop(min_max_height=(294, 588), height=588, width=588, p=0.5),
           PadIfNeeded(588, 588, border_mode=BORDER_CONSTANT)], p=1)        -> crop with prob 0.5 / (0.5 + 1.0) = 1/3, else no-op
    HorizontalFlip(p=0.5); RandomRotate90(p=0.5)
    OneOf([ElasticTransform, GridDistortion, OpticalDistortion], p=0)       -> never applied (``non_rigid_p``: the switch the
                                                                               reference comments out, `#p=0.8 if ... else 0`)
    CLAHE(p=0.8); RandomBrightnessContrast(p=0.8); RandomGamma(p=0.8)

Built here: crop + cv2.resize back to S x S (INTER_LINEAR, 8-bit fixed-point form; mask INTER_NEAREST), flip, rot90,
CLAHE (OpenCV's 8-bit RGB <-> Lab integer paths + tiled contrast-limited equalisation of L on the 8 x 8 grid, clip limit
~ U(1, 4): ``tools/clahe.py`` + the ``asis_clahe`` kernels), brightness/contrast and gamma as uint8 look-up tables (exactly how
albumentations applies them to uint8 images), float / 255.  A batch with CLAHE samples runs three kernels (the tile histograms
need the whole geometrically transformed image), a batch without any runs the single fused one.
The random draws come from this module's own ``numpy`` generator — the same distributions, not albumentations' stream.

Non-rigid block (``non_rigid_p`` > 0; ``csrc/nonrigid.hip``): each member is a resample through a coordinate map, so a batch
with such a sample runs geometric stage -> map (Q5 fixed point, 1/32 pixel) -> integer bilinear remap (reflect-101) -> the CLAHE
kernels, whose per-sample flag switches CLAHE off while the tables and / 255 still apply.  Restated from albumentations 1.x
(``elastic_transform``, ``grid_distortion``, ``optical_distortion``) and OpenCV 4.x (``remap``, ``initUndistortRectifyMap``)
as published; neither library can be run here, so parity is unpinned as for CLAHE.  Stated deviations: the elastic member's
``warpAffine`` + ``remap`` are composed into ONE resample (one interpolation instead of two); its noise is this project's Philox
stream, not numpy's; the mask is sampled at the rounded QUANTISED coordinate (OpenCV rounds the float map).

Strong view (``strong=dict(...)``; ``csrc/strongaug.hip``, ``ops.strong_view``): the student's view of FixMatch / UniMatch-style
training, a second stage on the fp32 output of ``ops.augment`` — colour jitter (brightness, contrast, saturation, hue in a drawn
order, p = 0.8), greyscale (p = 0.2), Gaussian blur (p = 0.5, sigma ~ U(0.1, 2), radius max(1, ceil(3 sigma)) <= 6, reflect
border).  These are torchvision's tensor semantics (``ColorJitter``, ``RandomGrayscale``, ``gaussian_blur``) restated as published;
torchvision cannot be run here, so parity is unpinned in the same sense as for CLAHE and the non-rigid block.  Stated deviations:
the blur radius follows ceil(3 sigma) with a cap of 6 instead of a fixed kernel size, and the blurred value is clamped to [0,1].
The draws come from a generator of their own, so the base stream is the same with and without the block.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .. import ops
from . import clahe as _clahe

COEF_BITS = 11   # OpenCV INTER_RESIZE_COEF_BITS


def _round_half_even(x: np.ndarray) -> np.ndarray:
    return np.rint(x)          # cvRound: round to nearest, ties to even


def resize_tables(src0: int, src_len: int, dst_len: int, full: int):
    """OpenCV ``resize`` (INTER_LINEAR, 8U) coordinate tables for one axis of a crop [src0, src0+src_len) of an axis of
    ``full`` pixels resized to ``dst_len``: (ofs int32 [dst], coef int16 [dst, 2], nearest int32 [dst])."""
    scale = float(src_len) / float(dst_len)                        # double
    d = np.arange(dst_len, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)               # fx = (float)((dx+0.5)*scale_x - 0.5)
    s = np.floor(f).astype(np.int32)
    f = f - s.astype(np.float32)
    lo = s < 0
    f[lo] = 0.0
    s[lo] = 0
    hi = s >= src_len - 1
    f[hi] = 0.0
    s[hi] = src_len - 1
    one = np.float32(1.0)
    scale_c = np.float32(1 << COEF_BITS)
    a0 = np.clip(_round_half_even((one - f) * scale_c), -32768, 32767).astype(np.int16)
    a1 = np.clip(_round_half_even(f * scale_c), -32768, 32767).astype(np.int16)
    near = np.minimum(np.floor(d * scale).astype(np.int32), src_len - 1)   # INTER_NEAREST: sx = min(floor(dx*scale), ssize-1)
    return (s + src0).astype(np.int32), np.stack([a0, a1], -1), (near + src0).astype(np.int32)


def brightness_contrast_lut(alpha: float, beta: float) -> np.ndarray:
    """albumentations ``_brightness_contrast_adjust_uint`` (brightness_by_max=True): lut = clip(arange*alpha + beta*255)."""
    lut = np.arange(0, 256, dtype=np.float32)
    if alpha != 1:
        lut *= np.float32(alpha)
    if beta != 0:
        lut += np.float32(beta * 255.0)
    return np.clip(lut, 0, 255).astype(np.uint8)


def gamma_lut(gamma: float) -> np.ndarray:
    """albumentations ``gamma_transform`` on uint8: table = (arange/255)**gamma * 255 (truncated), applied with cv2.LUT."""
    return (np.power(np.arange(0, 256, dtype=np.float64) / 255.0, gamma) * 255.0).astype(np.uint8)


# ---- non-rigid block: host tables ------------------------------------------------------------------------------------
NR_NONE, NR_ELASTIC, NR_GRID, NR_OPTICAL = 0, 1, 2, 3
NR_RMAX = 64      # largest Gauss radius of asis_nonrigid_map


def gauss_table(sigma: float) -> np.ndarray:
    """scipy ``gaussian_filter`` kernel (``_gaussian_kernel1d``, truncate = 4): radius int(4 sigma + 0.5), weights
    exp(-i^2 / 2 sigma^2) / sum, computed in float64 -> fp32 [2 r + 1]."""
    r = int(4.0 * float(sigma) + 0.5)
    if r > NR_RMAX:
        raise ValueError(f"gauss_table: sigma {sigma} needs radius {r} > {NR_RMAX}")
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (float(sigma) * float(sigma)) * x * x)
    return (w / w.sum()).astype(np.float32)


def grid_table(S: int, num_steps: int, steps) -> np.ndarray:
    """One axis of albumentations ``grid_distortion``: the source coordinate of every output index, float64 [S].  The loop as
    published, quirks included: ``step = S // num_steps`` segments of ``np.linspace(prev, cur, end - start)`` (both ends, so a
    join repeats a value); the last segment is pinned to ``S`` only when it overruns, so where ``step`` divides ``S`` the table
    ends wherever the steps add up to, above or below ``S``."""
    step = S // num_steps
    xx = np.zeros(S, np.float64)
    prev = 0.0
    for idx in range(num_steps + 1):
        start = idx * step
        end = start + step
        if end > S:
            end, cur = S, float(S)
        else:
            cur = prev + step * float(steps[idx])
        xx[start:end] = np.linspace(prev, cur, max(end - start, 0))
        prev = cur
    return xx


def elastic_affine(S: int, pts) -> np.ndarray:
    """albumentations ``elastic_transform``: M = cv2.getAffineTransform(pts1, pts1 + pts) around the centre square; returns
    the INVERSE map A float64 [2, 3] (what ``warpAffine`` samples through), source = A (x, y, 1)."""
    c, s = float(S // 2), float(S // 3)
    pts1 = np.array([[c + s, c + s], [c + s, c - s], [c - s, c - s]], np.float64)
    pts2 = pts1 + np.asarray(pts, np.float64)
    P = np.concatenate([pts1, np.ones((3, 1))], 1)
    M = np.eye(3)
    M[:2] = np.linalg.solve(P, pts2).T
    return np.linalg.inv(M)[:2]


def weak_params(params):
    """The draws ``params`` with the photometric stage neutralised (no CLAHE, identity brightness / contrast / gamma tables, no
    strong view) and the geometry kept (crop, flip, rot90, the non-rigid member and its draws): the teacher's view in mean-teacher
    training.  Draws without a strong configuration carry no ``strong`` key and gain none."""
    return [{**p, "clahe": None, "alpha": 1.0, "beta": 0.0, "gamma": None, **({"strong": None} if "strong" in p else {})} for p in params]


# ---- strong view: host tables ----------------------------------------------------------------------------------------
ST_BRIGHTNESS, ST_CONTRAST, ST_SATURATION, ST_HUE = 0, 1, 2, 3
ST_RMAX = 6       # largest blur radius of asis_strong_view
ST_SEED = 0x5354524F
STRONG_DEFAULTS = {"jitter": (0.5, 0.5, 0.5, 0.25), "jitter_p": 0.8, "grey_p": 0.2, "blur_p": 0.5, "sigma": (0.1, 2.0)}


def strong_radius(sigma: float) -> int:
    return min(ST_RMAX, max(1, int(np.ceil(3.0 * float(sigma)))))


def strong_gauss(sigma: float, r: int) -> np.ndarray:
    """weights exp(-i^2 / 2 sigma^2), |i| <= r, normalised to sum 1 in float64 -> fp32 [2 ST_RMAX + 1], centred, zero outside +-r"""
    i = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 * i * i / (float(sigma) * float(sigma)))
    out = np.zeros(2 * ST_RMAX + 1, np.float32)
    out[ST_RMAX - r:ST_RMAX + r + 1] = (w / w.sum()).astype(np.float32)
    return out


def _strong_config(strong) -> dict:
    if not isinstance(strong, dict) or set(strong) - set(STRONG_DEFAULTS):
        raise ValueError(f"TrainAugment: strong must be None or a dict with keys out of {sorted(STRONG_DEFAULTS)}")
    cfg = {**STRONG_DEFAULTS, **strong}
    jit, sig = tuple(float(v) for v in cfg["jitter"]), tuple(float(v) for v in cfg["sigma"])
    if len(jit) != 4 or not all(0.0 <= v <= 1.0 for v in jit[:3]) or not 0.0 <= jit[3] <= 0.5:
        raise ValueError("TrainAugment: strong jitter is (brightness, contrast, saturation, hue) with the first three in [0, 1] "
                         "and hue in [0, 0.5]")
    if len(sig) != 2 or not 0.0 < sig[0] <= sig[1]:
        raise ValueError("TrainAugment: strong sigma is (low, high) with 0 < low <= high")
    for k in ("jitter_p", "grey_p", "blur_p"):
        if not 0.0 <= float(cfg[k]) <= 1.0:
            raise ValueError(f"TrainAugment: strong {k} must be a probability in [0, 1]")
    return {"jitter": jit, "sigma": sig, "jitter_p": float(cfg["jitter_p"]), "grey_p": float(cfg["grey_p"]), "blur_p": float(cfg["blur_p"])}


class TrainAugment:
    def __init__(self, size: int = 588, seed: int = 0, crop_p: float = 0.5, pad_p: float = 1.0, flip_p: float = 0.5,
                 rot_p: float = 0.5, clahe_p: float = 0.8, bc_p: float = 0.8, gamma_p: float = 0.8,
                 min_crop: Optional[int] = None, clahe_clip=(1.0, 4.0), non_rigid_p: float = 0.0,
                 elastic=(120.0, 6.0, 3.6), grid=(5, 0.3), optical=(2.0, 0.5), strong: Optional[dict] = None):
        if size < 16:
            raise ValueError("TrainAugment: size must be at least 16 (8 x 8 CLAHE tile grid)")
        # A.ElasticTransform(alpha, sigma, alpha_affine), A.GridDistortion(num_steps, distort_limit),
        # A.OpticalDistortion(distort_limit, shift_limit): `train.py:151-158`, members' p = 0.5, 0.5, 1
        self.non_rigid_p, self.elastic, self.grid, self.optical = float(non_rigid_p), tuple(elastic), tuple(grid), tuple(optical)
        self._gauss = gauss_table(self.elastic[1])
        self.size = size
        self.clahe_p, self.clahe_clip = clahe_p, clahe_clip        # A.CLAHE(clip_limit=4.0) -> clip ~ U(1, 4), tiles (8, 8)
        self.min_crop = int(size * 0.5) if min_crop is None else min_crop      # min_max_height=(int(588*0.5), 588)
        self.p_crop = crop_p / (crop_p + pad_p)                                # OneOf normalises its members' p
        self.flip_p, self.rot_p, self.bc_p, self.gamma_p = flip_p, rot_p, bc_p, gamma_p
        self.rng = np.random.RandomState(seed)
        # the strong view (None: no draw, no key): a generator of its own, so that the base stream does not depend on the block
        self.strong = None if strong is None else _strong_config(strong)
        self.strong_rng = None if strong is None else np.random.RandomState((int(seed) ^ ST_SEED) & 0xFFFFFFFF)

    # ---- parameter draws (host) -----------------------------------------------------------------------------------
    def draw(self, n: int):
        """-> list of per-sample dicts (crop box or None, flip, rotk, nonrigid: None or the member's draws, clahe, alpha, beta,
        gamma), drawn in the pipeline's order.  With a strong configuration also ``strong``: None, or the draws of that stage."""
        S, r = self.size, self.rng
        out = []
        for _ in range(n):
            p: Dict = {"crop": None, "flip": False, "rotk": 0, "nonrigid": None, "clahe": None, "alpha": 1.0, "beta": 0.0,
                       "gamma": None}
            if r.random_sample() < self.p_crop:
                ch = int(r.randint(self.min_crop, S + 1))          # random.randint(min, max), both inclusive
                cw = ch                                            # w2h_ratio = 1.0
                hs, ws = r.random_sample(), r.random_sample()
                y1 = int((S - ch + 1) * hs)                        # get_random_crop_coords
                x1 = int((S - cw + 1) * ws)
                p["crop"] = (x1, y1, cw, ch)
            p["flip"] = bool(r.random_sample() < self.flip_p)
            if r.random_sample() < self.rot_p:
                p["rotk"] = int(r.randint(0, 4))
            if self.non_rigid_p > 0:                               # at 0 the stream of draws is the one without the block
                p["nonrigid"] = self._draw_nonrigid()
            if r.random_sample() < self.clahe_p:
                p["clahe"] = float(r.uniform(*self.clahe_clip))
            if r.random_sample() < self.bc_p:
                p["alpha"] = 1.0 + r.uniform(-0.2, 0.2)
                p["beta"] = 0.0 + r.uniform(-0.2, 0.2)
            if r.random_sample() < self.gamma_p:
                p["gamma"] = r.uniform(80, 120) / 100.0
            if self.strong is not None:
                p["strong"] = self._draw_strong()
            out.append(p)
        return out

    def _draw_strong(self):
        """-> None (the sample keeps its pixels) or {"order": the four operation codes in the drawn order or None, "factors": their
        factors in that order, "grey": bool, "sigma": float or None}"""
        r, c = self.strong_rng, self.strong
        d = {"order": None, "factors": None, "grey": False, "sigma": None}
        if r.random_sample() < c["jitter_p"]:
            b, ct, s, h = c["jitter"]
            f = {ST_BRIGHTNESS: r.uniform(1.0 - b, 1.0 + b), ST_CONTRAST: r.uniform(1.0 - ct, 1.0 + ct),
                 ST_SATURATION: r.uniform(1.0 - s, 1.0 + s), ST_HUE: r.uniform(-h, h)}
            d["order"] = tuple(int(v) for v in r.permutation(4))
            d["factors"] = tuple(float(f[o]) for o in d["order"])
        d["grey"] = bool(r.random_sample() < c["grey_p"])
        if r.random_sample() < c["blur_p"]:
            d["sigma"] = float(r.uniform(*c["sigma"]))
        return d if d["order"] is not None or d["grey"] or d["sigma"] is not None else None

    def strong_tables(self, params, device, apply=None) -> Dict:
        """The tables of ``ops.strong_view`` for the draws ``params`` (``p.get("strong")`` absent or None = the sample keeps its
        pixels): st_ops int32 [B,4] (codes in the drawn order, -1 none), st_fac fp32 [B,4], st_flags int32 [B,2] (grey, radius),
        st_gauss fp32 [B,13] (centred, zero outside +-r), st_apply int32 [B] (``apply``: a sequence of B truth values; default all
        1), packed on the host and uploaded in ONE non-blocking copy; the host flags strong_any, contrast_any, blur_any (over the
        samples ``apply`` leaves on) and ``st_host``, the host copies the op checks its values on."""
        B, G = len(params), 2 * ST_RMAX + 1
        if apply is not None and len(apply) != B:
            raise ValueError(f"strong_tables: apply has {len(apply)} entries, the batch has {B} samples")
        cuda = torch.device(device).type == "cuda"
        stage = torch.zeros(B * (4 + 4 + 2 + G + 1), dtype=torch.int32, pin_memory=cuda)
        cut = np.cumsum([0, 4 * B, 4 * B, 2 * B, G * B, B])
        names, shapes = ("st_ops", "st_fac", "st_flags", "st_gauss", "st_apply"), ((B, 4), (B, 4), (B, 2), (B, G), (B,))
        part = lambda t, k: t[cut[k]:cut[k + 1]].view(torch.float32 if names[k] in ("st_fac", "st_gauss") else torch.int32).view(shapes[k])
        host = {n: part(stage, k) for k, n in enumerate(names)}
        ops_, fac, flags, gauss, app = (host[n].numpy() for n in names)
        ops_[:] = -1
        app[:] = 1 if apply is None else [int(bool(a)) for a in apply]
        for b, p in enumerate(params):
            st = p.get("strong")
            if st is None:
                continue
            if st["order"] is not None:
                ops_[b], fac[b] = st["order"], st["factors"]
            if st["sigma"] is not None:
                r = strong_radius(st["sigma"])
                flags[b, 1], gauss[b] = r, strong_gauss(st["sigma"], r)
            flags[b, 0] = int(st["grey"])
        on = app != 0
        dev = stage.to(device, non_blocking=True)
        out = {n: part(dev, k) for k, n in enumerate(names)}
        out["st_host"] = host
        out["contrast_any"] = bool(((ops_ == ST_CONTRAST).any(1) & on).any())
        out["blur_any"] = bool(((flags[:, 1] > 0) & on).any())
        out["strong_any"] = bool((((ops_ >= 0).any(1) | (flags != 0).any(1)) & on).any())
        return out

    def _draw_nonrigid(self):
        """albumentations ``OneOf``: with probability ``non_rigid_p`` one member, by the members' normalised p (1/4, 1/4, 1/2)."""
        r = self.rng
        if not r.random_sample() < self.non_rigid_p:
            return None
        u = r.random_sample()
        if u < 0.25:
            seed = (int(r.randint(0, 1 << 32, dtype=np.uint64)) << 32) | int(r.randint(0, 1 << 32, dtype=np.uint64))
            aa = self.elastic[2]
            return {"kind": "elastic", "seed": seed, "pts": r.uniform(-aa, aa, size=(3, 2))}
        if u < 0.5:
            n, lim = int(self.grid[0]), self.grid[1]
            return {"kind": "grid", "xsteps": 1.0 + r.uniform(-lim, lim, size=n + 1), "ysteps": 1.0 + r.uniform(-lim, lim, size=n + 1)}
        d, sh = self.optical
        k = float(r.uniform(-d, d))
        # shift_limit = 0.5: Python's round() of U(-0.5, 0.5) is always 0, as in the reference; the draw is kept
        return {"kind": "optical", "k": k, "dx": round(r.uniform(-sh, sh)), "dy": round(r.uniform(-sh, sh))}

    def nonrigid_tables(self, params, device) -> Dict[str, torch.Tensor]:
        """The tables of ``asis_nonrigid_map`` for the draws ``params`` (``p.get("nonrigid")`` absent or None = kind none)."""
        S, B = self.size, len(params)
        kind = np.zeros(B, np.int32)
        par = np.zeros((B, 8), np.float32)
        seed = np.zeros(B, np.uint64)
        gx = np.zeros((B, S), np.float32); gy = np.zeros((B, S), np.float32)
        for b, p in enumerate(params):
            nr = p.get("nonrigid")
            if nr is None:
                continue
            if nr["kind"] == "elastic":
                kind[b] = NR_ELASTIC
                par[b, 0] = self.elastic[0]
                par[b, 1:7] = elastic_affine(S, nr["pts"]).reshape(-1)
                seed[b] = np.uint64(int(nr["seed"]) & 0xFFFFFFFFFFFFFFFF)
            elif nr["kind"] == "grid":
                kind[b] = NR_GRID
                gx[b] = grid_table(S, int(self.grid[0]), nr["xsteps"])
                gy[b] = grid_table(S, int(self.grid[0]), nr["ysteps"])
            elif nr["kind"] == "optical":
                kind[b] = NR_OPTICAL
                par[b, :3] = (nr["k"], nr["dx"], nr["dy"])
            else:
                raise ValueError(f"TrainAugment: unknown non-rigid kind {nr['kind']!r}")
        t = dict(nr_kind=kind, nr_par=par, nr_seed=seed.view(np.int64), nr_gx=gx, nr_gy=gy, nr_gauss=self._gauss)
        return {k: torch.from_numpy(v).to(device, non_blocking=True) for k, v in t.items()}

    def tables(self, params, device) -> Dict[str, torch.Tensor]:
        S = self.size
        B = len(params)
        geo = np.zeros((B, 4), np.int32)
        xofs = np.zeros((B, S), np.int32); yofs = np.zeros((B, S), np.int32)
        xa = np.zeros((B, S, 2), np.int16); ya = np.zeros((B, S, 2), np.int16)
        mx = np.zeros((B, S), np.int32); my = np.zeros((B, S), np.int32)
        lut = np.zeros((B, 256), np.uint8)
        clahe = np.zeros((B, 2), np.int32)
        for b, p in enumerate(params):
            if p.get("clahe") is not None:
                clahe[b] = (1, _clahe.clip_limit_int(p["clahe"], S))
            geo[b] = (int(p["flip"]), p["rotk"], int(p["crop"] is None), 0)
            if p["crop"] is not None:
                x1, y1, cw, ch = p["crop"]
                xofs[b], xa[b], mx[b] = resize_tables(x1, cw, S, S)
                yofs[b], ya[b], my[b] = resize_tables(y1, ch, S, S)
            l = np.arange(256, dtype=np.uint8)
            if p["alpha"] != 1.0 or p["beta"] != 0.0:
                l = brightness_contrast_lut(p["alpha"], p["beta"])[l]
            if p["gamma"] is not None:
                l = gamma_lut(p["gamma"])[l]
            lut[b] = l
        t = dict(geo=geo, xofs=xofs, yofs=yofs, xa=xa, ya=ya, mx=mx, my=my, lut=lut, clahe=clahe)
        out = {k: torch.from_numpy(v).to(device, non_blocking=True) for k, v in t.items()}
        out["clahe_any"] = bool(clahe[:, 0].any())      # host flag: no CLAHE sample -> the single fused kernel
        out["nonrigid_any"] = any(p.get("nonrigid") is not None for p in params)   # host flag: none -> today's launches
        if out["nonrigid_any"]:
            out.update(self.nonrigid_tables(params, device))
        return out

    def __call__(self, img_u8: torch.Tensor, mask_u8: torch.Tensor, params=None, return_params: bool = False,
                 return_strong: bool = False, strong_apply=None):
        """uint8 [B,S,S,3] + uint8 [B,S,S] on the device -> (fp32 [B,3,S,S] in [0,1], int64 [B,S,S]); ``return_params`` appends the
        parameters used (the ones drawn when ``params`` is None).  Parameters that carry strong draws (a strong configuration, or
        ``params`` with ``strong`` entries) make the image the strong view (``ops.strong_view``, out of place; ``strong_apply``: the
        samples it is applied to); ``return_strong`` then appends the pre-strong tensor last (the image itself without a draw)."""
        if params is None:
            params = self.draw(img_u8.shape[0])
        x, m = ops.augment(img_u8, mask_u8, self.tables(params, img_u8.device))
        out, pre = (x, m), x
        if any(p.get("strong") is not None for p in params):
            out = (ops.strong_view(x, self.strong_tables(params, img_u8.device, strong_apply)), m)
        out = (*out, params) if return_params else out
        return (*out, pre) if return_strong else out
