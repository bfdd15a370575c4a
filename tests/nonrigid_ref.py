"""numpy / float64 restatement of the non-rigid augmentation block (csrc/nonrigid.hip, adaptersis_amd/tools/augment.py) —
TEST INFRASTRUCTURE ONLY.  Holds the Philox generator, the elastic noise, the scipy-blurred displacement field, the three
maps, the Q5 quantisation and the integer remap.  Restated from albumentations 1.x / OpenCV 4.x as published; neither library
can be run here, so parity against them is unpinned (as for CLAHE in oracle/augment_ref.py): these numbers define the behaviour.
"""
import numpy as np

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11) with the round function of csrc/philox.h; arrays of uint32 values -> 4 x uint64 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & _MASK for c in (c0, c1, c2, c3))
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0, p1 = np.uint64(_M0) * c0, np.uint64(_M1) * c2            # 32 x 32 -> 64 bit: no overflow in uint64
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _MASK, p1 >> np.uint64(32), p1 & _MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(_W0)) & _MASK, (k1 + np.uint64(_W1)) & _MASK
    return c0, c1, c2, c3


def noise(seed: int, S: int) -> np.ndarray:
    """float64 [2, S, S]: n[f, y, x] = 2 U - 1, U = (w >> 8) 2^-24, w = word e & 3 of philox(counter (lo32(e >> 2), hi32(e >> 2),
    f, 0), key (lo32(seed), hi32(seed))), e = y S + x.  Every value is exactly representable in fp32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    e = np.arange(S * S, dtype=np.uint64)
    blk = e >> np.uint64(2)
    out = np.empty((2, S * S), np.float64)
    for f in range(2):
        words = np.stack(philox4x32_10(blk & _MASK, blk >> np.uint64(32), np.full_like(blk, f), np.zeros_like(blk),
                                       seed & 0xFFFFFFFF, seed >> 32), 0)
        w = words[(e & np.uint64(3)).astype(np.int64), np.arange(S * S)]
        out[f] = 2.0 * ((w >> np.uint64(8)).astype(np.float64) * 2.0 ** -24) - 1.0
    return out.reshape(2, S, S)


def gauss_kernel(sigma: float) -> np.ndarray:
    """scipy ``_gaussian_kernel1d`` (order 0, truncate 4), float64 [2 r + 1]."""
    r = int(4.0 * sigma + 0.5)
    x = np.arange(-r, r + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    return w / w.sum()


def reflect_half(i, S):
    """scipy mode='reflect' (d c b a | a b c d | d c b a), periodic with period 2 S."""
    m = np.mod(i, 2 * S)
    return np.where(m < S, m, 2 * S - 1 - m)


def reflect_101(i, S):
    """cv2.BORDER_REFLECT_101 (d c b | a b c d | c b a), periodic with period 2 (S - 1)."""
    P = 2 * S - 2
    m = np.mod(i, P)
    return np.where(m < S, m, P - m)


def blur_reflect(n: np.ndarray, w: np.ndarray) -> np.ndarray:
    """Separable correlation of a float64 [S, S] plane with the symmetric kernel ``w`` under the periodic half-sample reflection."""
    S, r = n.shape[0], len(w) // 2
    idx = reflect_half(np.arange(S)[:, None] + np.arange(-r, r + 1)[None, :], S)        # [S, 2 r + 1]
    rows = (n[:, idx] * w).sum(-1)                                                      # along x
    return (rows[idx] * w[None, :, None]).sum(1)                                        # along y


def field64(seed: int, S: int, alpha: float, sigma: float) -> np.ndarray:
    """alpha * scipy.ndimage.gaussian_filter(noise, sigma, mode='reflect'), float64 [2, S, S] = (dx, dy)."""
    from scipy.ndimage import gaussian_filter
    n = noise(seed, S)
    return alpha * np.stack([gaussian_filter(n[f], sigma, mode="reflect") for f in range(2)], 0)


def elastic_affine(S: int, pts) -> np.ndarray:
    """Inverse of cv2.getAffineTransform(pts1, pts1 + pts) with albumentations' centre square, float64 [2, 3]."""
    c, s = float(S // 2), float(S // 3)
    pts1 = np.array([[c + s, c + s], [c + s, c - s], [c - s, c - s]], np.float64)
    pts2 = pts1 + np.asarray(pts, np.float64)
    # M (x, y, 1)^T = pts2 for the three points: Cramer-free, by least squares on the 3 x 3 system
    M = np.eye(3)
    M[:2] = np.linalg.lstsq(np.concatenate([pts1, np.ones((3, 1))], 1), pts2, rcond=None)[0].T
    return np.linalg.inv(M)[:2]


def elastic_map64(S: int, field: np.ndarray, A: np.ndarray):
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    X, Y = x + field[0], y + field[1]
    return A[0, 0] * X + A[0, 1] * Y + A[0, 2], A[1, 0] * X + A[1, 1] * Y + A[1, 2]


def grid_axis(S: int, num_steps: int, steps) -> np.ndarray:
    """albumentations ``grid_distortion``, one axis, the loop as published; float64 [S]."""
    step = S // num_steps
    xx = np.zeros(S, np.float64)
    prev = 0.0
    for idx in range(num_steps + 1):
        x = idx * step
        start, end = int(x), int(x) + step
        if end > S:
            end = S
            cur = float(S)
        else:
            cur = prev + step * steps[idx]
        n = end - start
        for i in range(max(n, 0)):                                   # np.linspace(prev, cur, n), both ends included
            xx[start + i] = prev if n == 1 else prev + (cur - prev) * i / (n - 1)
        prev = cur
    return xx


def grid_map64(S: int, num_steps: int, xsteps, ysteps):
    xx, yy = grid_axis(S, num_steps, xsteps), grid_axis(S, num_steps, ysteps)
    return np.broadcast_to(xx[None, :], (S, S)), np.broadcast_to(yy[:, None], (S, S))


def optical_map64(S: int, k: float, dx: float, dy: float):
    """cv2.initUndistortRectifyMap with fx = fy = S, centre ((S - 1) / 2 seen from the output, S / 2 + shift in the source),
    distortion (k, k, 0, 0, 0)."""
    y, x = np.mgrid[0:S, 0:S].astype(np.float64)
    xh, yh = (x - (S - 1) / 2.0) / S, (y - (S - 1) / 2.0) / S
    r2 = xh * xh + yh * yh
    kr = 1.0 + k * r2 + k * r2 * r2
    return S * xh * kr + S / 2.0 + dx, S * yh * kr + S / 2.0 + dy


def quantise(u, v) -> np.ndarray:
    """Q5 fixed point, round half to even (cvRound; OpenCV INTER_BITS = 5): int64 [S, S, 2] = (x, y)."""
    return np.stack([np.rint(32.0 * u), np.rint(32.0 * v)], -1).astype(np.int64)


def identity_map(S: int) -> np.ndarray:
    y, x = np.mgrid[0:S, 0:S]
    return np.stack([32 * x, 32 * y], -1).astype(np.int64)


def remap(img: np.ndarray, mask: np.ndarray, q: np.ndarray):
    """uint8 [S, S, 3] + integer [S, S] through the Q5 map ``q`` [S, S, 2]: OpenCV's 8-bit INTER_LINEAR remap (BilinearTab_i
    without its common factor 32) with every tap reflected by reflect-101; mask nearest at the rounded quantised coordinate."""
    S = img.shape[0]
    q = q.astype(np.int64)
    qx, qy = q[..., 0], q[..., 1]
    ix, iy, fx, fy = qx >> 5, qy >> 5, (qx & 31)[..., None], (qy & 31)[..., None]
    x0, x1, y0, y1 = reflect_101(ix, S), reflect_101(ix + 1, S), reflect_101(iy, S), reflect_101(iy + 1, S)
    src = img.astype(np.int64)
    acc = (32 - fx) * (32 - fy) * src[y0, x0] + fx * (32 - fy) * src[y0, x1] + (32 - fx) * fy * src[y1, x0] + fx * fy * src[y1, x1]
    out = ((acc + 512) >> 10).astype(np.uint8)
    return out, mask[reflect_101((qy + 16) >> 5, S), reflect_101((qx + 16) >> 5, S)]
