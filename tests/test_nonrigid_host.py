"""CPU: the host side of the non-rigid augmentation block (adaptersis_amd/tools/augment.py) and the numpy restatement the GPU
tests compare against (tests/nonrigid_ref.py): Philox known answers, Gauss and grid tables, the draws, the integer remap,
argument errors of the two ABI entries.

Five of these validate the restatement itself, not product code (they need only tests/nonrigid_ref.py): the Philox known
answers, the noise's exactness in fp32, the periodic reflection against scipy, the integer shift and the half-pixel average.
The GPU tests are only as good as that reference, so it is pinned here; the other tests call ``tools.augment`` or the library."""
import ctypes

import numpy as np
import pytest

from adaptersis_amd import _lib
from adaptersis_amd.tools import augment as A
from tests import nonrigid_ref as R


def _hex(words):
    return " ".join(f"{int(w[0]):08x}" for w in words)


def test_philox_known_answers():
    """The vectors published with Random123 (kat_vectors, philox4x32-10)."""
    z, o = np.zeros(1, np.uint64), np.full(1, 0xFFFFFFFF, np.uint64)
    assert _hex(R.philox4x32_10(z, z, z, z, 0, 0)) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(R.philox4x32_10(o, o, o, o, 0xFFFFFFFF, 0xFFFFFFFF)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"


def test_noise_is_exact_in_fp32_and_uses_all_four_words():
    n = R.noise(0x0123456789ABCDEF, 7)
    assert n.shape == (2, 7, 7) and np.all(n >= -1.0) and np.all(n < 1.0)
    assert np.array_equal(n.astype(np.float32).astype(np.float64), n)
    # element e = 5 is word 1 of block 1, field 1: spelled out once
    w = R.philox4x32_10(np.array([1], np.uint64), np.array([0], np.uint64), np.array([1], np.uint64), np.array([0], np.uint64),
                        0x89ABCDEF, 0x01234567)[1][0]
    assert n[1, 0, 5] == 2.0 * (float(int(w) >> 8) * 2.0 ** -24) - 1.0


@pytest.mark.parametrize("sigma", [6.0, 1.0, 0.1, 16.0])
def test_gauss_table_vs_scipy_impulse(sigma):
    from scipy.ndimage import gaussian_filter1d
    w = A.gauss_table(sigma)
    r = int(4 * sigma + 0.5)
    assert w.dtype == np.float32 and w.shape == (2 * r + 1,)
    imp = np.zeros(4 * r + 1)
    imp[2 * r] = 1.0
    want = gaussian_filter1d(imp, sigma, mode="constant")[r:3 * r + 1]
    assert np.abs(w.astype(np.float64) - want).max() <= 2.0 ** -24            # one fp32 rounding of weights <= 1
    assert np.abs(R.gauss_kernel(sigma) - want).max() <= 1e-15
    with pytest.raises(ValueError):
        A.gauss_table(17.0)                                                   # r = 68 > 64


def test_periodic_reflection_equals_scipy_reflect_beyond_the_plane():
    """S = 20 < r = 24: the window reflects more than once."""
    from scipy.ndimage import gaussian_filter
    n = R.noise(5, 20)[0]
    assert np.abs(R.blur_reflect(n, R.gauss_kernel(6.0)) - gaussian_filter(n, 6.0, mode="reflect")).max() < 1e-15


@pytest.mark.parametrize("S", [20, 64, 100, 588])
def test_grid_tables_vs_the_loop(S):
    """Non-decreasing wherever the published loop is: over the five drawn segments always (steps > 0), and over the pinned
    sixth segment too unless the drawn segments already passed S — then the loop walks back down to S (S = 64, steps 1.3:
    78 -> 64), which is kept like its other quirks."""
    r = np.random.RandomState(S)
    step = S // 5
    for steps in (1.0 + r.uniform(-0.3, 0.3, 6), np.full(6, 1.3), np.full(6, 0.7)):
        got, want = A.grid_table(S, 5, steps), R.grid_axis(S, 5, steps)
        assert got.shape == (S,) and np.abs(got - want).max() <= 1e-9
        assert got[0] == 0.0 and np.all(np.diff(got[:5 * step]) >= 0)
        assert np.all(np.diff(got) >= 0) == bool(S % 5 == 0 or got[5 * step - 1] <= S)
    up, down = A.grid_table(S, 5, np.full(6, 1.3)), A.grid_table(S, 5, np.full(6, 0.7))
    if S % 5 == 0:            # the 6th segment is empty: nothing pins the end, the table ends where the steps add up to
        assert abs(up[-1] - 5 * step * 1.3) < 1e-9 and abs(down[-1] - 5 * step * 0.7) < 1e-9
        assert (up[-1] > S) and (down[-1] < S)           # S = 100 ends above 100, S = 20 below 20
    else:                     # the 6th segment overruns and is pinned to S
        assert up[-1] == S and down[-1] == S
    assert up[step - 1] == up[step]                      # a join repeats a value (linspace includes both ends)


def test_elastic_affine_is_the_inverse_of_the_three_point_map():
    S = 64
    pts = np.random.RandomState(0).uniform(-3.6, 3.6, (3, 2))
    Ainv = A.elastic_affine(S, pts)
    c, s = S // 2, S // 3
    pts1 = np.array([[c + s, c + s], [c + s, c - s], [c - s, c - s]], np.float64)
    back = (Ainv[:, :2] @ (pts1 + pts).T).T + Ainv[:, 2]
    assert np.abs(back - pts1).max() < 1e-10
    assert np.abs(Ainv - R.elastic_affine(S, pts)).max() < 1e-10
    assert np.abs(A.elastic_affine(S, np.zeros((3, 2))) - np.eye(3)[:2]).max() < 1e-14


def test_draw_shares():
    """OneOf: P overall, members by their normalised p = 1/4, 1/4, 1/2 (allowance of test_draw_distributions_and_luts)."""
    aug = A.TrainAugment(size=64, seed=11, non_rigid_p=0.8)
    ps = aug.draw(4000)
    nr = [p["nonrigid"] for p in ps if p["nonrigid"] is not None]
    assert abs(len(nr) / 4000 - 0.8) < 0.03
    share = {k: sum(d["kind"] == k for d in nr) / len(nr) for k in ("elastic", "grid", "optical")}
    assert abs(share["elastic"] - 0.25) < 0.03 and abs(share["grid"] - 0.25) < 0.03 and abs(share["optical"] - 0.5) < 0.03
    for d in nr:
        if d["kind"] == "elastic":
            assert 0 <= d["seed"] < 1 << 64 and d["pts"].shape == (3, 2) and np.abs(d["pts"]).max() <= 3.6
        elif d["kind"] == "grid":
            assert d["xsteps"].shape == (6,) and d["ysteps"].shape == (6,)
            assert np.all(np.abs(np.concatenate([d["xsteps"], d["ysteps"]]) - 1.0) <= 0.3)
        else:
            assert abs(d["k"]) <= 2.0 and d["dx"] == 0 and d["dy"] == 0      # round(U(-0.5, 0.5)) is always 0
    assert any(d["seed"] >> 32 for d in nr if d["kind"] == "elastic")        # the seed uses its upper half


def test_p0_consumes_the_stream_of_today():
    a, b = A.TrainAugment(size=64, seed=3), A.TrainAugment(size=64, seed=3, non_rigid_p=0.0)
    pa, pb = a.draw(50), b.draw(50)
    assert all(p["nonrigid"] is None for p in pb)
    strip = lambda ps: [{k: v for k, v in p.items() if k != "nonrigid"} for p in ps]
    assert strip(pa) == strip(pb)
    sa, sb = a.rng.get_state(), b.rng.get_state()
    assert sa[0] == sb[0] and np.array_equal(sa[1], sb[1]) and sa[2:] == sb[2:]
    # and the stream is the one of the constructor without the argument: first draws of seed 3, spelled out
    r = np.random.RandomState(3)
    first_crop = r.random_sample() < 0.5 / 1.5
    assert (pa[0]["crop"] is not None) == first_crop
    c = A.TrainAugment(size=64, seed=3, non_rigid_p=0.5)
    c.draw(50)
    assert not np.array_equal(c.rng.get_state()[1], sa[1])


def test_integer_shift_map_shifts_with_reflect_101():
    S = 9
    r = np.random.RandomState(1)
    img = r.randint(0, 256, (S, S, 3)).astype(np.uint8)
    msk = r.randint(0, 5, (S, S)).astype(np.int64)
    out, mo = R.remap(img, msk, R.identity_map(S))
    assert np.array_equal(out, img) and np.array_equal(mo, msk)
    for sx, sy in ((3, 0), (-2, 4), (11, -13), (-40, 37)):
        q = R.identity_map(S) + 32 * np.array([sx, sy])
        out, mo = R.remap(img, msk, q)
        pad = np.pad(np.arange(S), 48, mode="reflect")          # numpy's 'reflect' is reflect-101, as deep as asked
        ix, iy = pad[48 + sx:48 + sx + S], pad[48 + sy:48 + sy + S]
        assert np.array_equal(out, img[iy][:, ix]) and np.array_equal(mo, msk[iy][:, ix])


def test_half_pixel_map_averages_and_rounds():
    img = np.zeros((2, 2, 3), np.uint8)
    img[0, 1], img[1, 0], img[1, 1] = 10, 21, 255
    q = np.zeros((2, 2, 2), np.int64)
    q[0, 0] = (16, 16)                                  # centre of the four pixels
    out, _ = R.remap(img, np.zeros((2, 2), np.int64), q)
    assert out[0, 0, 0] == (256 * (0 + 10 + 21 + 255) + 512) >> 10


def test_argument_errors_are_reported_without_a_gpu():
    lib = _lib.lib()
    buf = (ctypes.c_char * 256)()
    p = ctypes.addressof(buf)
    p += (-p) % 16
    ok_map = dict(kind=p, params=p, seed=p, gx=p, gy=p, gauss=p, r=24, tmp=p, map=p, field=None, B=1, S=20)

    def call_map(**kw):
        a = dict(ok_map, **kw)
        return lib.asis_nonrigid_map(None, a["kind"], a["params"], a["seed"], a["gx"], a["gy"], a["gauss"], a["r"], a["tmp"], a["map"],
                                     a["field"], a["B"], a["S"])
    for kw, msg in ((dict(kind=None), b"null pointer"), (dict(tmp=None), b"null pointer"), (dict(map=None), b"null pointer"),
                    (dict(S=1), b"bad batch / size"), (dict(S=8193), b"bad batch / size"), (dict(B=0), b"bad batch / size"),
                    (dict(r=65), b"Gauss radius"), (dict(r=-1), b"Gauss radius"), (dict(params=p + 4), b"alignment"),
                    (dict(map=p + 4), b"alignment")):
        assert call_map(**kw) == -1 and msg in lib.asis_last_error(), kw
    ok_re = dict(img=p, mask=p + 64, map=p + 128, out=p + 32, mask_out=p + 192, B=1, S=2)

    def call_re(**kw):
        a = dict(ok_re, **kw)
        return lib.asis_nonrigid_remap(None, a["img"], a["mask"], a["map"], a["out"], a["mask_out"], a["B"], a["S"])
    for kw, msg in ((dict(img=None), b"null pointer"), (dict(mask_out=None), b"null pointer"), (dict(S=1), b"bad batch / size"),
                    (dict(B=0), b"bad batch / size"), (dict(out=p), b"alias"), (dict(mask_out=p + 64), b"alias"),
                    (dict(map=p + 132), b"alignment"), (dict(mask=p + 68), b"alignment")):
        assert call_re(**kw) == -1 and msg in lib.asis_last_error(), kw
    with pytest.raises(ValueError):
        _lib.check(-1, "asis_nonrigid_remap")
