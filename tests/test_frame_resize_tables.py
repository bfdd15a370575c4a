"""CPU: the host tables of the on-device frame resize (tools/frame_resize.py) restate PIL's BILINEAR / NEAREST resize bit for bit,
through the same integer passes the kernel (csrc/frame_resize.hip) runs; the label tables of the datasets."""
import numpy as np
import pytest
from PIL import Image

from adaptersis_amd.tools import frame_resize as F

# (height, width) -> square size: EndoVis 1280x1024, 16:9 960x540, odd sizes, an upscale, one unchanged axis, 1080p, 518
PAIRS = [((1024, 1280), 588), ((1024, 1280), 224), ((540, 960), 588), ((540, 960), 224), ((257, 333), 588), ((257, 333), 224),
         ((150, 200), 224), ((700, 588), 588), ((1080, 1920), 588), ((1024, 1280), 518)]


@pytest.mark.parametrize("hw,S", PAIRS)
def test_bilinear_passes_equal_pil(hw, S):
    rng = np.random.default_rng(hash((hw, S)) % (1 << 32))
    img = rng.integers(0, 256, hw + (3,), dtype=np.uint8)
    want = np.asarray(Image.fromarray(img).resize((S, S), resample=Image.BILINEAR))
    got = F.resize_frame_host(img, S, S)
    assert got.shape == want.shape
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"


@pytest.mark.parametrize("hw,S", PAIRS)
def test_nearest_tables_equal_pil(hw, S):
    rng = np.random.default_rng(7)
    m = rng.integers(0, 256, hw, dtype=np.uint8)
    want = np.asarray(Image.fromarray(m).resize((S, S), resample=Image.NEAREST))
    assert np.array_equal(F.resize_mask_host(m, S, S), want)
    assert F.nearest_table(hw[1], S).dtype == np.int32 and F.nearest_table(hw[1], S).shape == (S,)


def test_table_shapes_and_ranges():
    span, k = F.bilinear_tables(1280, 588)
    assert span.shape == (588, 2) and k.shape == (588, 2 * 3 + 1)
    assert (span[:, 0] >= 0).all() and (span.sum(1) <= 1280).all() and (span[:, 1] >= 1).all()
    assert (k[np.arange(k.shape[1])[None, :] >= span[:, 1:2]] == 0).all()
    assert (np.abs(k.sum(1) - (1 << 22)) <= k.shape[1]).all()
    span, k = F.bilinear_tables(200, 224)             # upscale: fs = 1, support 1, ksize 3
    assert k.shape == (224, 3)


def test_label_tables():
    x = np.arange(256)
    assert np.array_equal(F.LUT_BINARY, (x > 0).astype(np.uint8))
    assert np.array_equal(F.LUT_MULTI, np.floor(x / 32.0).astype(np.uint8))
    assert list(F.LUT_MULTI[[0, 32, 64, 96, 128, 160, 192, 224]]) == list(range(8))
    assert F.LUT_BINARY.dtype == F.LUT_MULTI.dtype == np.uint8 and F.LUT_MULTI.shape == (256,)


def test_mask_resize_commutes_with_the_label_table():
    rng = np.random.default_rng(3)
    m = (rng.integers(0, 8, (257, 333)) * 32).astype(np.uint8)
    a = F.resize_mask_host(m, 224, 224, F.LUT_MULTI)
    b = np.asarray(Image.fromarray(F.LUT_MULTI[m]).resize((224, 224), resample=Image.NEAREST))
    assert np.array_equal(a, b)
