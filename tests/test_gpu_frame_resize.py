"""GPU: ops.frame_resize (csrc/frame_resize.hip) is byte-identical to PIL's BILINEAR (frames) and NEAREST + label table
(masks) for every size pair, at B = 1 and B = 12; a mixed-size collate_frames batch gives the all-host route's bytes; runs
repeat exactly."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from adaptersis_amd import ops
from adaptersis_amd import train as T
from adaptersis_amd.tools import dataset as D
from adaptersis_amd.tools import frame_resize as F

pytestmark = pytest.mark.gpu

PAIRS = [((1024, 1280), 588), ((1024, 1280), 224), ((540, 960), 588), ((540, 960), 224), ((257, 333), 588), ((257, 333), 224),
         ((150, 200), 224), ((700, 588), 588), ((1080, 1920), 588), ((1024, 1280), 518)]


def _pil(img, mask, S, lut):
    return (np.asarray(Image.fromarray(img).resize((S, S), resample=Image.BILINEAR)),
            lut[np.asarray(Image.fromarray(mask).resize((S, S), resample=Image.NEAREST))])


@pytest.mark.parametrize("B", [1, 12])
@pytest.mark.parametrize("hw,S", PAIRS)
def test_kernel_equals_pil(dev, hw, S, B):
    rng = np.random.default_rng(S * 7 + hw[0] + B)
    imgs = rng.integers(0, 256, (B,) + hw + (3,), dtype=np.uint8)
    masks = rng.integers(0, 256, (B,) + hw, dtype=np.uint8)
    lut = rng.permutation(256).astype(np.uint8)
    oi, om = ops.frame_resize(torch.from_numpy(imgs).to(dev), torch.from_numpy(masks).to(dev), S, lut)
    oi, om = oi.cpu().numpy(), om.cpu().numpy()
    assert oi.shape == (B, S, S, 3) and om.shape == (B, S, S)
    for b in range(B):
        wi, wm = _pil(imgs[b], masks[b], S, lut)
        assert np.array_equal(oi[b], wi), f"frame {b}: {int((oi[b] != wi).sum())} bytes differ"
        assert np.array_equal(om[b], wm), f"mask {b}: {int((om[b] != wm).sum())} bytes differ"


def test_unaligned_views_and_single_inputs(dev):
    """Views at odd byte offsets take the byte paths; frames-only and masks-only calls."""
    rng = np.random.default_rng(5)
    imgs = torch.from_numpy(rng.integers(0, 256, (4, 257, 333, 3), dtype=np.uint8)).to(dev)
    masks = torch.from_numpy(rng.integers(0, 256, (4, 257, 333), dtype=np.uint8)).to(dev)
    for S in (224, 518):
        oi, om = ops.frame_resize(imgs[1:], masks[1:], S, F.LUT_MULTI)
        fi, none_m = ops.frame_resize(imgs[1:], None, S)
        none_i, fm = ops.frame_resize(None, masks[1:], S, F.LUT_MULTI)
        assert none_m is None and none_i is None
        assert torch.equal(oi, fi) and torch.equal(om, fm)
        for b in range(3):
            wi, wm = _pil(imgs[b + 1].cpu().numpy(), masks[b + 1].cpu().numpy(), S, F.LUT_MULTI)
            assert np.array_equal(oi[b].cpu().numpy(), wi) and np.array_equal(om[b].cpu().numpy(), wm)


def test_repeat_runs_identical(dev):
    rng = np.random.default_rng(9)
    imgs = torch.from_numpy(rng.integers(0, 256, (12, 1024, 1280, 3), dtype=np.uint8)).to(dev)
    masks = torch.from_numpy(rng.integers(0, 256, (12, 1024, 1280), dtype=np.uint8)).to(dev)
    a = ops.frame_resize(imgs, masks, 588, F.LUT_BINARY)
    b = ops.frame_resize(imgs, masks, 588, F.LUT_BINARY)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_mixed_size_batch_equals_host_route(dev, tmp_path):
    rng = np.random.default_rng(11)
    for d, hw, n in (("instrument_dataset_1", (256, 320), 3), ("instrument_dataset_2", (150, 200), 2)):
        for k in range(n):
            for sub, arr in (("images", rng.integers(0, 256, hw + (3,), dtype=np.uint8)),
                             ("instruments_masks", (rng.integers(0, 8, hw) * 32).astype(np.uint8))):
                os.makedirs(tmp_path / "Train" / d / sub, exist_ok=True)
                Image.fromarray(arr).save(tmp_path / "Train" / d / sub / f"f{k}.png")
    gpu = D.EndoVis2017(str(tmp_path), "Train", imsize=224, task="multi")
    host = D.EndoVis2017(str(tmp_path), "Train", imsize=224, task="multi", resize_on_gpu=False)
    order = [3, 0, 4, 1, 2]                                  # batch size = 150x200 (first item); three frames take the host route
    fb, _, _ = gpu.collate_fn([gpu[i] for i in order])
    assert fb.pos.tolist() == [0, 2] and fb.host_pos.tolist() == [1, 3, 4]
    img, msk = T._resize_frames(fb)
    hi, hm, _ = D.collate_u8([host[i] for i in order])
    assert torch.equal(img.cpu(), hi) and torch.equal(msk.cpu(), hm)
    fb, _, _ = gpu.collate_fn([gpu[i] for i in range(3)])    # one size: all on the device
    img, msk = T._resize_frames(fb)
    hi, hm, _ = D.collate_u8([host[i] for i in range(3)])
    assert fb.host_pos.numel() == 0 and torch.equal(img.cpu(), hi) and torch.equal(msk.cpu(), hm)
