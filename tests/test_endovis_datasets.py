"""CPU: EndoVis2017 / EndoVis2018 / Autolapro (tools/dataset.py) on small PNG trees — folder layouts, sorted and checked pairing,
host-route items equal to the PIL expressions of the reference's datasets, both EndoVis2017 tasks, and collate_frames."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from adaptersis_amd.tools import dataset as D
from adaptersis_amd.tools import frame_resize as F

S = 24


def _png(path, arr, mode=None):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    im = Image.fromarray(arr)
    if mode == "P":
        im = Image.fromarray(arr, "P")
        im.putpalette([(255 - i) % 256 for i in range(768)])   # palette differs from the indices
    im.save(path)


def _tree(root, split, folders, masks_dir, n=3, hw=(30, 40), mask_mode="L", multi=False, seed=0):
    rng = np.random.default_rng(seed)
    for f in folders:
        for k in reversed(range(n)):          # written out of order: pairing must not rely on creation order
            name = f"frame{k:03d}.png"
            _png(os.path.join(root, split, f, "images", name), rng.integers(0, 256, hw + (3,), dtype=np.uint8))
            if multi:
                m = (rng.integers(0, 8, hw) * 32).astype(np.uint8)
            else:
                m = (rng.random(hw) > 0.6).astype(np.uint8) * rng.integers(1, 256, hw).astype(np.uint8)
            _png(os.path.join(root, split, f, masks_dir, name), m, mask_mode)


def _ref_item(img_path, mask_path, imsize, kind):
    """The reference's __getitem__ (`tools/dataset.py:37-59,100-112`) up to np.array."""
    img = Image.open(img_path).convert("RGB")
    mask = Image.open(mask_path)
    if kind == "binary2017":
        mask = mask.convert("L").point(lambda x: 1 if x > 0 else 0)
    elif kind == "multi":
        mask = Image.fromarray((np.array(mask) / 32.).astype(np.uint8)).convert("L")
    else:
        mask = mask.point(lambda x: 1 if x > 0 else 0)
    img = img.resize((imsize, imsize), resample=Image.BILINEAR)
    mask = mask.resize((imsize, imsize), resample=Image.NEAREST)
    return np.array(img).astype(np.uint8), np.array(mask).astype(np.uint8)


@pytest.mark.parametrize("mask_mode", ["L", "P"])
@pytest.mark.parametrize("task", ["binary", "multi"])
def test_endovis2017_host_route_equals_reference(tmp_path, task, mask_mode):
    sub = "binary_masks" if task == "binary" else "instruments_masks"
    _tree(str(tmp_path), "Train", ["instrument_dataset_1", "instrument_dataset_3"], sub, mask_mode=mask_mode, multi=task == "multi")
    ds = D.EndoVis2017(str(tmp_path), "Train", imsize=S, task=task, resize_on_gpu=False)
    assert len(ds) == 6
    assert [os.path.basename(p) for p in ds.img_files[:3]] == ["frame000.png", "frame001.png", "frame002.png"]
    assert "instrument_dataset_1" in ds.img_files[0] and "instrument_dataset_3" in ds.img_files[-1]
    for i in range(len(ds)):
        img, mask, idx = ds[i]
        wi, wm = _ref_item(ds.img_files[i], ds.mask_files[i], S, "binary2017" if task == "binary" else "multi")
        assert idx == i and img.dtype == torch.uint8 and mask.dtype == torch.uint8
        assert np.array_equal(img.numpy(), wi) and np.array_equal(mask.numpy(), wm)
    if task == "multi":
        assert int(max(ds[i][1].max() for i in range(len(ds)))) <= 7


@pytest.mark.parametrize("mask_mode", ["L", "P"])
@pytest.mark.parametrize("cls,split,folder", [(D.EndoVis2018, "Train", "seq_2"), (D.EndoVis2018, "Test", "seq_4"),
                                              (D.Autolapro, "Train", "seq_0"), (D.Autolapro, "Validation", "seq_226"),
                                              (D.Autolapro, "Test", "seq_227")])
def test_binary_datasets_host_route_equals_reference(tmp_path, cls, split, folder, mask_mode):
    _tree(str(tmp_path), split, [folder], "binary_masks", mask_mode=mask_mode)
    ds = cls(str(tmp_path), split, imsize=S, resize_on_gpu=False)
    assert len(ds) == 3
    for i in range(len(ds)):
        img, mask, _ = ds[i]
        wi, wm = _ref_item(ds.img_files[i], ds.mask_files[i], S, "binary")
        assert np.array_equal(img.numpy(), wi) and np.array_equal(mask.numpy(), wm)


def test_autolapro_ranges(tmp_path):
    _tree(str(tmp_path), "Train", ["seq_169", "seq_170"], "binary_masks", n=1)     # seq_170 belongs to Validation
    assert len(D.Autolapro(str(tmp_path), "Train", imsize=S)) == 1


def test_pairing_errors(tmp_path):
    root = str(tmp_path)
    _tree(root, "Train", ["seq_1"], "binary_masks")
    os.remove(os.path.join(root, "Train", "seq_1", "binary_masks", "frame001.png"))
    with pytest.raises(ValueError, match="seq_1"):
        D.EndoVis2018(root, "Train", imsize=S)
    Image.fromarray(np.zeros((30, 40), np.uint8)).save(os.path.join(root, "Train", "seq_1", "binary_masks", "other.png"))
    with pytest.raises(ValueError, match="paired"):
        D.EndoVis2018(root, "Train", imsize=S)
    with pytest.raises(ValueError, match="no images"):
        D.EndoVis2018(root, "Test", imsize=S)
    with pytest.raises(ValueError, match="no images"):
        D.EndoVis2017(root, "Train", imsize=S, task="multi")
    with pytest.raises(ValueError):
        D.EndoVis2017(root, "Validation", imsize=S)


def test_device_route_items_and_collate(tmp_path):
    root = str(tmp_path)
    _tree(root, "Train", ["instrument_dataset_2"], "instruments_masks", n=2, multi=True)
    _tree(root, "Train", ["instrument_dataset_5"], "instruments_masks", n=1, hw=(20, 26), multi=True, seed=1)
    ds = D.EndoVis2017(root, "Train", imsize=S, task="multi")
    host = D.EndoVis2017(root, "Train", imsize=S, task="multi", resize_on_gpu=False)
    img, mask, idx = ds[0]
    assert tuple(img.shape) == (30, 40, 3) and tuple(mask.shape) == (30, 40)
    raw = np.array(Image.open(ds.mask_files[0]))
    assert np.array_equal(mask.numpy(), raw)                       # raw mask: the table is applied with the resize
    fb, masks, idx = ds.collate_fn([ds[0], ds[2], ds[1]])          # item 2 is 20x26: host route
    assert fb.shape[0] == 3 and fb.size == S and list(idx) == [0, 2, 1]
    assert list(fb.pos) == [0, 2] and list(fb.host_pos) == [1]
    assert np.array_equal(fb.lut.numpy(), F.LUT_MULTI)
    assert np.array_equal(fb.host_frames[0].numpy(), host[2][0].numpy())
    assert np.array_equal(fb.host_masks[0].numpy(), host[2][1].numpy())
    # what the device computes for the native group, restated on the host, equals the host route
    for j, i in enumerate((0, 1)):                                 # batch places 0, 2 hold dataset items 0, 1
        assert np.array_equal(F.resize_frame_host(fb.frames[j].numpy(), S, S), host[i][0].numpy())
        assert np.array_equal(F.resize_mask_host(fb.masks[j].numpy(), S, S, F.LUT_MULTI), host[i][1].numpy())
    assert D.EndoVis2017(root, "Train", imsize=S, task="multi", resize_on_gpu=False).collate_fn is D.collate_u8


def test_callable_transform(tmp_path):
    _tree(str(tmp_path), "Test", ["seq_1"], "binary_masks", n=1)
    ds = D.EndoVis2018(str(tmp_path), "Test", imsize=S, transform=lambda image, mask: {"image": image[:, ::-1], "mask": mask[:, ::-1]})
    img, mask, idx = ds[0]
    wi, wm = _ref_item(ds.img_files[0], ds.mask_files[0], S, "binary")
    assert img.dtype == torch.float32 and tuple(img.shape) == (3, S, S) and mask.dtype == torch.int64
    assert torch.equal(img, torch.from_numpy(wi[:, ::-1].transpose(2, 0, 1).copy()) / 255.0)
    assert np.array_equal(mask.numpy(), wm[:, ::-1])
