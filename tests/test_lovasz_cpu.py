"""CPU: the host side of the Lovasz-Softmax loss — ``lovasz_grad`` in closed form against the reference formula, the C-ABI
entries that need no GPU, the engine keys, the ``--loss`` flag of the three training scripts, and the input rule of the
golden fixture tests/golden/lovasz_ref.pt (made by tests/golden/make_lovasz_golden.py)."""
import ctypes
import importlib.util
import os

import pytest
import torch

from adaptersis_amd import _lib, ops
from adaptersis_amd import train as T
from adaptersis_amd import train_mla as TMLA
from adaptersis_amd import train_multi_class as TMC
from adaptersis_amd.backbones.engines import SegEngine
from adaptersis_amd.segloss.lovasz_loss import LovaszSoftmax, lovasz_grad
from tests import lovasz_ref as R
from tests.conftest import GOLDEN, load_golden


@pytest.mark.parametrize("n", [1, 2, 3, 65, 1000, 4097])
@pytest.mark.parametrize("share", [0.0, 0.02, 0.5, 1.0])
def test_lovasz_grad_closed_form_against_the_reference_formula(n, share):
    """float64 against float64: the limit is the cancellation of the difference form, ~ n 2^-52 <= 1e-12 here"""
    gen = torch.Generator().manual_seed(n * 7 + int(share * 100))
    flags = (torch.rand(n, generator=gen) < share).long() if 0.0 < share < 1.0 else torch.full((n,), int(share), dtype=torch.int64)
    g = lovasz_grad(flags)
    assert g.dtype == torch.float64 and g.shape == (n,)
    assert float((g - R.reference_g(flags)).abs().max()) <= 1e-12
    assert float((g - R.closed_g(flags)).abs().max()) <= 1e-15
    assert abs(float(g.sum()) - 1.0) <= 1e-12   # the differences telescope to the last Jaccard value, 1


def test_scratch_and_tile_need_no_gpu():
    lib = _lib.lib()
    tile = lib.asis_lovasz_tile()
    assert tile > 0 and tile % 64 == 0
    last = 0
    for N in (1, tile - 1, tile, tile + 1, 12 * 588 * 588):
        b = lib.asis_lovasz_scratch_bytes(N, 8)
        assert b > 0 and b >= last and b >= 20 * N * 8   # buffers are rounded up to 256 bytes: equal for neighbouring N
        last = b
    assert lib.asis_lovasz_scratch_bytes(1, 8) < lib.asis_lovasz_scratch_bytes(tile + 1, 8) < last
    last = 0
    for C in range(1, 17):
        b = ops.lovasz_scratch_bytes(4097, C)
        assert b > last
        last = b
    assert 0.6e9 < ops.lovasz_scratch_bytes(12 * 588 * 588, 8) < 0.75e9   # the figure of the docs
    for N, C in ((0, 2), (1 << 31, 2), (100, 0), (100, 17)):
        assert lib.asis_lovasz_scratch_bytes(N, C) == -1 and lib.asis_last_error()
        with pytest.raises(ValueError):
            ops.lovasz_scratch_bytes(N, C)


def test_argument_errors_before_any_launch():
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(logits=p, target=p, B=1, h=2, w=2, H=2, W=2, C=2, n_softmax=1, reduction=0, scratch=p, loss=p, per_class=p, dz=p):
        return lib.asis_lovasz_softmax(None, logits, target, B, h, w, H, W, C, n_softmax, reduction, 1.0, 0, scratch, loss,
                                       per_class, dz, None, None)

    for kw, word in ((dict(logits=None), b"null"), (dict(target=None), b"null"), (dict(scratch=None), b"null"),
                     (dict(loss=None), b"null"), (dict(per_class=None), b"null"), (dict(dz=None), b"null"),
                     (dict(C=17), b"C=17"), (dict(C=0), b"C=0"), (dict(n_softmax=2), b"n_softmax"),
                     (dict(reduction=3), b"reduction"), (dict(B=1 << 11, H=1 << 10, W=1 << 10), b"2^31")):
        assert call(**kw) == _lib.ASIS_EINVAL, kw
        assert word in lib.asis_last_error(), (kw, lib.asis_last_error())
    with pytest.raises(ValueError):
        _lib.check(call(C=17), "asis_lovasz_softmax")


def test_engine_keys_and_loss_flag():
    assert "lovasz" in SegEngine.LOSSES and "ce_lovasz" in SegEngine.LOSSES
    for mod, default in ((T, "dice"), (TMLA, "dice"), (TMC, "iou")):
        p = mod.get_args_parser()
        assert p.parse_args([]).loss == default
        assert p.parse_args(["--loss", "lovasz"]).loss == "lovasz"
        assert p.parse_args(["--loss", "ce_lovasz"]).loss == "ce_lovasz"
        for key in SegEngine.LOSSES:
            assert p.parse_args(["--loss", key]).loss == key
        with pytest.raises(SystemExit):
            p.parse_args(["--loss", "hinge"])


def test_module_surface():
    assert LovaszSoftmax().reduction == "mean" and LovaszSoftmax(reduction="sum").reduction == "sum"
    with pytest.raises(NotImplementedError):
        LovaszSoftmax()(torch.zeros(1, 2, 3, 4, 5), torch.zeros(1, 3, 4, 5, dtype=torch.int64))
    with pytest.raises(_lib.AsisError):   # no CPU fallback
        LovaszSoftmax()(torch.full((1, 2, 3, 4), 0.5), torch.zeros(1, 3, 4, dtype=torch.int64))


def test_golden_input_rule():
    """the minimal gap between sorted keys is >= 1e-5 per class, in float64 and in float32: the order of the fixture's keys
    is the same in every precision"""
    spec = importlib.util.spec_from_file_location("make_lovasz_golden", os.path.join(GOLDEN, "make_lovasz_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    cases = load_golden("lovasz_ref")["cases"]
    assert [tuple(c["shape"]) for c in cases] == gen.SHAPES
    for c in cases:
        B, h, w, C = c["shape"]
        assert c["logits"].shape == (B, h, w, C) and c["target"].shape == (B, h, w) and c["probs"].shape == (B, C, h, w)
        z = c["logits"].permute(0, 3, 1, 2)
        assert float((torch.softmax(z.double(), 1) - c["probs"]).abs().max()) < 1e-6
        for q in (torch.softmax(z.double(), 1), c["probs"]):
            keys = R.keys_of(q.permute(0, 2, 3, 1), c["target"])
            s = torch.sort(keys, dim=1).values
            gaps = (s[:, 1:] - s[:, :-1]).min(1).values
            assert float(gaps.min()) >= 1e-5, (c["shape"], q.dtype, gaps)
