"""CPU: the float64 restatement of the distillation loss (tests/distill_ref.py) against torch's own ``F.kl_div`` and the closed form
of its gradient; the ABI of libasis_distill.so (include/asis_distill.h: every declared symbol exported and bound, none of them in
libasis_hip.so) and the argument errors of ``asis_distill_loss`` that need no GPU; the module surface."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from adaptersis_amd import _lib, _lib_distill, ops
from adaptersis_amd.segloss.distill import DistillationLoss
from tests import distill_ref as R
from tests.bound_helpers import _gen


@pytest.mark.parametrize("temp", [1.0, 2.0, 4.0])
@pytest.mark.parametrize("C", [2, 3, 8])
@pytest.mark.parametrize("scale", [1.0, 30.0])
def test_restatement_is_kl_div_and_its_gradient_the_closed_form(temp, C, scale):
    g = _gen(C, int(temp), int(scale))
    B, h, w, H, W = 2, 5, 7, 13, 11
    z = torch.randn(B, h, w, C, generator=g, dtype=torch.float64) * scale
    t = torch.randn(B, 6, 4, C, generator=g, dtype=torch.float64) * scale
    loss, dz, dlow, p, q = R.distill_ref(z, [t], [False], (H, W), temp)
    N = B * H * W
    zr, tr = R._resized(z, (H, W)), R._resized(t, (H, W))
    want = temp * temp * F.kl_div(torch.log_softmax(zr / temp, 1), torch.softmax(tr / temp, 1), reduction="sum") / N
    assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want))
    closed = (temp / N) * (p - q).permute(0, 2, 3, 1)
    assert float((dz - closed).abs().max()) <= 1e-12 * float(closed.abs().max())
    assert float(loss) >= 0.0 and torch.isfinite(dz).all() and tuple(dlow.shape) == (B, h, w, C)


def test_restatement_mirrored_view_and_zero_at_the_teacher():
    g = _gen(5)
    z = torch.randn(2, 5, 7, 3, generator=g, dtype=torch.float64)
    v = torch.randn(2, 9, 3, 3, generator=g, dtype=torch.float64)
    a = R.distill_ref(z, [v], [False], (13, 11), 2.0)
    b = R.distill_ref(z, [v.flip(2).contiguous()], [True], (13, 11), 2.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    loss, dz, *_ = R.distill_ref(z, [z], [False], (13, 11), 2.0)
    assert abs(float(loss)) < 1e-15 and float(dz.abs().max()) < 1e-17


def test_side_library_abi():
    """include/asis_distill.h against libasis_distill.so and its binding, as tests/test_abi.py does for the main library, which
    holds none of these symbols (it is what the training step loads, and it is built from the sources it was built from)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "asis_distill.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(asis_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(_lib_distill.SIGNATURES) == ["asis_distill_loss", "asis_distill_nblk", "asis_distill_tile"]
    assert os.path.dirname(_lib_distill.LIB_PATH) == os.path.dirname(_lib.LIB_PATH)
    side, main = ctypes.CDLL(_lib_distill.LIB_PATH), ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(side, n) and not hasattr(main, n) and n not in _lib.SIGNATURES
    assert _lib_distill.lib() is _lib_distill.lib()


def test_nblk_and_tile_need_no_gpu():
    lib = _lib_distill.lib()
    tile = lib.asis_distill_tile()
    assert tile > 0 and tile % 64 == 0
    cap = lib.asis_distill_nblk((1 << 31) - 1)
    assert cap >= 256
    for N, want in ((1, 1), (tile - 1, 1), (tile, 1), (tile + 1, 2), (cap * tile, cap), (cap * tile + 1, cap)):
        assert lib.asis_distill_nblk(N) == want
        assert ops.distill_scratch_bytes(N) == 8 * want
    for N in (0, -5, 1 << 31, 1 << 40):
        assert lib.asis_distill_nblk(N) == -1 and b"2^31" in _lib.lib().asis_last_error()
        with pytest.raises(ValueError):
            ops.distill_scratch_bytes(N)


def test_argument_errors_before_any_launch():
    lib, last_error = _lib_distill.lib(), _lib.lib().asis_last_error
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)

    def call(logits=p, teachers="list", V=1, B=1, h=2, w=2, H=2, W=2, C=2, temp=1.0, partial=p, loss=p, dz=p, hs=2, ws=2, first=p):
        n = max(V, 1)
        ptrs = (ctypes.c_void_p * n)(*([first] + [p] * (n - 1)))
        th, tw, fl = (ctypes.c_int * n)(*[hs] * n), (ctypes.c_int * n)(*[ws] * n), (ctypes.c_int * n)(*[0] * n)
        return lib.asis_distill_loss(None, logits, B, h, w, ptrs if teachers == "list" else teachers, th, tw, fl, V, H, W, C, temp,
                                     1.0, 0, partial, loss, dz)

    for kw, word in ((dict(logits=None), b"null"), (dict(teachers=None), b"null"), (dict(partial=None), b"null"),
                     (dict(loss=None), b"null"), (dict(dz=None), b"null"), (dict(first=None), b"teachers[0]"),
                     (dict(V=0), b"V=0"), (dict(V=9), b"V=9"), (dict(C=0), b"C=0"), (dict(C=17), b"C=17"), (dict(B=0), b"non-positive"),
                     (dict(h=0), b"non-positive"), (dict(W=-3), b"non-positive"), (dict(hs=0), b"teacher map 0"),
                     (dict(temp=0.0), b"temperature"), (dict(temp=-1.0), b"temperature"), (dict(temp=float("nan")), b"temperature"),
                     (dict(B=1 << 11, H=1 << 10, W=1 << 10), b"2^31"), (dict(partial=p + 4), b"aligned")):
        assert call(**kw) == _lib.ASIS_EINVAL, kw
        assert word in last_error(), (kw, last_error())
    with pytest.raises(ValueError):
        _lib.check(call(C=17), "asis_distill_loss")


def test_op_and_module_have_no_cpu_fallback():
    z, t = torch.zeros(1, 2, 2, 3), torch.zeros(1, 2, 2, 3)
    with pytest.raises(_lib.AsisError):
        ops.distill_loss(z, t, (4, 4))
    with pytest.raises(_lib.AsisError):
        DistillationLoss(2.0)(z.permute(0, 3, 1, 2), t.permute(0, 3, 1, 2), (4, 4))
    m = DistillationLoss(4.0, [False, True])
    assert m.temperature == 4.0 and m.flips == [False, True] and DistillationLoss().temperature == 1.0
    with pytest.raises(ValueError):
        DistillationLoss(0.0)
    with pytest.raises(NotImplementedError):
        DistillationLoss()(torch.zeros(1, 3, 2, 4, 5), t)
