"""GPU: knowledge distillation — ``ops.distill_loss`` (csrc/distill.hip) against the float64 restatement of tests/distill_ref.py,
and ``DistillationLoss``.

Bounds (tests/bound_helpers.py as it stands): for the loss and for dz, |device - float64| <= max(4 Y, U ulp32 max|ref|) with Y the
error of torch's own float32 evaluation of the restatement on the CPU, U = U_SUM for the loss and U_ELEM for dz.  Everything else
is an equality of bits: a mirrored view against the un-mirrored map, accumulation against torch's fp32 add, repeated calls, a
power-of-two ``grad_scale``, a student that is its own teacher (dz exactly 0).  Every case prints its figures before it asserts
(one MI355X, 2026-10-20: the largest error over all cases is 0.25 of its bound for the loss and 0.37 for dz)."""
import math

import pytest
import torch

from adaptersis_amd import _lib, _lib_distill, ops
from adaptersis_amd.segloss.distill import DistillationLoss
from tests import distill_ref as R
from tests.bound_helpers import U_ELEM, U_SUM, _bound, _err, _gen
from tests.soft_target_helpers import STUDENT, TEACHER_SETS, _factor, _maps, _tile_sizes

pytestmark = pytest.mark.gpu

TEMPS = [1.0, 2.0, 4.0]


def _against_float64(dev, tag, z, ts, flips, size, temp, **kw):
    """one call of the op against the restatement in float64, bounded by its float32 evaluation -> (loss, dz) on the device"""
    loss, dz = ops.distill_loss(z.to(dev), [t.to(dev) for t in ts], size, flips=flips, temperature=temp, **kw)
    ref = R.distill_ref(z, ts, flips, size, temp)
    f32 = R.distill_ref(z, ts, flips, size, temp, torch.float32)
    bl, yl = _bound(f32[0], ref[0], U_SUM)
    bd, yd = _bound(f32[1], ref[1], U_ELEM)
    el, ed = _err(loss.view(()), ref[0]), _err(dz, ref[1])
    print(f"MEASURE distill {tag}: loss {float(loss):.6e} ref {float(ref[0]):.6e} err {el:.3e} bound {bl:.3e} (yard {yl:.2e}); "
          f"dz err {ed:.3e} bound {bd:.3e} (yard {yd:.2e}, max|ref| {float(ref[1].abs().max()):.3e})")
    assert math.isfinite(float(loss)) and bool(torch.isfinite(dz).all())
    assert el <= bl and ed <= bd
    return loss, dz


# ---- 1. against float64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("C", [2, 3, 8, 16])
@pytest.mark.parametrize("views", sorted(TEACHER_SETS))
@pytest.mark.parametrize("size", [(13, 11), (5, 7)])
def test_against_float64(dev, size, views, C, temp, scale):
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS[views], scale, 1, size[0], len(views), C, int(temp), int(scale))
    _against_float64(dev, f"size={size} views={views} C={C} T={temp} x{scale}", z, ts, flips, size, temp)


@pytest.mark.parametrize("views", ["other", "three"])
@pytest.mark.parametrize("C", [3, 8])
def test_zero_log_zero_and_saturated_student(dev, C, views):
    """whether a random q_c underflows at x30 depends on the draw; here one teacher class is at -1e4 in every map (q_c = 0 in
    float32 and in float64: the term is 0), and the student is at -300 in a class the teacher holds likely (p_c = 0 in float32,
    log p_c finite)"""
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS[views], 1.0, 11, C, len(views))
    for t in ts:
        t[..., 0] = -1e4
    z[..., 1] = -300.0
    assert bool((R.soft_targets(ts, flips, (13, 11), 1.0)[:, 0] == 0).all())
    assert bool((torch.softmax(R._resized(z, (13, 11)), 1)[:, 1] == 0).all())
    loss, _ = _against_float64(dev, f"0log0 views={views} C={C}", z, ts, flips, (13, 11), 1.0)
    assert float(loss) > 10.0


# ---- 2. sizes around the tile, more workgroups than one sweep of the finalize kernel, more tiles than workgroups ------------------
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1", "257 tiles + 1"])
def test_sizes_around_the_tile(dev, which, C):
    tile, _ = _tile_sizes(_lib_distill.lib(), "distill")
    N = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "257 tiles + 1": 257 * tile + 1}[which]
    assert _lib_distill.lib().asis_distill_nblk(N) == -(-N // tile)
    H, Wd = _factor(N)
    z, ts, flips = _maps(1, C, STUDENT, TEACHER_SETS["three"], 1.0, 2, N % 1000, C)
    _against_float64(dev, f"N={N}={H}x{Wd} C={C}", z, ts, flips, (H, Wd), 2.0)


def test_more_tiles_than_workgroups(dev):
    """a workgroup walks several tiles (the grid is capped); C = 3 only: the walk does not depend on the store path, and the
    float64 restatement of 2 M pixels x 8 classes would take the seconds a test has"""
    tile, cap = _tile_sizes(_lib_distill.lib(), "distill")
    N = cap * tile + 1
    assert _lib_distill.lib().asis_distill_nblk(N) == cap
    H, Wd = _factor(N)
    z, ts, flips = _maps(1, 3, STUDENT, TEACHER_SETS["other"], 1.0, 3)
    _against_float64(dev, f"N={N}={H}x{Wd} C=3", z, ts, flips, (H, Wd), 2.0)


# ---- 3. the student is the teacher -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 8, 16])
@pytest.mark.parametrize("size", [(13, 11), (5, 7)])
def test_student_is_the_teacher(dev, size, C):
    for scale in (1.0, 30.0):
        z, _, _ = _maps(2, C, STUDENT, [], scale, 4, C, int(scale))
        for temp in TEMPS:
            _, dz = _against_float64(dev, f"self size={size} C={C} T={temp} x{scale}", z, [z], [False], size, temp)
            assert int(torch.count_nonzero(dz)) == 0


# ---- 4. mirrored view --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("wk", [3, 4, 7, 8])
def test_mirrored_view(dev, wk, C):
    z, (v,), _ = _maps(2, C, STUDENT, [((9, wk), False)], 1.0, 5, wk, C)
    zd = z.to(dev)
    for size in ((13, 11), (9, wk)):
        a = ops.distill_loss(zd, v.to(dev), size, temperature=2.0)
        b = ops.distill_loss(zd, [v.flip(2).contiguous().to(dev)], size, flips=[True], temperature=2.0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        c = ops.distill_loss(zd, [v.to(dev), v.flip(2).contiguous().to(dev)], size, flips=[False, True], temperature=2.0)
        assert torch.equal(a[1], c[1])                       # the mean of two equal distributions: (q + q) / 2 is exact


# ---- 5. accumulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 8, 12])
def test_accumulation(dev, C):
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 6, C)
    zd, td = z.to(dev), [t.to(dev) for t in ts]
    loss, fresh = ops.distill_loss(zd, td, (13, 11), flips=flips, temperature=2.0, grad_scale=3.0)
    dz0 = torch.randn(fresh.shape, generator=_gen(7, C)).to(dev) * float(fresh.abs().max())
    given = dz0.clone()
    loss2, out = ops.distill_loss(zd, td, (13, 11), flips=flips, temperature=2.0, grad_scale=3.0, dz=given)
    assert out is given and torch.equal(loss, loss2)
    assert torch.equal(out, dz0 + fresh)
    # a dz whose address allows no 16-byte access (C = 8, 12: the scalar path of a vector class count)
    store = torch.zeros(fresh.numel() + 1, device=dev)
    odd = store[1:].view(fresh.shape)
    odd.copy_(dz0)
    assert odd.data_ptr() % 16 != 0
    ops.distill_loss(zd, td, (13, 11), flips=flips, temperature=2.0, grad_scale=3.0, dz=odd)
    assert torch.equal(odd, dz0 + fresh) and float(store[0]) == 0.0


# ---- 6. determinism and scaling ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 8])
def test_determinism_and_scaling(dev, C):
    tile, _ = _tile_sizes(_lib_distill.lib(), "distill")
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 8, C)
    zd, td = z.to(dev), [t.to(dev) for t in ts]
    size = (61, 3 * tile // 61)                              # several workgroups
    runs = [ops.distill_loss(zd, td, size, flips=flips, temperature=2.0) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1])
    scratch = torch.empty(ops.distill_scratch_bytes(2 * size[0] * size[1]) + 64, device=dev, dtype=torch.uint8)
    kept = ops.distill_loss(zd, td, size, flips=flips, temperature=2.0, scratch=scratch)
    assert torch.equal(kept[0], runs[0][0]) and torch.equal(kept[1], runs[0][1])
    big = ops.distill_loss(zd, td, size, flips=flips, temperature=2.0, grad_scale=1024.0)
    assert torch.equal(big[0], runs[0][0]) and torch.equal(big[1], runs[0][1] * 1024.0)
    assert bool(runs[0][1].abs().max() > 0)


# ---- 7. argument checks ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(dev):
    g = _gen(9)
    z = torch.randn((2, 5, 7, 3), generator=g).to(dev)
    t = torch.randn((2, 6, 4, 3), generator=g).to(dev)
    dz = torch.full((2, 13, 11, 3), 7.0, device=dev)
    size = (13, 11)

    def refused(*a, exc=ValueError, **kw):
        with pytest.raises(exc):
            ops.distill_loss(*a, dz=dz, **kw)
        assert bool((dz == 7.0).all())

    refused(z, [t, t[:1]], size)                                               # differing B
    refused(z, [t, torch.zeros((2, 6, 4, 4), device=dev)], size)               # differing C among the maps
    refused(torch.zeros((2, 5, 7, 4), device=dev), t, size)                    # ... and against the student
    refused(torch.zeros((1, 5, 7, 3), device=dev), t, size)
    refused(z, [t] * 9, size)
    refused(z, [], size)
    refused(z, [t.permute(0, 2, 1, 3)], size)                                  # not contiguous
    refused(z, t.half(), size)
    refused(z.half(), t, size)
    refused(z.permute(0, 2, 1, 3), t, size)
    refused(z, [t, t], size, flips=[True])
    refused(z, t, size, flips=[False, False])
    refused(z, t, size, temperature=0.0)
    refused(z, t, size, temperature=-1.0)
    refused(z, t, (0, 11))
    refused(z, t, size, scratch=torch.empty(4, device=dev, dtype=torch.uint8))
    refused(z.cpu(), t.cpu(), size, exc=_lib.AsisError)                        # no CPU fallback
    with pytest.raises(ValueError):                                            # a dz of another shape
        ops.distill_loss(z, t, size, dz=torch.zeros((2, 13, 11, 4), device=dev))
    z17, t17 = torch.zeros((1, 2, 2, 17), device=dev), torch.zeros((1, 2, 2, 17), device=dev)
    dz17 = torch.full((1, 4, 4, 17), 7.0, device=dev)
    with pytest.raises(ValueError, match="C=17"):
        ops.distill_loss(z17, t17, (4, 4), dz=dz17)
    assert bool((dz17 == 7.0).all())
    # what is accepted: a tensor for one map, an int size, a target tensor for the size
    a = ops.distill_loss(z, t, 9)
    b = ops.distill_loss(z, [t], torch.zeros((2, 9, 9), dtype=torch.int64, device=dev))
    assert a[1].shape == (2, 9, 9, 3) and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 8. module ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("size", [(13, 11), None])
def test_module_gradient(dev, size, C):
    temp = 2.0
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 10, C)
    x = z.permute(0, 3, 1, 2).to(dev).requires_grad_(True)                     # NCHW view of an NHWC buffer
    out = DistillationLoss(temp, flips)(x, [t.permute(0, 3, 1, 2).to(dev) for t in ts], size)
    (out * 3.0).backward()
    full = STUDENT if size is None else size
    ref = R.distill_ref(z, ts, flips, full, temp)
    f32 = R.distill_ref(z, ts, flips, full, temp, torch.float32)
    bl, yl = _bound(f32[0], ref[0], U_SUM)
    bg, yg = _bound(3.0 * f32[2], 3.0 * ref[2], U_ELEM)
    el, eg = _err(out, ref[0]), _err(x.grad.permute(0, 2, 3, 1), 3.0 * ref[2])
    print(f"MEASURE distill module size={size} C={C}: loss err {el:.3e} bound {bl:.3e} (yard {yl:.2e}); "
          f"low-resolution gradient err {eg:.3e} bound {bg:.3e} (yard {yg:.2e})")
    assert x.grad.shape == x.shape and el <= bl and eg <= bg
    direct = ops.distill_loss(z.to(dev), [t.to(dev) for t in ts], full, flips=flips, temperature=temp)
    assert torch.equal(out.detach().view(1), direct[0])
