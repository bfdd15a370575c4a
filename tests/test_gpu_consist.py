"""GPU: the gated consistency loss — ``ops.consistency_loss`` (csrc/consist.hip) against the float64 restatement of
tests/consist_ref.py, and ``ConsistencyLoss``.

Bounds (tests/bound_helpers.py as it stands): for the loss and for dz, |device - float64| <= max(4 Y, U ulp32 max|ref|) with Y the
error of torch's own float32 evaluation of the restatement on the CPU, U = U_SUM for the loss and U_ELEM for dz.

The gate compares a float32 confidence, a mean of float32 softmaxes good to about 1e-7, with the threshold, so a pixel whose float64
confidence lies within DELTA = 1e-5 of the threshold (a hundred times that) may gate either way.  The small cases choose a threshold no
pixel is near (``consist_ref.pick_threshold``, asserted on the CPU before the device is touched): the kept count is then exact and
every pixel meets the bounds.  The large cases take the midpoint of the confidences' range: dz is compared on the pixels that are
not near, the loss bound is widened by what the near pixels could contribute and the kept count by their number, and their share is
asserted to be at most 0.1 %.  Everything else is an equality of bits.  Every case prints its figures before it asserts (one
MI355X, 2026-10-20: the largest error over all cases is 0.70 of its bound for the loss and 0.43 for dz; near shares of the large
cases 0.005 %, 0.034 % and 0.036 % with the kept counts equal to the reference's; every small case found a mid-range gap)."""
import math

import pytest
import torch

from adaptersis_amd import _lib, _lib_consist, ops
from adaptersis_amd.segloss.consistency import ConsistencyLoss
from tests import consist_ref as R
from tests import distill_ref as D
from tests.bound_helpers import U_ELEM, U_SUM, _bound, _err, _gen
from tests.soft_target_helpers import STUDENT, TEACHER_SETS, _bits, _factor, _maps, _tile_sizes

pytestmark = pytest.mark.gpu

DELTA = 1e-5
TEMPS = [1.0, 2.0, 4.0]


def _same(a, b):
    """(loss, kept, dz) triples equal bit for bit"""
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(_bits(a[2]), _bits(b[2]))


def _against_float64(dev, tag, z, ts, flips, size, temp, thr, weights=None, note="", **kw):
    """one call of the op, at a threshold no pixel is near, against the restatement in float64, bounded by its float32 evaluation
    -> (loss, kept, dz) on the device, the reference"""
    ref = R.consist_ref(z, ts, flips, size, temp, thr, weights)
    if thr is not None and thr > 0:
        assert float((ref.conf - thr).abs().min()) > DELTA                     # before the device is touched
    f32 = R.consist_ref(z, ts, flips, size, temp, thr, weights, torch.float32)
    assert torch.equal(f32.gate, ref.gate)
    wd = None if weights is None else weights.to(dev)
    loss, kept, dz = ops.consistency_loss(z.to(dev), [t.to(dev) for t in ts], size, flips=flips, temperature=temp, threshold=thr,
                                          sample_weight=wd, **kw)
    bl, yl = _bound(f32.loss, ref.loss, U_SUM)
    bd, yd = _bound(f32.dz, ref.dz, U_ELEM)
    el, ed = _err(loss.view(()), ref.loss), _err(dz, ref.dz)
    print(f"MEASURE consist {tag}: threshold {thr} ({note}) kept {int(kept)} ref {ref.kept} of {ref.gate.numel()}; loss {float(loss):.6e} "
          f"ref {float(ref.loss):.6e} err {el:.3e} bound {bl:.3e} (yard {yl:.2e}); dz err {ed:.3e} bound {bd:.3e} (yard {yd:.2e}, "
          f"max|ref| {float(ref.dz.abs().max()):.3e})")
    assert kept.dtype == torch.int32 and int(kept) == ref.kept
    assert math.isfinite(float(loss)) and bool(torch.isfinite(dz).all())
    assert el <= bl and ed <= bd
    if "dz" not in kw:
        drop = (~ref.gate) if weights is None else (~ref.gate | (weights.view(-1, 1, 1) <= 0))
        assert int(torch.count_nonzero(dz.cpu()[drop])) == 0                   # a fresh dz holds zeros on the dropped pixels
    return (loss, kept, dz), ref


def _threshold(ts, flips, size, temp):
    return R.pick_threshold(R.confidence(ts, flips, size, temp), DELTA)


# ---- 1. against float64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("C", [2, 3, 8, 16])
@pytest.mark.parametrize("views", sorted(TEACHER_SETS))
@pytest.mark.parametrize("size", [(13, 11), (5, 7)])
def test_against_float64(dev, size, views, C, temp, scale):
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS[views], scale, 1, size[0], len(views), C, int(temp), int(scale))
    thr, note = _threshold(ts, flips, size, temp)
    for weights in (None, torch.tensor([0.0, 0.5]), torch.tensor([1.0, 1.0])):
        wtag = "none" if weights is None else weights.tolist()
        _against_float64(dev, f"size={size} views={views} C={C} T={temp} x{scale} w={wtag}", z, ts, flips, size, temp, thr, weights, note)


# ---- 2. without gate and weights: the plain distillation term ---------------------------------------------------------------------
def _against_distill_ref(dev, tag, z, ts, flips, size, temp):
    ref = D.distill_ref(z, ts, flips, size, temp)
    f32 = D.distill_ref(z, ts, flips, size, temp, torch.float32)
    loss, kept, dz = ops.consistency_loss(z.to(dev), [t.to(dev) for t in ts], size, flips=flips, temperature=temp)
    bl, yl = _bound(f32[0], ref[0], U_SUM)
    bd, yd = _bound(f32[1], ref[1], U_ELEM)
    el, ed = _err(loss.view(()), ref[0]), _err(dz, ref[1])
    print(f"MEASURE consist ungated {tag}: loss {float(loss):.6e} ref {float(ref[0]):.6e} err {el:.3e} bound {bl:.3e} (yard {yl:.2e}); "
          f"dz err {ed:.3e} bound {bd:.3e} (yard {yd:.2e})")
    assert int(kept) == dz.numel() // dz.shape[-1] and math.isfinite(float(loss)) and bool(torch.isfinite(dz).all())
    assert el <= bl and ed <= bd
    return loss


@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("C", [2, 3, 8, 16])
@pytest.mark.parametrize("views", sorted(TEACHER_SETS))
def test_reduces_to_the_plain_term(dev, views, C, temp):
    for scale in (1.0, 30.0):
        z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS[views], scale, 12, len(views), C, int(temp), int(scale))
        _against_distill_ref(dev, f"views={views} C={C} T={temp} x{scale}", z, ts, flips, (13, 11), temp)


@pytest.mark.parametrize("views", ["other", "three"])
@pytest.mark.parametrize("C", [3, 8])
def test_zero_log_zero_and_saturated_student(dev, C, views):
    """one teacher class at -1e4 in every map (q_c = 0 in float32 and in float64: the term is 0), the student at -300 in a class
    the teacher holds likely (p_c = 0 in float32, log p_c finite); ungated, and gated at a threshold clear of every pixel"""
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS[views], 1.0, 11, C, len(views))
    for t in ts:
        t[..., 0] = -1e4
    z[..., 1] = -300.0
    assert bool((D.soft_targets(ts, flips, (13, 11), 1.0)[:, 0] == 0).all())
    assert bool((torch.softmax(D._resized(z, (13, 11)), 1)[:, 1] == 0).all())
    loss = _against_distill_ref(dev, f"0log0 views={views} C={C}", z, ts, flips, (13, 11), 1.0)
    assert float(loss) > 10.0
    thr, note = _threshold(ts, flips, (13, 11), 1.0)
    _against_float64(dev, f"0log0 gated views={views} C={C}", z, ts, flips, (13, 11), 1.0, thr, None, note)


# ---- 3. sizes around the tile, more workgroups than one sweep of the finalize kernel, more tiles than workgroups ------------------
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1"])
def test_sizes_around_the_tile(dev, which, C):
    tile, _ = _tile_sizes(_lib_consist.lib(), "consist")
    N = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[which]
    assert _lib_consist.lib().asis_consist_nblk(N) == -(-N // tile)
    H, Wd = _factor(N)
    z, ts, flips = _maps(1, C, STUDENT, TEACHER_SETS["three"], 1.0, 2, N % 1000, C)
    thr, note = _threshold(ts, flips, (H, Wd), 2.0)
    _against_float64(dev, f"N={N}={H}x{Wd} C={C}", z, ts, flips, (H, Wd), 2.0, thr, None, note)


def _large(dev, N, C, views, *key):
    """N pixels at the midpoint threshold: dz on the pixels that are not near, the loss and the kept count widened by the near ones"""
    temp = 2.0
    H, Wd = _factor(N)
    z, ts, flips = _maps(1, C, STUDENT, TEACHER_SETS[views], 1.0, *key)
    conf = R.confidence(ts, flips, (H, Wd), temp)
    thr = float(torch.tensor((float(conf.min()) + float(conf.max())) / 2, dtype=torch.float32))
    ref = R.consist_ref(z, ts, flips, (H, Wd), temp, thr)
    f32 = R.consist_ref(z, ts, flips, (H, Wd), temp, thr, None, torch.float32, gate=ref.gate)
    near = (ref.conf - thr).abs() <= DELTA
    n_near = int(near.sum())
    assert n_near <= 1e-3 * N, f"{n_near} of {N} pixels lie within {DELTA} of the threshold"
    loss, kept, dz = ops.consistency_loss(z.to(dev), [t.to(dev) for t in ts], (H, Wd), flips=flips, temperature=temp, threshold=thr)
    far = ~near
    widen = temp * temp * float(ref.kd[near].sum()) / N
    bl, yl = _bound(f32.loss, ref.loss, U_SUM)
    bd, yd = _bound(f32.dz[far], ref.dz[far], U_ELEM)
    el, ed = _err(loss.view(()), ref.loss), _err(dz.cpu()[far], ref.dz[far])
    print(f"MEASURE consist N={N}={H}x{Wd} C={C}: threshold {thr:.6f} kept {int(kept)} ref {ref.kept} ({ref.kept / N:.1%}), near "
          f"{n_near} ({n_near / N:.4%}); loss {float(loss):.6e} ref {float(ref.loss):.6e} err {el:.3e} bound {bl:.3e} + {widen:.3e} "
          f"(yard {yl:.2e}); dz err {ed:.3e} bound {bd:.3e} (yard {yd:.2e})")
    assert 0.05 * N < ref.kept < 0.95 * N
    assert abs(int(kept) - ref.kept) <= n_near
    assert el <= bl + widen and ed <= bd
    assert bool(torch.isfinite(dz).all())


@pytest.mark.parametrize("C", [3, 8])
def test_257_tiles_and_one(dev, C):
    tile, _ = _tile_sizes(_lib_consist.lib(), "consist")
    N = 257 * tile + 1
    assert _lib_consist.lib().asis_consist_nblk(N) == 258
    _large(dev, N, C, "three", 2, N % 1000, C)


def test_more_tiles_than_workgroups(dev):
    """a workgroup walks several tiles (the grid is capped); C = 3 only: the walk does not depend on the store path, and the
    float64 restatement of 2 M pixels x 8 classes would take the seconds a test has"""
    tile, cap = _tile_sizes(_lib_consist.lib(), "consist")
    N = cap * tile + 1
    assert _lib_consist.lib().asis_consist_nblk(N) == cap
    _large(dev, N, 3, "other", 3)


# ---- 4. equalities of bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 8, 16])
@pytest.mark.parametrize("size", [(13, 11), (5, 7)])
def test_student_is_the_teacher(dev, size, C):
    for scale in (1.0, 30.0):
        z, _, _ = _maps(2, C, STUDENT, [], scale, 4, C, int(scale))
        for temp in TEMPS:
            thr, note = _threshold([z], [False], size, temp)
            (loss, kept, dz), ref = _against_float64(dev, f"self size={size} C={C} T={temp} x{scale}", z, [z], [False], size, temp, thr,
                                                     None, note)
            assert int(torch.count_nonzero(dz)) == 0 and float(loss) == 0.0
            assert int(kept) == int((ref.conf >= thr).sum())                  # the gate still counts


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("wk", [3, 4, 7, 8])
def test_mirrored_view(dev, wk, C):
    z, (v,), _ = _maps(2, C, STUDENT, [((9, wk), False)], 1.0, 5, wk, C)
    zd = z.to(dev)
    for size in ((13, 11), (9, wk)):
        thr, _ = _threshold([v], [False], size, 2.0)
        a = ops.consistency_loss(zd, v.to(dev), size, temperature=2.0, threshold=thr)
        b = ops.consistency_loss(zd, [v.flip(2).contiguous().to(dev)], size, flips=[True], temperature=2.0, threshold=thr)
        assert _same(a, b) and 0 < int(a[1]) < 2 * size[0] * size[1]
        c = ops.consistency_loss(zd, [v.to(dev), v.flip(2).contiguous().to(dev)], size, flips=[False, True], temperature=2.0,
                                 threshold=thr)
        assert torch.equal(a[2], c[2]) and torch.equal(a[1], c[1])            # the mean of two equal distributions: (q + q) / 2 is exact


@pytest.mark.parametrize("C", [3, 8])
def test_determinism_scaling_and_unit_weights(dev, C):
    tile, _ = _tile_sizes(_lib_consist.lib(), "consist")
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 8, C)
    zd, td = z.to(dev), [t.to(dev) for t in ts]
    size = (61, 3 * tile // 61)                              # several workgroups
    thr, _ = _threshold(ts, flips, size, 2.0)
    kw = dict(flips=flips, temperature=2.0, threshold=thr)
    runs = [ops.consistency_loss(zd, td, size, **kw) for _ in range(3)]
    for r in runs[1:]:
        assert _same(r, runs[0])
    scratch = torch.empty(ops.consistency_scratch_bytes(2 * size[0] * size[1]) + 64, device=dev, dtype=torch.uint8)
    assert _same(ops.consistency_loss(zd, td, size, scratch=scratch, **kw), runs[0])
    big = ops.consistency_loss(zd, td, size, grad_scale=1024.0, **kw)
    assert torch.equal(big[0], runs[0][0]) and torch.equal(big[1], runs[0][1]) and torch.equal(big[2], runs[0][2] * 1024.0)
    small = ops.consistency_loss(zd, td, size, grad_scale=2.0 ** -7, **kw)
    assert torch.equal(small[2], runs[0][2] * 2.0 ** -7)
    assert _same(ops.consistency_loss(zd, td, size, sample_weight=torch.ones(2, device=dev), **kw), runs[0])
    assert bool(runs[0][2].abs().max() > 0) and 0 < int(runs[0][1]) < 2 * size[0] * size[1]


@pytest.mark.parametrize("C", [3, 8])
def test_sample_of_weight_zero(dev, C):
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 13, C)
    zd, td = z.to(dev), [t.to(dev) for t in ts]
    size = (13, 11)
    thr, _ = _threshold(ts, flips, size, 2.0)
    kw = dict(flips=flips, temperature=2.0, threshold=thr)
    w = torch.tensor([0.0, 1.0], device=dev)
    full = ops.consistency_loss(zd, td, size, **kw)
    loss, kept, fresh = ops.consistency_loss(zd, td, size, sample_weight=w, **kw)
    assert int(torch.count_nonzero(fresh[0])) == 0 and torch.equal(_bits(fresh[1]), _bits(full[2][1]))
    ref = R.consist_ref(z, ts, flips, size, 2.0, thr)
    assert int(kept) == int(ref.gate[1].sum()) and int(full[1]) == ref.kept
    # its maps are not read: NaNs in them reach nothing
    zn, tn = zd.clone(), [t.clone() for t in td]
    zn[0] = float("nan")
    for t in tn:
        t[0] = float("nan")
    assert _same(ops.consistency_loss(zn, tn, size, sample_weight=w, **kw), (loss, kept, fresh))
    # accumulated: the sample's dz is untouched (-0.0 would become +0.0 under an add of zero)
    given = torch.randn(fresh.shape, generator=_gen(14, C)).to(dev)
    given[0, :, ::2] = -0.0
    before = given.clone()
    out = ops.consistency_loss(zd, td, size, sample_weight=w, dz=given, **kw)[2]
    assert out is given and torch.equal(_bits(given[0]), _bits(before[0]))
    assert torch.equal(given[1], before[1] + fresh[1])


# ---- 5. accumulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 8, 12])
def test_accumulation(dev, C):
    """kept pixels: dz_out == dz_in + fresh by torch's fp32 add; dropped pixels: dz_out is dz_in bit for bit (half of them hold
    -0.0, which an add of zero would turn into +0.0).  The 16-byte path (C = 8, 12 on an aligned dz) and the scalar one (C = 2, 3,
    and C = 8, 12 on a dz offset by one float)."""
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 6, C)
    zd, td = z.to(dev), [t.to(dev) for t in ts]
    size = (13, 11)
    thr, _ = _threshold(ts, flips, size, 2.0)
    gate = R.consist_ref(z, ts, flips, size, 2.0, thr).gate.to(dev)
    assert 0 < int(gate.sum()) < gate.numel()
    kw = dict(flips=flips, temperature=2.0, threshold=thr, grad_scale=3.0)
    loss, kept, fresh = ops.consistency_loss(zd, td, size, **kw)
    assert int(kept) == int(gate.sum()) and int(torch.count_nonzero(fresh[~gate])) == 0
    dz0 = torch.randn(fresh.shape, generator=_gen(7, C)).to(dev) * float(fresh.abs().max())
    dz0[:, :, ::2][~gate[:, :, ::2]] = -0.0
    want = torch.where(gate.unsqueeze(-1), dz0 + fresh, dz0)
    given = dz0.clone()
    loss2, kept2, out = ops.consistency_loss(zd, td, size, dz=given, **kw)
    assert out is given and torch.equal(loss, loss2) and torch.equal(kept, kept2)
    assert torch.equal(_bits(out), _bits(want))
    # a dz whose address allows no 16-byte access
    store = torch.zeros(fresh.numel() + 1, device=dev)
    odd = store[1:].view(fresh.shape)
    odd.copy_(dz0)
    assert odd.data_ptr() % 16 != 0
    ops.consistency_loss(zd, td, size, dz=odd, **kw)
    assert torch.equal(_bits(odd), _bits(want)) and float(store[0]) == 0.0


# ---- 6. all dropped, all kept ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 8])
def test_all_dropped_and_all_kept(dev, C):
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 15, C)
    zd = z.to(dev)
    size = (13, 11)
    N = 2 * 13 * 11
    flat = [torch.zeros_like(t).to(dev) for t in ts]                            # q = 1 / C everywhere: below a threshold of 1
    given = torch.randn((2, 13, 11, C), generator=_gen(16, C)).to(dev)
    before = given.clone()
    loss, kept, dz = ops.consistency_loss(zd, flat, size, flips=flips, threshold=1.0)
    assert float(loss) == 0.0 and int(kept) == 0 and int(torch.count_nonzero(dz)) == 0
    loss, kept, out = ops.consistency_loss(zd, flat, size, flips=flips, threshold=1.0, dz=given)
    assert float(loss) == 0.0 and int(kept) == 0 and torch.equal(_bits(out), _bits(before))
    if C == 8:    # the gate is >=: a threshold of exactly 1 / C (a power of two: exact however it is rounded) keeps them all
        _, kept, _ = ops.consistency_loss(zd, flat[:1], size, threshold=0.125)
        assert int(kept) == N
    td = [t.to(dev) for t in ts]
    lowest = float(R.confidence(ts, flips, size, 1.0).min())
    for thr in (None, 0.0, -3.0, lowest - 1e-4):
        a = ops.consistency_loss(zd, td, size, flips=flips, threshold=thr)
        b = ops.consistency_loss(zd, td, size, flips=flips)
        assert int(a[1]) == N and _same(a, b)


# ---- 7. argument checks ----------------------------------------------------------------------------------------------------------------
def test_argument_checks(dev):
    g = _gen(9)
    z = torch.randn((2, 5, 7, 3), generator=g).to(dev)
    t = torch.randn((2, 6, 4, 3), generator=g).to(dev)
    dz = torch.full((2, 13, 11, 3), 7.0, device=dev)
    size = (13, 11)

    def refused(*a, exc=ValueError, **kw):
        with pytest.raises(exc):
            ops.consistency_loss(*a, dz=dz, **kw)
        assert bool((dz == 7.0).all())

    refused(z, [t, t[:1]], size)                                               # what distill_loss refuses
    refused(z, [t, torch.zeros((2, 6, 4, 4), device=dev)], size)
    refused(torch.zeros((2, 5, 7, 4), device=dev), t, size)
    refused(z, [t] * 9, size)
    refused(z, [], size)
    refused(z, [t.permute(0, 2, 1, 3)], size)
    refused(z, t.half(), size)
    refused(z, [t, t], size, flips=[True])
    refused(z, t, size, temperature=0.0)
    refused(z, t, (0, 11))
    refused(z, t, size, scratch=torch.empty(4, device=dev, dtype=torch.uint8))
    refused(z.cpu(), t.cpu(), size, exc=_lib.AsisError)                        # no CPU fallback
    refused(z, t, size, threshold=1.5)                                         # the gate and the weights
    refused(z, t, size, threshold=float("nan"))
    refused(z, t, size, sample_weight=torch.ones(3, device=dev))
    refused(z, t, size, sample_weight=torch.ones(2, device=dev, dtype=torch.float64))
    refused(z, t, size, sample_weight=torch.ones(2, 1, device=dev))
    refused(z, t, size, sample_weight=torch.ones(2), exc=_lib.AsisError)
    z17, t17 = torch.zeros((1, 2, 2, 17), device=dev), torch.zeros((1, 2, 2, 17), device=dev)
    with pytest.raises(ValueError, match="C=17"):
        ops.consistency_loss(z17, t17, (4, 4))
    a = ops.consistency_loss(z, t, 9, threshold=0.5)
    b = ops.consistency_loss(z, [t], torch.zeros((2, 9, 9), dtype=torch.int64, device=dev), threshold=0.5)
    assert a[2].shape == (2, 9, 9, 3) and a[1].shape == (1,) and _same(a, b)


# ---- 8. module ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("size", [(13, 11), None])
def test_module_gradient(dev, size, C):
    temp = 2.0
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 10, C)
    full = STUDENT if size is None else size
    thr, note = _threshold(ts, flips, full, temp)
    w = torch.tensor([0.5, 2.0])
    x = z.permute(0, 3, 1, 2).to(dev).requires_grad_(True)                     # NCHW view of an NHWC buffer
    mod = ConsistencyLoss(temp, thr, flips)
    out = mod(x, [t.permute(0, 3, 1, 2).to(dev) for t in ts], size, w.to(dev))
    (out * 3.0).backward()
    ref = R.consist_ref(z, ts, flips, full, temp, thr, w)
    f32 = R.consist_ref(z, ts, flips, full, temp, thr, w, torch.float32)
    bl, yl = _bound(f32.loss, ref.loss, U_SUM)
    bg, yg = _bound(3.0 * f32.dlow, 3.0 * ref.dlow, U_ELEM)
    el, eg = _err(out, ref.loss), _err(x.grad.permute(0, 2, 3, 1), 3.0 * ref.dlow)
    print(f"MEASURE consist module size={size} C={C} threshold {thr} ({note}): kept {int(mod.last_kept)} ref {ref.kept}; loss err "
          f"{el:.3e} bound {bl:.3e} (yard {yl:.2e}); low-resolution gradient err {eg:.3e} bound {bg:.3e} (yard {yg:.2e})")
    assert mod.last_kept.is_cuda and mod.last_kept.dtype == torch.int32 and int(mod.last_kept) == ref.kept
    assert x.grad.shape == x.shape and el <= bl and eg <= bg
    direct = ops.consistency_loss(z.to(dev), [t.to(dev) for t in ts], full, flips=flips, temperature=temp, threshold=thr,
                                  sample_weight=w.to(dev))
    assert torch.equal(out.detach().view(1), direct[0])
