"""GPU: the consistency loss over a mixed batch — ``ops.consistency_loss(..., mix=(sel, donor))`` (csrc/mix.hip, the third
instantiation of csrc/soft_target.h) against the float64 restatement of tests/mix_ref.py.

Bounds and thresholds are those of tests/test_gpu_consist.py, on the MIXED confidence: |device - float64| <= max(4 Y, U ulp32
max|ref|) (tests/bound_helpers.py as it stands); the small cases take a threshold that no float64 confidence of the mixed batch is
within DELTA = 1e-5 of (``consist_ref.pick_threshold``, asserted on the CPU before the device is touched; every case found such a
gap with its first seed), the large ones the midpoint of the confidences' range with the near pixels (at most
0.1 %) set aside as there.  The identities are equalities of bits: there is one instantiation and the pixels are independent, so a
batch whose every pixel is pasted is the unmixed batch of the donors' maps, and a partly pasted one is that and the unmixed batch,
pixel by pixel.  The flat pixel count of the sizes around the tile is odd or a power of two, so each takes the smallest batch above
one that divides it (3, 2, 5; 3 for the two large sizes).  Every case prints its figures before it asserts (one MI355X, 2026-10-20:
the largest error over all cases is 0.55 of its bound for the loss and 0.43 for dz; near shares of the large cases 0.006 %, 0.006 %
and 0.002 % with the kept counts equal to the reference's; every small case found a mid-range gap)."""
import math

import pytest
import torch

from adaptersis_amd import _lib, _lib_mix, ops
from adaptersis_amd.segloss.consistency import ConsistencyLoss
from tests import consist_ref as R
from tests import mix_ref as M
from tests.bound_helpers import U_ELEM, U_SUM, _bound, _err, _gen
from tests.soft_target_helpers import STUDENT, TEACHER_SETS, _bits, _factor, _maps, _tile_sizes

pytestmark = pytest.mark.gpu

DELTA = 1e-5
TEMPS = [1.0, 2.0, 4.0]


def _same(a, b):
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(_bits(a[2]), _bits(b[2]))


def _sel(B, size, *key, share=0.5):
    return (torch.rand((B,) + tuple(size), generator=_gen(99, *key)) < share).to(torch.uint8)


def _shift(B):
    return [(b + 1) % B for b in range(B)]


def _op(dev, z, ts, size, sel, donor, **kw):
    return ops.consistency_loss(z.to(dev), [t.to(dev) for t in ts], size, mix=(sel.to(dev), donor), **kw)


def _against_float64(dev, tag, z, ts, flips, size, temp, thr, sel, donor, weights=None, note="", **kw):
    ref = M.mixed_consist_ref(z, ts, flips, size, temp, sel, donor, thr, weights)
    if thr is not None and thr > 0:
        assert float((ref.conf - thr).abs().min()) > DELTA                     # before the device is touched
    f32 = M.mixed_consist_ref(z, ts, flips, size, temp, sel, donor, thr, weights, torch.float32)
    assert torch.equal(f32.gate, ref.gate)
    wd = None if weights is None else weights.to(dev)
    loss, kept, dz = _op(dev, z, ts, size, sel, donor, flips=flips, temperature=temp, threshold=thr, sample_weight=wd, **kw)
    bl, yl = _bound(f32.loss, ref.loss, U_SUM)
    bd, yd = _bound(f32.dz, ref.dz, U_ELEM)
    el, ed = _err(loss.view(()), ref.loss), _err(dz, ref.dz)
    print(f"MEASURE mix consist {tag}: threshold {thr} ({note}) pasted {int(sel.sum())} kept {int(kept)} ref {ref.kept} of "
          f"{ref.gate.numel()}; loss {float(loss):.6e} ref {float(ref.loss):.6e} err {el:.3e} bound {bl:.3e} (yard {yl:.2e}, frac "
          f"{el / bl:.2f}); dz err {ed:.3e} bound {bd:.3e} (yard {yd:.2e}, frac {ed / bd:.2f})")
    assert kept.dtype == torch.int32 and int(kept) == ref.kept
    assert math.isfinite(float(loss)) and bool(torch.isfinite(dz).all())
    assert el <= bl and ed <= bd
    if "dz" not in kw:
        drop = (~ref.gate) if weights is None else (~ref.gate | (weights.view(-1, 1, 1) <= 0))
        assert int(torch.count_nonzero(dz.cpu()[drop])) == 0
    return (loss, kept, dz), ref


def _threshold(ts, flips, size, temp, sel, donor):
    return R.pick_threshold(M.mixed_confidence(ts, flips, size, temp, sel, donor), DELTA)


# ---- 1. against float64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("C", [2, 3, 8, 16])
@pytest.mark.parametrize("views", sorted(TEACHER_SETS))
@pytest.mark.parametrize("size", [(13, 11), (5, 7)])
def test_against_float64(dev, size, views, C, temp, scale):
    seed = 1
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS[views], scale, seed, size[0], len(views), C, int(temp), int(scale))
    sel, donor = _sel(2, size, seed, size[0], C, int(temp)), [1, 0]
    assert 0.3 < float(sel.float().mean()) < 0.7
    thr, note = _threshold(ts, flips, size, temp, sel, donor)
    for weights in (None, torch.tensor([0.0, 0.5]), torch.tensor([1.0, 1.0])):
        wtag = "none" if weights is None else weights.tolist()
        _against_float64(dev, f"size={size} views={views} C={C} T={temp} x{scale} w={wtag}", z, ts, flips, size, temp, thr, sel, donor,
                         weights, note)


# ---- 2. identities of bits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 8, 16])
@pytest.mark.parametrize("size", [(13, 11), (5, 7)])
def test_all_pasted_is_the_donors_maps_and_partly_pasted_is_both(dev, size, C):
    B = 3
    donor = [2, 0, 1]
    z, ts, flips = _maps(B, C, STUDENT, TEACHER_SETS["three"], 1.0, 21, size[0], C)
    moved = [t[donor].contiguous() for t in ts]
    ones, zeros = torch.ones((B,) + size, dtype=torch.uint8), torch.zeros((B,) + size, dtype=torch.uint8)
    sel = _sel(B, size, 21, C)
    # one threshold clear of the confidences of both batches, and so of every mixture of them
    conf1, conf0 = R.confidence(moved, flips, size, 2.0), R.confidence(ts, flips, size, 2.0)
    thr, _ = R.pick_threshold(torch.cat([conf1, conf0]), DELTA)
    kw = dict(flips=flips, temperature=2.0, threshold=thr, grad_scale=3.0)
    all1, own = _op(dev, z, ts, size, ones, donor, **kw), _op(dev, z, ts, size, zeros, donor, **kw)
    assert _same(all1, _op(dev, z, moved, size, zeros, donor, **kw))           # sel == 1 on t is sel == 0 on t[donor]
    assert _same(own, _op(dev, z, ts, size, zeros, [0, 1, 2], **kw))           # where nothing is pasted the donor is not looked at
    assert int(all1[1]) == int((conf1 >= thr).sum()) and int(own[1]) == int((conf0 >= thr).sum())
    part = _op(dev, z, ts, size, sel, donor, **kw)
    m = sel.bool().to(dev)
    assert torch.equal(_bits(part[2]), _bits(torch.where(m.unsqueeze(-1), all1[2], own[2])))
    assert int(part[1]) == int(((conf1 >= thr) & sel.bool()).sum()) + int(((conf0 >= thr) & ~sel.bool()).sum())
    assert 0 < int(part[1]) < B * size[0] * size[1] and not torch.equal(all1[2], own[2])
    print(f"MEASURE mix consist identities size={size} C={C}: threshold {thr} kept all-pasted {int(all1[1])} unmixed {int(own[1])} "
          f"partly {int(part[1])} of {B * size[0] * size[1]}")


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("wk", [3, 4, 7, 8])
def test_mirrored_view(dev, wk, C):
    z, (v,), _ = _maps(2, C, STUDENT, [((9, wk), False)], 1.0, 5, wk, C)
    for size in ((13, 11), (9, wk)):
        sel = _sel(2, size, 22, wk, C)
        thr, _ = _threshold([v], [False], size, 2.0, sel, [1, 0])
        a = _op(dev, z, [v], size, sel, [1, 0], temperature=2.0, threshold=thr)
        b = _op(dev, z, [v.flip(2).contiguous()], size, sel, [1, 0], flips=[True], temperature=2.0, threshold=thr)
        assert _same(a, b) and 0 < int(a[1]) < 2 * size[0] * size[1]


@pytest.mark.parametrize("C", [3, 8])
def test_sample_of_weight_zero_reads_neither_its_maps_nor_its_donors(dev, C):
    """samples 0 and 1 weigh nothing, and sample 2, the one reader left, pastes nothing: the maps of samples 0 (its own) and 1 (its
    donor's, and sample 1's own) are read by nobody"""
    B, size, donor = 3, (13, 11), [1, 2, 0]
    z, ts, flips = _maps(B, C, STUDENT, TEACHER_SETS["three"], 1.0, 23, C)
    sel = _sel(B, size, 23, C)
    sel[2] = 0
    thr, _ = _threshold(ts, flips, size, 2.0, sel, donor)
    w = torch.tensor([0.0, 0.0, 1.0])
    kw = dict(flips=flips, temperature=2.0, threshold=thr, sample_weight=w.to(dev))
    clean = _op(dev, z, ts, size, sel, donor, **kw)
    ref = M.mixed_consist_ref(z, ts, flips, size, 2.0, sel, donor, thr, w)
    assert int(clean[1]) == ref.kept == int(ref.gate[2].sum()) and int(torch.count_nonzero(clean[2][:2])) == 0
    zn, tn = z.clone(), [t.clone() for t in ts]
    zn[:2] = float("nan")
    for t in tn:
        t[:2] = float("nan")
    assert _same(_op(dev, zn, tn, size, sel, donor, **kw), clean) and bool(torch.isfinite(clean[2]).all())
    # accumulated: their dz is untouched (-0.0 would become +0.0 under an add of zero)
    given = torch.randn(clean[2].shape, generator=_gen(24, C)).to(dev)
    given[:2, :, ::2] = -0.0
    before = given.clone()
    out = _op(dev, zn, tn, size, sel, donor, dz=given, **kw)[2]
    assert out is given and torch.equal(_bits(given[:2]), _bits(before[:2])) and torch.equal(given[2], before[2] + clean[2][2])


@pytest.mark.parametrize("C", [2, 3, 8, 12])
def test_accumulation(dev, C):
    """kept pixels: dz_out == dz_in + fresh by torch's fp32 add; dropped pixels: dz_out is dz_in bit for bit (half of them hold
    -0.0); the 16-byte path (C = 8, 12 on an aligned dz) and the scalar one (C = 2, 3, and a dz offset by one float)"""
    size, donor = (13, 11), [1, 0]
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 25, C)
    sel = _sel(2, size, 25, C)
    thr, _ = _threshold(ts, flips, size, 2.0, sel, donor)
    gate = M.mixed_consist_ref(z, ts, flips, size, 2.0, sel, donor, thr).gate.to(dev)
    assert 0 < int(gate.sum()) < gate.numel()
    kw = dict(flips=flips, temperature=2.0, threshold=thr, grad_scale=3.0)
    loss, kept, fresh = _op(dev, z, ts, size, sel, donor, **kw)
    assert int(kept) == int(gate.sum()) and int(torch.count_nonzero(fresh[~gate])) == 0
    dz0 = torch.randn(fresh.shape, generator=_gen(26, C)).to(dev) * float(fresh.abs().max())
    dz0[:, :, ::2][~gate[:, :, ::2]] = -0.0
    want = torch.where(gate.unsqueeze(-1), dz0 + fresh, dz0)
    given = dz0.clone()
    loss2, kept2, out = _op(dev, z, ts, size, sel, donor, dz=given, **kw)
    assert out is given and torch.equal(loss, loss2) and torch.equal(kept, kept2) and torch.equal(_bits(out), _bits(want))
    store = torch.zeros(fresh.numel() + 1, device=dev)
    odd = store[1:].view(fresh.shape)
    odd.copy_(dz0)
    assert odd.data_ptr() % 16 != 0
    _op(dev, z, ts, size, sel, donor, dz=odd, **kw)
    assert torch.equal(_bits(odd), _bits(want)) and float(store[0]) == 0.0
    again = _op(dev, z, ts, size, sel, donor, **kw)                             # bit-identical from call to call
    assert _same(again, (loss, kept, fresh))


# ---- 3. sizes around the tile, more workgroups than one sweep of the finalize kernel, more tiles than workgroups ------------------
def _batch_of(N):
    """the smallest batch above one that divides N, and the frame of a sample"""
    B = next(d for d in range(2, N + 1) if N % d == 0)
    return B, _factor(N // B)


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1"])
def test_sizes_around_the_tile(dev, which, C):
    tile, _ = _tile_sizes(_lib_mix.lib(), "mix_consist")
    N = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[which]
    assert _lib_mix.lib().asis_mix_consist_nblk(N) == -(-N // tile)
    B, (H, Wd) = _batch_of(N)
    z, ts, flips = _maps(B, C, STUDENT, TEACHER_SETS["three"], 1.0, 2, N % 1000, C)
    sel, donor = _sel(B, (H, Wd), N % 1000, C), _shift(B)
    thr, note = _threshold(ts, flips, (H, Wd), 2.0, sel, donor)
    _against_float64(dev, f"N={N}={B}x{H}x{Wd} C={C}", z, ts, flips, (H, Wd), 2.0, thr, sel, donor, None, note)


def _large(dev, N, C, views, *key):
    """N pixels at the midpoint threshold: dz on the pixels that are not near, the loss and the kept count widened by the near ones"""
    temp = 2.0
    B, (H, Wd) = _batch_of(N)
    z, ts, flips = _maps(B, C, STUDENT, TEACHER_SETS[views], 1.0, *key)
    sel, donor = _sel(B, (H, Wd), *key), _shift(B)
    conf = M.mixed_confidence(ts, flips, (H, Wd), temp, sel, donor)
    thr = float(torch.tensor((float(conf.min()) + float(conf.max())) / 2, dtype=torch.float32))
    ref = M.mixed_consist_ref(z, ts, flips, (H, Wd), temp, sel, donor, thr)
    f32 = M.mixed_consist_ref(z, ts, flips, (H, Wd), temp, sel, donor, thr, None, torch.float32, gate=ref.gate)
    near = (ref.conf - thr).abs() <= DELTA
    n_near = int(near.sum())
    assert n_near <= 1e-3 * N, f"{n_near} of {N} pixels lie within {DELTA} of the threshold"
    loss, kept, dz = _op(dev, z, ts, (H, Wd), sel, donor, flips=flips, temperature=temp, threshold=thr)
    far = ~near
    widen = temp * temp * float(ref.kd[near].sum()) / N
    bl, yl = _bound(f32.loss, ref.loss, U_SUM)
    bd, yd = _bound(f32.dz[far], ref.dz[far], U_ELEM)
    el, ed = _err(loss.view(()), ref.loss), _err(dz.cpu()[far], ref.dz[far])
    print(f"MEASURE mix consist N={N}={B}x{H}x{Wd} C={C}: threshold {thr:.6f} kept {int(kept)} ref {ref.kept} ({ref.kept / N:.1%}), near "
          f"{n_near} ({n_near / N:.4%}); loss {float(loss):.6e} ref {float(ref.loss):.6e} err {el:.3e} bound {bl:.3e} + {widen:.3e} "
          f"(yard {yl:.2e}, frac {el / (bl + widen):.2f}); dz err {ed:.3e} bound {bd:.3e} (yard {yd:.2e}, frac {ed / bd:.2f})")
    assert 0.05 * N < ref.kept < 0.95 * N
    assert abs(int(kept) - ref.kept) <= n_near
    assert el <= bl + widen and ed <= bd
    assert bool(torch.isfinite(dz).all())


@pytest.mark.parametrize("C", [3, 8])
def test_257_tiles_and_one(dev, C):
    tile, _ = _tile_sizes(_lib_mix.lib(), "mix_consist")
    N = 257 * tile + 1
    assert _lib_mix.lib().asis_mix_consist_nblk(N) == 258
    _large(dev, N, C, "three", 2, N % 1000, C)


def test_more_tiles_than_workgroups(dev):
    """a workgroup walks several tiles (the grid is capped); C = 3 only, as in tests/test_gpu_consist.py"""
    tile, cap = _tile_sizes(_lib_mix.lib(), "mix_consist")
    N = cap * tile + 1
    assert _lib_mix.lib().asis_mix_consist_nblk(N) == cap
    _large(dev, N, 3, "other", 3)


# ---- 4. argument checks ------------------------------------------------------------------------------------------------------------
def test_argument_checks(dev):
    g = _gen(9)
    z = torch.randn((2, 5, 7, 3), generator=g).to(dev)
    t = torch.randn((2, 6, 4, 3), generator=g).to(dev)
    dz = torch.full((2, 13, 11, 3), 7.0, device=dev)
    size = (13, 11)
    sel = _sel(2, size, 9).to(dev)

    def refused(mix, exc=ValueError, **kw):
        with pytest.raises(exc):
            ops.consistency_loss(z, t, size, dz=dz, mix=mix, **kw)
        assert bool((dz == 7.0).all())

    for donor in ([0, 2], [-1, 0], [1], [1, 0, 1], torch.tensor([1, 0]), torch.tensor([1, 0], dtype=torch.int32).to(dev),
                  torch.tensor([2, 0], dtype=torch.int32)):
        refused((sel, donor))                                                  # a bad table never reaches the device
    refused((sel[:1], [1, 0]))
    refused((sel[:, :12].contiguous(), [1, 0]))
    refused((sel.view(2, 11, 13), [1, 0]))
    refused((sel.bool(), [1, 0]))
    refused((sel.float(), [1, 0]))
    refused((sel.cpu(), [1, 0]))
    refused((torch.zeros((2, 13, 22), dtype=torch.uint8, device=dev)[:, :, ::2], [1, 0]))
    refused((sel,))
    refused(sel)
    refused((sel, [1, 0]), threshold=1.5)                                      # what the unmixed call refuses
    refused((sel, [1, 0]), temperature=0.0)
    refused((sel, [1, 0]), sample_weight=torch.ones(3, device=dev))
    a = ops.consistency_loss(z, t, size, threshold=0.5, mix=(sel, [1, 0]))
    b = ops.consistency_loss(z, [t], size, threshold=0.5, mix=(sel, torch.tensor([1, 0], dtype=torch.int32)))
    assert a[2].shape == (2, 13, 11, 3) and a[1].shape == (1,) and _same(a, b)


# ---- 5. module ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 8])
def test_module_passes_the_keyword_through(dev, C):
    temp, size, donor = 2.0, (13, 11), [1, 0]
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 10, C)
    sel = _sel(2, size, 10, C)
    thr, note = _threshold(ts, flips, size, temp, sel, donor)
    x = z.permute(0, 3, 1, 2).to(dev).requires_grad_(True)
    mod = ConsistencyLoss(temp, thr, flips)
    out = mod(x, [t.permute(0, 3, 1, 2).to(dev) for t in ts], size, None, mix=(sel.to(dev), donor))
    (out * 3.0).backward()
    ref = M.mixed_consist_ref(z, ts, flips, size, temp, sel, donor, thr)
    f32 = M.mixed_consist_ref(z, ts, flips, size, temp, sel, donor, thr, None, torch.float32)
    bl, yl = _bound(f32.loss, ref.loss, U_SUM)
    bg, yg = _bound(3.0 * f32.dlow, 3.0 * ref.dlow, U_ELEM)
    el, eg = _err(out, ref.loss), _err(x.grad.permute(0, 2, 3, 1), 3.0 * ref.dlow)
    print(f"MEASURE mix consist module C={C} threshold {thr} ({note}): kept {int(mod.last_kept)} ref {ref.kept}; loss err {el:.3e} bound "
          f"{bl:.3e}; low-resolution gradient err {eg:.3e} bound {bg:.3e}")
    assert int(mod.last_kept) == ref.kept and el <= bl and eg <= bg
    direct = _op(dev, z, ts, size, sel, donor, flips=flips, temperature=temp, threshold=thr)
    assert torch.equal(out.detach().view(1), direct[0])
