"""GPU: class-adaptive confidence thresholds — ``ops.consistency_loss(class_threshold=)``, ``ops.confidence_stats`` and
``ops.adaptive_threshold_update`` (csrc/adapt.hip) against the float64 restatement of tests/adapt_ref.py.

Bounds (tests/bound_helpers.py as it stands): |device - float64| <= max(4 Y, U ulp32 max|ref|) with Y the error of torch's own
float32 evaluation of the restatement on the CPU, U = U_SUM for the loss and the statistics and U_ELEM for dz.  DELTA = 1e-5 as in
tests/test_gpu_consist.py: a pixel is *near* where its float64 confidence lies within DELTA of its class threshold, or where its top
two classes lie within DELTA of each other and decide differently.  The small cases and the sizes around the tile take thresholds no pixel is near
(``adapt_ref.pick_class_thresholds``, asserted on the CPU before the device is touched): kept is exact and no pixel is excused.  The
large cases take per class the midpoint of its two middle confidences: dz is compared on the pixels that are not near, the loss is
widened by what the near ones could contribute and the count by their number, and their share is asserted to be at most 0.1 %.
Everything else is an equality of bits.  Every case prints its figures before it asserts."""
import math

import pytest
import torch

from adaptersis_amd import _lib_adapt, ops
from tests import adapt_ref as A
from tests.bound_helpers import U_ELEM, U_SUM, ULP32, _bound, _err, _gen
from tests.soft_target_helpers import STUDENT, TEACHER_SETS, _bits, _factor, _maps, _tile_sizes

pytestmark = pytest.mark.gpu

DELTA = 1e-5
TEMPS = [1.0, 2.0, 4.0]
WEIGHTS = (None, [0.0, 0.5], [1.0, 1.0])


def _same(a, b):
    return torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) and torch.equal(_bits(a[2]), _bits(b[2]))


def _small(size, views, C, temp, scale):
    return _maps(2, C, STUDENT, TEACHER_SETS[views], scale, 1, size[0], len(views), C, int(temp), int(scale))


# ---- 1. the class-gated loss, small cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("C", [2, 3, 8, 16])
@pytest.mark.parametrize("views", sorted(TEACHER_SETS))
@pytest.mark.parametrize("size", [(13, 11), (5, 7)])
def test_class_gated_loss_against_float64(dev, size, views, C, temp, scale):
    z, ts, flips = _small(size, views, C, temp, scale)
    _exact(dev, f"size={size} views={views} C={C} T={temp} x{scale}", z, ts, flips, size, temp, WEIGHTS)


def _exact(dev, tag, z, ts, flips, size, temp, weight_sets=(None,)):
    """thresholds no pixel is near: kept is exact and every pixel meets the bounds"""
    q = A.soft_q(ts, flips, size, temp)
    thr, note = A.pick_class_thresholds(q, DELTA)
    assert not bool(A.near_pixels(q, thr, DELTA).any())                        # before the device is touched
    zd, td, thd = z.to(dev), [t.to(dev) for t in ts], thr.to(dev)
    for w in weight_sets:
        weights = None if w is None else torch.tensor(w)
        ref = A.adapt_consist_ref(z, ts, flips, size, temp, thr, weights)
        f32 = A.adapt_consist_ref(z, ts, flips, size, temp, thr, weights, torch.float32, gate=ref.gate)
        loss, kept, dz = ops.consistency_loss(zd, td, size, flips=flips, temperature=temp, class_threshold=thd,
                                              sample_weight=None if weights is None else weights.to(dev))
        bl, yl = _bound(f32.loss, ref.loss, U_SUM)
        bd, yd = _bound(f32.dz, ref.dz, U_ELEM)
        el, ed = _err(loss.view(()), ref.loss), _err(dz, ref.dz)
        print(f"MEASURE adapt {tag} w={w}: thr {note}; kept {int(kept)} ref {ref.kept} of {ref.gate.numel()}; loss {float(loss):.6e} "
              f"ref {float(ref.loss):.6e} err {el:.3e} bound {bl:.3e} (yard {yl:.2e}); dz err {ed:.3e} bound {bd:.3e} (yard {yd:.2e})")
        assert kept.dtype == torch.int32 and int(kept) == ref.kept
        assert math.isfinite(float(loss)) and bool(torch.isfinite(dz).all())
        assert el <= bl and ed <= bd
        drop = (~ref.gate) if weights is None else (~ref.gate | (weights.view(-1, 1, 1) <= 0))
        assert int(torch.count_nonzero(dz.cpu()[drop])) == 0                   # a fresh dz holds zeros on the dropped pixels
        if weights is None:
            assert 0.1 * ref.gate.numel() <= ref.kept <= 0.9 * ref.gate.numel()


# ---- 2. the class-gated loss, large cases and the sizes around the tile -----------------------------------------------------------
def _large(dev, N, C, B=1):
    temp = 2.0
    H, Wd = _factor(N // B)
    z, ts, flips = _maps(B, C, STUDENT, TEACHER_SETS["three"], 1.0, 2, N % 1000, C)
    q = A.soft_q(ts, flips, (H, Wd), temp)
    thr = A.middle_class_thresholds(q)
    near = A.near_pixels(q, thr, DELTA)
    n_near = int(near.sum())
    assert n_near <= 1e-3 * N, f"{n_near} of {N} pixels are near"
    ref = A.adapt_consist_ref(z, ts, flips, (H, Wd), temp, thr)
    f32 = A.adapt_consist_ref(z, ts, flips, (H, Wd), temp, thr, None, torch.float32, gate=ref.gate)
    loss, kept, dz = ops.consistency_loss(z.to(dev), [t.to(dev) for t in ts], (H, Wd), flips=flips, temperature=temp,
                                          class_threshold=thr.to(dev))
    far = ~near
    widen = temp * temp * float(ref.kd[near].sum()) / N
    bl, yl = _bound(f32.loss, ref.loss, U_SUM)
    bd, yd = _bound(f32.dz[far], ref.dz[far], U_ELEM)
    el, ed = _err(loss.view(()), ref.loss), _err(dz.cpu()[far], ref.dz[far])
    print(f"MEASURE adapt N={N}={B}x{H}x{Wd} C={C}: thr {[round(v, 4) for v in thr.tolist()]} kept {int(kept)} ref {ref.kept} "
          f"({ref.kept / N:.1%}), near {n_near} ({n_near / N:.4%}); loss {float(loss):.6e} ref {float(ref.loss):.6e} err {el:.3e} bound "
          f"{bl:.3e} + {widen:.3e} (yard {yl:.2e}); dz err {ed:.3e} bound {bd:.3e} (yard {yd:.2e})")
    assert 0.05 * N < ref.kept < 0.95 * N
    assert abs(int(kept) - ref.kept) <= n_near
    assert el <= bl + widen and ed <= bd
    assert bool(torch.isfinite(dz).all())


@pytest.mark.parametrize("C", [3, 8])
def test_class_gated_loss_257_tiles_and_one(dev, C):
    tile, _ = _tile_sizes(_lib_adapt.lib(), "adapt")
    N = 257 * tile + 1
    assert _lib_adapt.lib().asis_adapt_nblk(N) == 258
    _large(dev, N, C)


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1"])
def test_class_gated_loss_sizes_around_the_tile(dev, which, C):
    tile, _ = _tile_sizes(_lib_adapt.lib(), "adapt")
    N = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1}[which]
    assert _lib_adapt.lib().asis_adapt_nblk(N) == -(-N // tile)
    H, Wd = _factor(N)
    z, ts, flips = _maps(1, C, STUDENT, TEACHER_SETS["three"], 1.0, 2, N % 1000, C)
    _exact(dev, f"N={N}={H}x{Wd} C={C}", z, ts, flips, (H, Wd), 2.0)          # ~1000 pixels: thresholds no pixel is near


# ---- 3. equalities of bits ---------------------------------------------------------------------------------------------------------
def _mix_of(B, size, *key):
    sel = (torch.rand((B,) + tuple(size), generator=_gen(99, *key)) < 0.5).to(torch.uint8)
    return sel, [(b + 1) % B for b in range(B)]


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("mixed", [False, True])
def test_equal_thresholds_give_the_bits_of_the_scalar_gate(dev, mixed, C):
    size, temp = (13, 11), 2.0
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 21, C)
    zd, td = z.to(dev), [t.to(dev) for t in ts]
    conf = A.soft_q(ts, flips, size, temp).amax(dim=1)
    t = float(torch.tensor(float(conf.median()), dtype=torch.float32))
    kw = dict(flips=flips, temperature=temp, grad_scale=3.0)
    if mixed:
        sel, donor = _mix_of(2, size, C)
        kw["mix"] = (sel.to(dev), donor)
    full = torch.full((C,), t, device=dev)
    for w in (None, torch.tensor([0.25, 2.0], device=dev)):
        a = ops.consistency_loss(zd, td, size, threshold=t, sample_weight=w, **kw)
        b = ops.consistency_loss(zd, td, size, class_threshold=full, sample_weight=w, **kw)
        assert _same(a, b) and 0 < int(a[1]) < 2 * size[0] * size[1]
        assert _same(ops.consistency_loss(zd, td, size, class_threshold=full, sample_weight=w, **kw), b)      # two calls
        given = torch.randn(a[2].shape, generator=_gen(22, C)).to(dev)
        given[:, :, ::2] = -0.0
        ga, gb = given.clone(), given.clone()
        ra = ops.consistency_loss(zd, td, size, threshold=t, sample_weight=w, dz=ga, **kw)
        rb = ops.consistency_loss(zd, td, size, class_threshold=full, sample_weight=w, dz=gb, **kw)
        assert rb[2] is gb and _same(ra, rb) and not torch.equal(_bits(gb), _bits(given))
    # every threshold <= 0: the ungated call
    for low in (torch.zeros(C), torch.full((C,), -3.0), -torch.arange(C, dtype=torch.float32)):
        a = ops.consistency_loss(zd, td, size, class_threshold=low.to(dev), **kw)
        assert int(a[1]) == 2 * size[0] * size[1] and _same(a, ops.consistency_loss(zd, td, size, **kw))


@pytest.mark.parametrize("C", [3, 8])
def test_one_class_at_two_is_dropped(dev, C):
    size, temp = (13, 11), 1.0
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 23, C)
    zd, td = z.to(dev), [t.to(dev) for t in ts]
    q = A.soft_q(ts, flips, size, temp)
    a, conf = A.top_class(q)
    v1, v2, _, _ = A._top_two(q)
    assert float((v1 - v2).min()) > DELTA                                      # no pixel's class is in doubt
    c = int(a.flatten().bincount(minlength=C).argmax())
    thr = torch.zeros(C)
    thr[c] = 2.0
    of_c = (a == c).to(dev)
    n_c = int(of_c.sum())
    assert 0 < n_c < a.numel()
    loss, kept, dz = ops.consistency_loss(zd, td, size, flips=flips, temperature=temp, class_threshold=thr.to(dev))
    assert int(kept) == a.numel() - n_c and int(torch.count_nonzero(dz[of_c])) == 0
    free = ops.consistency_loss(zd, td, size, flips=flips, temperature=temp)
    assert torch.equal(_bits(dz[~of_c]), _bits(free[2][~of_c]))
    given = torch.randn(dz.shape, generator=_gen(24, C)).to(dev)
    given[:, :, ::2] = -0.0
    before = given.clone()
    ops.consistency_loss(zd, td, size, flips=flips, temperature=temp, class_threshold=thr.to(dev), dz=given)
    assert torch.equal(_bits(given[of_c]), _bits(before[of_c]))                # untouched: -0.0 stays -0.0
    assert torch.equal(given[~of_c], before[~of_c] + dz[~of_c])


# ---- 4. the statistics ---------------------------------------------------------------------------------------------------------------
def _stats_against_float64(dev, tag, ts, flips, size, temp, weights=None, poison=False):
    ref = A.stats_ref(ts, flips, size, temp, weights)
    f32 = A.stats_ref(ts, flips, size, temp, weights, torch.float32)
    td = [t.to(dev) for t in ts]
    if poison:                                                                 # a sample of weight 0 is not read
        for t in td:
            t[[b for b, w in enumerate(weights.tolist()) if w <= 0]] = float("nan")
    wd = None if weights is None else weights.to(dev)
    got = ops.confidence_stats(td, size, flips=flips, temperature=temp, sample_weight=wd)
    C = ts[0].shape[-1]
    assert got.dtype == torch.float64 and got.shape == (C + 2,)
    again = ops.confidence_stats(td, size, flips=flips, temperature=temp, sample_weight=wd, out=torch.empty_like(got),
                                 scratch=torch.empty(ops.confidence_stats_scratch_bytes(ts[0].shape[0] * size[0] * size[1]) + 8,
                                                     device=dev, dtype=torch.uint8))
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))         # two calls, the same bits
    b, y = _bound(f32[:C + 1], ref[:C + 1], U_SUM)
    e = _err(got[:C + 1], ref[:C + 1])
    cnt = float(ref[C + 1])
    total, ytot = abs(float(got[:C].sum()) - cnt), abs(float(f32[:C].double().sum()) - cnt)
    print(f"MEASURE adapt stats {tag}: cnt {int(got[C + 1])} ref {int(cnt)}; sums err {e:.3e} bound {b:.3e} (yard {y:.2e}, max|ref| "
          f"{float(ref[:C + 1].abs().max()):.3e}); |sum_c S_c - cnt| {total:.3e}")
    assert float(got[C + 1]) == cnt
    assert e <= b
    assert total <= max(4 * ytot, U_SUM * ULP32 * cnt)                          # every row of q sums to 1: the bound of cnt
    return got


@pytest.mark.parametrize("scale", [1.0, 30.0])
@pytest.mark.parametrize("temp", TEMPS)
@pytest.mark.parametrize("C", [2, 3, 8, 16])
@pytest.mark.parametrize("views", sorted(TEACHER_SETS))
@pytest.mark.parametrize("size", [(13, 11), (5, 7)])
def test_statistics_against_float64(dev, size, views, C, temp, scale):
    _, ts, flips = _small(size, views, C, temp, scale)
    tag = f"size={size} views={views} C={C} T={temp} x{scale}"
    full = _stats_against_float64(dev, tag, ts, flips, size, temp)
    ones = _stats_against_float64(dev, tag + " w=[1,1]", ts, flips, size, temp, torch.tensor([1.0, 1.0]))
    assert torch.equal(full, ones)
    half = _stats_against_float64(dev, tag + " w=[0,0.5]", ts, flips, size, temp, torch.tensor([0.0, 0.5]), poison=True)
    assert int(half[C + 1]) == size[0] * size[1]
    none = ops.confidence_stats([t.to(dev) for t in ts], size, flips=flips, temperature=temp, sample_weight=torch.zeros(2, device=dev))
    assert none.tolist() == [0.0] * (C + 2)


@pytest.mark.parametrize("C", [3, 8])
@pytest.mark.parametrize("which", ["tile-1", "tile", "tile+1", "257 tiles+1"])
def test_statistics_sizes(dev, which, C):
    tile, _ = _tile_sizes(_lib_adapt.lib(), "adapt")
    N = {"tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "257 tiles+1": 257 * tile + 1}[which]
    assert _lib_adapt.lib().asis_adapt_stats_nblk(N) == -(-N // tile)
    H, Wd = _factor(N)
    _, ts, flips = _maps(1, C, STUDENT, TEACHER_SETS["three"], 1.0, 2, N % 1000, C)
    _stats_against_float64(dev, f"N={N}={H}x{Wd} C={C}", ts, flips, (H, Wd), 2.0)


# ---- 5. the update -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 16])
def test_update_against_the_float64_recursion(dev, C):
    lam = 0.9
    g = _gen(31, C)
    state = A.init_state(C)
    st = torch.tensor(state, dtype=torch.float64, device=dev)
    thr = torch.full((C,), -7.0, device=dev)
    for step in range(5):
        p = torch.rand(C, generator=g, dtype=torch.float64) + 0.05
        cnt = float(1000 + 37 * step)
        sums = [float(v) * cnt for v in p / p.sum()] + [(0.4 + 0.1 * step) * cnt, cnt]
        state, want = A.update_ref(state, sums, lam)
        out = ops.adaptive_threshold_update(torch.tensor(sums, dtype=torch.float64, device=dev), st, thr, lam)
        assert out is thr
        rel = float(((st.cpu() - torch.tensor(state, dtype=torch.float64)).abs() / torch.tensor(state, dtype=torch.float64).abs()).max())
        exact = torch.tensor([state[0] * v / max(state[2:]) for v in state[2:]], dtype=torch.float64)
        off = (thr.cpu().view(torch.int32) - want.view(torch.int32)).abs().max()
        print(f"MEASURE adapt update C={C} step {step}: state rel err {rel:.3e}; thr {[round(v, 6) for v in thr.tolist()]} ulps off {int(off)}")
        assert rel <= 1e-15 and float(st[1]) == step + 1
        assert int(off) <= 1 and float((thr.cpu().double() - exact).abs().max()) <= ULP32 * float(exact.max())
    # no pixel: neither the state nor the thresholds are written
    s0, t0 = st.clone(), thr.clone()
    sums = torch.tensor([1.0] * (C + 1) + [0.0], dtype=torch.float64, device=dev)
    ops.adaptive_threshold_update(sums, st, thr, lam)
    assert torch.equal(st.view(torch.int64), s0.view(torch.int64)) and torch.equal(_bits(thr), _bits(t0))
    if C == 1:
        assert float(thr[0]) == float(torch.tensor(state[0], dtype=torch.float32))


def test_statistics_into_update_from_the_object(dev):
    """``AdaptiveThreshold.update`` is the two ops in a row, and its thresholds gate the loss they are passed to"""
    from adaptersis_amd.adaptive_threshold import AdaptiveThreshold
    C, size, temp = 3, (13, 11), 1.0
    z, ts, flips = _maps(2, C, STUDENT, TEACHER_SETS["three"], 1.0, 41, C)
    td = [t.to(dev) for t in ts]
    ad = AdaptiveThreshold(C, 0.5, dev)
    thr = ad.update(td, flips, size, temp)
    assert thr is ad.thresholds
    sums = ops.confidence_stats(td, size, flips=flips, temperature=temp)
    st = torch.tensor(A.init_state(C), dtype=torch.float64, device=dev)
    by_hand = ops.adaptive_threshold_update(sums, st, torch.empty(C, device=dev), 0.5)
    assert torch.equal(_bits(thr), _bits(by_hand)) and torch.equal(ad.state, st) and torch.equal(ad.sums, sums)
    state, want = A.update_ref(A.init_state(C), A.stats_ref(ts, flips, size, temp).tolist(), 0.5)
    assert float((thr.cpu() - want).abs().max()) <= 1e-6
    sd = ad.state_dict()
    other = AdaptiveThreshold(C, 0.5, dev)
    other.load_state_dict(sd)
    assert torch.equal(other.state.view(torch.int64), ad.state.view(torch.int64)) and torch.equal(_bits(other.thresholds), _bits(thr))
    loss, kept, dz = ops.consistency_loss(z.to(dev), td, size, flips=flips, temperature=temp, class_threshold=thr)
    q = A.soft_q(ts, flips, size, temp)
    if not bool(A.near_pixels(q, thr.cpu(), DELTA).any()):
        assert int(kept) == int(A.class_gate(q, thr.cpu()).sum())
