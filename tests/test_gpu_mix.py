"""GPU: ``ops.mix_batch`` (csrc/mix.hip) against the restatement of tests/mix_ref.py.  Everything is an equality: the mixed image
bit for bit (compared as integers, so a NaN is a pattern like any other), the mixed labels, ``sel`` and the pasted counts.

Shapes: W % 4 == 0 takes the 16-byte path, anything else the scalar one; a tile is ``asis_mix_tile()`` pixels of ONE sample, so the
sizes around it are pixel counts of a sample, and the case with more tiles than workgroups has B = 2 samples of cap / 2 tiles and
one pixel (or, on the 16-byte path, four) each: cap + 2 tiles.  The ABI's NULL ``pasted_sets``, which ``ops.mix_batch`` passes only
when no sample has kind 2, is called directly with such a sample.  Every case prints its pasted counts before it asserts."""
import pytest
import torch

from adaptersis_amd import _lib, _lib_mix, ops
from adaptersis_amd.tools.mix import MixSampler
from tests import mix_ref as M
from tests.bound_helpers import _gen
from tests.soft_target_helpers import _factor

pytestmark = pytest.mark.gpu

KIND_MIXES = {"none": [0, 0, 0], "cutmix": [1, 1, 1], "classmix": [2, 2, 2], "mixed": [1, 2, 0]}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _batch(B, H, W, C, *key, labels=None):
    g = _gen(*key)
    inp = torch.randn((B, 3, H, W), generator=g)
    tgt = torch.randint(0, C, (B, H, W), generator=g) if labels is None else labels
    return inp, tgt


def _tables(B, H, W, kinds, step=0, seed=1, **over):
    t = MixSampler("cutmix", seed=seed).draw(B, H, W, step)
    t["kind"] = torch.tensor(kinds, dtype=torch.int32)
    for k, v in over.items():
        t[k] = torch.as_tensor(v).to(t[k].dtype).reshape(t[k].shape).contiguous()
    return t


def _check(dev, tag, inp, tgt, tables, C, background=False):
    ref = M.mix_ref(inp, tgt, tables, C, background)
    got = ops.mix_batch(inp.to(dev), tgt.to(dev), tables, C, background)
    print(f"MEASURE mix {tag}: kind {tables['kind'].tolist()} donor {tables['donor'].tolist()} pasted {got[3].tolist()} ref "
          f"{ref[3].tolist()} of {tgt[0].numel()} pixels a sample")
    out, tout, sel, pasted = got
    assert out.dtype == torch.float32 and tout.dtype == torch.int64 and sel.dtype == torch.uint8 and pasted.dtype == torch.int32
    assert out.shape == inp.shape and tout.shape == tgt.shape and sel.shape == tgt.shape and pasted.shape == (inp.shape[0],)
    assert torch.equal(sel.cpu(), ref[2]) and torch.equal(pasted.cpu(), ref[3])
    assert torch.equal(tout.cpu(), ref[1])
    assert torch.equal(_bits(out).cpu(), _bits(ref[0]))
    return got, ref


# ---- 1. shapes, class counts, kinds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 8, 16])
@pytest.mark.parametrize("kinds", sorted(KIND_MIXES))
@pytest.mark.parametrize("size", [(5, 7), (13, 11), (8, 12)])
def test_shapes_classes_kinds(dev, size, kinds, C):
    H, W = size
    inp, tgt = _batch(3, H, W, C, 1, H, C)
    for step, background in ((0, False), (1, True), (2, False)):
        tables = _tables(3, H, W, KIND_MIXES[kinds], step, seed=C)
        (_, _, sel, pasted), _ = _check(dev, f"size={size} C={C} {kinds} bg={background} step={step}", inp, tgt, tables, C, background)
        if kinds == "none":
            assert int(pasted.sum()) == 0 and int(sel.sum()) == 0


# ---- 2. boxes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(5, 7), (8, 12)])
def test_boxes(dev, size):
    H, W = size
    inp, tgt = _batch(3, H, W, 3, 2, H)
    boxes = {"empty": (2, 3, 2, 3), "empty rows": (3, 0, 3, W), "empty columns": (0, 4, H, 4), "whole": (0, 0, H, W),
             "top": (0, 2, 2, 5), "bottom": (H - 2, 1, H, 4), "left": (1, 0, 4, 3), "right": (1, W - 3, 4, W),
             "corner": (H - 1, W - 1, H, W), "one column of a group": (0, 5, H, 6), "across groups": (1, 3, H - 1, 9 if W > 9 else W)}
    for name, box in boxes.items():
        tables = _tables(3, H, W, [1, 1, 1], box=[box] * 3)
        (_, _, sel, pasted), _ = _check(dev, f"size={size} box {name}", inp, tgt, tables, 3)
        want = (box[2] - box[0]) * (box[3] - box[1])
        assert pasted.tolist() == [want] * 3
        if name == "whole":
            assert bool(sel.all())


# ---- 3. sizes around the tile, more tiles than workgroups ------------------------------------------------------------------------
def test_sizes_around_the_tile(dev):
    lib = _lib_mix.lib()
    tile = lib.asis_mix_tile()
    for H, W in (_factor(tile - 1), (32, tile // 32), _factor(tile + 1), (tile // 4 - 1, 4), (tile // 4 + 1, 4)):
        assert lib.asis_mix_nblk(3, H * W) == 3 * -(-H * W // tile)
        inp, tgt = _batch(3, H, W, 8, 3, H, W)
        for kinds in ([1, 2, 0], [2, 1, 2]):
            _check(dev, f"tile {H}x{W}", inp, tgt, _tables(3, H, W, kinds, step=W), 8)


@pytest.mark.parametrize("vec", [False, True])
def test_more_tiles_than_workgroups(dev, vec):
    lib = _lib_mix.lib()
    tile, cap = lib.asis_mix_tile(), lib.asis_mix_nblk(1, (1 << 31) - 1)
    H, W = (cap // 2 * tile // 4 + 1, 4) if vec else _factor(cap // 2 * tile + 1)
    assert -(-H * W // tile) * 2 == cap + 2 and lib.asis_mix_nblk(2, H * W) == cap and (W % 4 == 0) == vec
    inp, tgt = _batch(2, H, W, 3, 4, int(vec))
    tables = _tables(2, H, W, [2, 1], box=[(0, 0, 0, 0), (H // 3, 0, H // 2, W)])
    (_, _, _, pasted), _ = _check(dev, f"capped grid {H}x{W}", inp, tgt, tables, 3)
    assert int(pasted[0]) > 0 and int(pasted[1]) == (H // 2 - H // 3) * W


# ---- 4. targets ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(13, 11), (8, 12)])
def test_class_sets(dev, size):
    H, W = size
    g = _gen(5, H)
    order = torch.stack([torch.randperm(16, generator=g) for _ in range(3)])
    # sample 0: background alone; 1: background and class 5; 2: five classes and the labels -100, 255
    tgt = torch.zeros((3, H, W), dtype=torch.int64)
    tgt[1, 2:5, 3:9] = 5
    tgt[2] = torch.tensor([1, 2, 3, 6, 7, -100, 255, 0])[torch.randint(0, 8, (H, W), generator=g)]
    inp, _ = _batch(3, H, W, 8, 6, H)
    for donor, want in (([1, 2, 0], [{5}, None, set()]), ([2, 0, 1], [None, set(), {5}])):
        tables = _tables(3, H, W, [2, 2, 2], donor=donor, order=order)
        sets = M.pasted_sets(tgt, tables, 8)
        for s, w in zip(sets, want):
            assert (s == w) if w is not None else (len(s) == 3 and s < {1, 2, 3, 6, 7})
        (_, tout, sel, pasted), _ = _check(dev, f"sets {size} donor={donor}", inp, tgt, tables, 8)
        b_empty, b_one = want.index(set()), want.index({5})
        assert int(pasted[b_empty]) == 0 and int(pasted[b_one]) == 18          # a donor of background alone pastes nothing
        assert not bool(torch.isin(tout[sel.bool()].cpu(), torch.tensor([0, -100, 255])).any())   # never pasted
        # with the background eligible: class 0 of the all-background donor is pasted whole
        (_, _, sel_bg, pasted_bg), _ = _check(dev, f"sets {size} donor={donor} background", inp, tgt, tables, 8, True)
        assert int(pasted_bg[b_empty]) == H * W
    # C = 4: classes 5, 6, 7 are out of range and never present
    tables = _tables(3, H, W, [2, 2, 2], donor=[1, 2, 0], order=order)
    assert M.pasted_sets(tgt, tables, 4)[0] == set()
    _check(dev, f"sets {size} C=4", inp, tgt, tables, 4)


@pytest.mark.parametrize("size", [(13, 11), (8, 12)])
def test_abi_without_class_sets(dev, size):
    """``asis_mix_apply`` with pasted_sets == NULL (``ops.mix_batch`` passes it only when no kind is 2): a sample of kind 2 pastes
    nothing, the CutMix sample beside it is mixed as ever"""
    H, W = size
    inp, tgt = _batch(3, H, W, 3, 9, H)
    tables = _tables(3, H, W, [2, 1, 0], box=[(0, 0, H, W), (1, 2, H - 1, W - 1), (0, 0, H, W)])
    ref = M.mix_ref(inp, tgt, {**tables, "kind": torch.tensor([0, 1, 0], dtype=torch.int32)}, 3)
    x, y = inp.to(dev), tgt.to(dev)
    donor, kind, box = (tables[k].to(dev) for k in ("donor", "kind", "box"))
    out, tout = torch.empty_like(x), torch.empty_like(y)
    sel, pasted = torch.empty((3, H, W), device=dev, dtype=torch.uint8), torch.empty(3, device=dev, dtype=torch.int32)
    _lib.check(_lib_mix.lib().asis_mix_apply(torch.cuda.current_stream().cuda_stream, x.data_ptr(), y.data_ptr(), donor.data_ptr(),
                                             kind.data_ptr(), box.data_ptr(), None, 3, H, W, out.data_ptr(), tout.data_ptr(),
                                             sel.data_ptr(), pasted.data_ptr()), "asis_mix_apply")
    print(f"MEASURE mix abi NULL sets {size}: pasted {pasted.tolist()} ref {ref[3].tolist()}")
    assert pasted.tolist() == [0, (H - 2) * (W - 3), 0] == ref[3].tolist()
    assert torch.equal(sel.cpu(), ref[2]) and torch.equal(tout.cpu(), ref[1]) and torch.equal(_bits(out).cpu(), _bits(ref[0]))
    assert torch.equal(_bits(out[0]), _bits(x[0])) and torch.equal(tout[0], y[0])


# ---- 5. what is not selected is not read; determinism ----------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(13, 11), (8, 12)])
def test_unselected_donor_pixels_reach_nothing_and_calls_repeat(dev, size):
    H, W = size
    inp, tgt = _batch(3, H, W, 8, 7, H)
    tables = _tables(3, H, W, [1, 2, 1], donor=[1, 2, 0], box=[(2, 3, 6, 9), (0, 0, 0, 0), (0, 0, H, W)])
    sel = M.sel_ref(tgt, tables, 8).bool()
    assert 0 < int(sel[0].sum()) < H * W and 0 < int(sel[1].sum()) < H * W
    poisoned = inp.clone()
    poisoned[1][:, ~sel[0]] = float("nan")                                     # sample 0 takes from sample 1 inside its box alone
    (out, _, _, _), _ = _check(dev, f"nan {size}", poisoned, tgt, tables, 8)
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isnan(out[1]).any())
    a = ops.mix_batch(inp.to(dev), tgt.to(dev), tables, 8)
    b = ops.mix_batch(inp.to(dev), tgt.to(dev), tables, 8)
    assert all(torch.equal(_bits(x) if x.dtype == torch.float32 else x, _bits(y) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


# ---- 6. argument checks ----------------------------------------------------------------------------------------------------------
def test_argument_checks(dev):
    inp, tgt = _batch(3, 5, 7, 3, 8)
    x, y = inp.to(dev), tgt.to(dev)
    good = _tables(3, 5, 7, [1, 2, 0])
    ops.mix_batch(x, y, good, 3)

    def refused(*a, exc=ValueError, **over):
        t = {**good, **over}
        with pytest.raises(exc):
            ops.mix_batch(*(a or (x, y)), t, 3)

    refused(donor=torch.tensor([1, 2, 3], dtype=torch.int32))                  # a donor outside the batch
    refused(donor=torch.tensor([-1, 2, 0], dtype=torch.int32))
    refused(donor=good["donor"].long())
    refused(donor=good["donor"].to(dev))                                       # the tables are host tensors
    refused(donor=good["donor"][:2])
    refused(kind=good["kind"].long())
    refused(kind=torch.zeros(4, dtype=torch.int32))
    refused(box=good["box"].t().contiguous())
    refused(box=good["box"].to(dev))
    refused(order=good["order"].int())
    refused(order=good["order"][:, :8].contiguous())
    refused(order=torch.zeros((3, 32), dtype=torch.uint8)[:, ::2])
    refused(x.double(), y)
    refused(x[:, :, :, ::2], y)
    refused(x[:, :2].contiguous(), y)
    refused(x, y.int())
    refused(x, y[:2])
    refused(x, tgt, exc=_lib.AsisError)                                        # no CPU fallback
    with pytest.raises(ValueError):
        ops.mix_batch(x, y, {k: v for k, v in good.items() if k != "order"}, 3)
    for C in (0, 17):
        with pytest.raises(ValueError, match="num_classes"):
            ops.mix_batch(x, y, good, C)
