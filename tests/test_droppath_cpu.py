"""CPU: stochastic depth of the unfrozen ViT — constructor rates, the host sampler (sizes, frequencies, determinism, draw order),
the index tables, and the command-line flags.  No GPU: nothing here launches a kernel."""
import math

import numpy as np
import pytest
import torch

from adaptersis_amd import droppath
from adaptersis_amd.dinov2.layers.blocks import Block
from adaptersis_amd.dinov2.models import vision_transformer as vits
from adaptersis_amd.droppath import DropPathSampler


# ---- rates and refusals ------------------------------------------------------------------------------------------------------
def test_constructor_accepts_rate_and_spreads_it_like_fp32_linspace():
    m = vits.vit_tiny_test(drop_path_rate=0.3)
    want = [x.item() for x in torch.linspace(0, 0.3, 4)]
    assert [blk.sample_drop_ratio for blk in m.blocks] == want
    assert want[0] == 0.0 and want[-1] == pytest.approx(0.3, abs=1e-7)


def test_uniform_rate():
    m = vits.vit_tiny_test(drop_path_rate=0.25, drop_path_uniform=True)
    assert [blk.sample_drop_ratio for blk in m.blocks] == [0.25] * 4


def test_rate_zero_is_the_default():
    assert [blk.sample_drop_ratio for blk in vits.vit_tiny_test().blocks] == [0.0] * 4


@pytest.mark.parametrize("bad", [1.0, -0.1, 1.5])
def test_rate_outside_unit_interval_is_refused(bad):
    with pytest.raises(ValueError):
        vits.vit_tiny_test(drop_path_rate=bad)


def test_other_refusals_stay():
    with pytest.raises(ValueError):
        vits.vit_tiny_test(drop_path_rate=0.1, num_register_tokens=4)
    with pytest.raises(ValueError):
        vits.vit_tiny_test(drop_path_rate=0.1, interpolate_antialias=True)
    Block(128, 2, drop_path=0.2)                      # accepted now
    with pytest.raises(ValueError):
        Block(128, 2, drop_path=0.2, drop=0.1)        # dropout inside the block is still refused


# ---- sampler: subset mode ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [1, 2, 3, 12])
@pytest.mark.parametrize("p", [0.11, 0.25, 0.4, 0.9])
def test_subset_sizes_and_alpha(b, p):
    s = DropPathSampler([p], seed=3, rank=0)
    for _ in range(5):
        (ka, kf), = s.plan([(b, 7), (b, 6)])
        for spec in (ka, kf):
            assert len(spec) == 2
            for idx, alpha in spec:
                k = max(int(b * (1 - p)), 1)
                assert len(idx) == k == droppath.keep_count(b, p)
                assert len(set(idx)) == k and all(0 <= i < b for i in idx)
                assert alpha == b / k


def test_subset_is_a_permutation_prefix_not_sorted():
    s = DropPathSampler([0.5], seed=0)
    seen_unsorted = False
    for _ in range(50):
        (ka, _), = s.plan([(12, 3)])
        idx = ka[0][0]
        seen_unsorted |= idx != sorted(idx)
    assert seen_unsorted            # kept samples come in drawn order


# ---- sampler: DropPath mode --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.05, 0.1])
def test_droppath_mode_alpha_and_frequency(p):
    s = DropPathSampler([p], seed=11)
    b, rounds = 20, 500                      # 2 branches x 500 x 20 = 20 000 independent draws
    kept = total = 0
    for _ in range(rounds):
        (ka, kf), = s.plan([(b, 5)])
        for spec in (ka, kf):
            idx, alpha = spec[0]
            assert alpha == 1.0 / (1.0 - p)
            assert len(set(idx)) == len(idx) and all(0 <= i < b for i in idx)
            kept += len(idx)
            total += b
    assert total == 20000
    se = math.sqrt(p * (1 - p) / total)
    assert abs(kept / total - (1 - p)) <= 4 * se


def test_droppath_mode_can_keep_nothing_or_everything():
    s = DropPathSampler([0.1], seed=5)
    sizes = set()
    for _ in range(400):
        (ka, kf), = s.plan([(1, 4)])
        sizes |= {len(ka[0][0]), len(kf[0][0])}
    assert sizes == {0, 1}


# ---- sampler: draws ----------------------------------------------------------------------------------------------------------
RATES = [0.0, 0.05, 0.2, 0.4]
SEGS = [(6, 11), (6, 10)]


def test_same_seed_and_rank_same_plan_other_rank_differs():
    a = [DropPathSampler(RATES, seed=7, rank=1).plan(SEGS) for _ in range(2)]
    assert a[0] == a[1]
    b = DropPathSampler(RATES, seed=7, rank=2).plan(SEGS)
    c = DropPathSampler(RATES, seed=8, rank=1).plan(SEGS)
    assert a[0] != b and a[0] != c
    s = DropPathSampler(RATES, seed=7, rank=1)
    assert s.plan(SEGS) == a[0] and s.plan(SEGS) != a[0]      # the generator advances from step to step


def test_rate_zero_block_gets_none_and_draws_nothing():
    plan = DropPathSampler(RATES, seed=7, rank=1).plan(SEGS)
    assert plan[0] is None and all(p is not None for p in plan[1:])
    # dropping the rate-0 block from the list changes nothing for the others: it consumed no random numbers
    assert DropPathSampler(RATES[1:], seed=7, rank=1).plan(SEGS) == plan[1:]


def test_draw_order_is_block_major_attention_first_segments_in_order():
    plan = DropPathSampler(RATES, seed=7, rank=1).plan(SEGS)
    rng = np.random.default_rng([7, 1])
    for p, entry in zip(RATES, plan):
        if p == 0.0:
            continue
        for branch in entry:                 # attention, then FFN
            for (b, _), (idx, alpha) in zip(SEGS, branch):
                if p > 0.1:
                    k = max(int(b * (1 - p)), 1)
                    assert idx == [int(i) for i in rng.permutation(b)[:k]] and alpha == b / k
                else:
                    u = rng.random(b)
                    assert idx == [j for j in range(b) if u[j] >= p]


# ---- index tables ------------------------------------------------------------------------------------------------------------
def test_branch_words_layout():
    segs = [(3, 7), (3, 6)]
    words, csegs, K, S, rows, rows_c = droppath.branch_words(segs, [([2, 0], 1.5), ([], 3.0)])
    assert (K, S, rows, rows_c) == (2, 6, 39, 14) and csegs == [(2, 7)]
    assert words.dtype == np.int32 and words.size == 3 * K + 3 * S + 2
    cpre, src = words[:3], words[3:5]
    alpha = words[5:7].view(np.float32)
    spre, cpos = words[7:14], words[14:20]
    assert list(cpre) == [0, 7, 14] and list(src) == [14, 0] and list(alpha) == [1.5, 1.5]
    assert list(spre) == [0, 7, 14, 21, 27, 33, 39] and list(cpos) == [7, -1, 0, -1, -1, -1]


@pytest.mark.parametrize("idx", [[0, 0], [3], [-1]])
def test_branch_words_refuses_bad_lists(idx):
    with pytest.raises(ValueError):
        droppath.branch_words([(3, 4)], [(idx, 1.0)])


def test_pack_on_cpu_shares_one_buffer():
    plan = DropPathSampler([0.0, 0.4], seed=1).plan(SEGS)
    packed = droppath.pack(plan, SEGS, "cpu")
    assert packed[0] is None
    ka, kf = packed[1]
    assert ka.tab.untyped_storage().data_ptr() == kf.tab.untyped_storage().data_ptr()
    assert ka.tab.numel() == 3 * ka.K + 3 * ka.S + 2 and ka.rows == 6 * 21 and ka.rows_c == 3 * 21
    assert ka.segs == [(3, 11), (3, 10)]


# ---- command line ------------------------------------------------------------------------------------------------------------
def test_parser_flags():
    from adaptersis_amd import train as T
    p = T.get_args_parser()
    a = p.parse_args([])
    assert (a.train_backbone, a.optimize_backbone, a.drop_path, a.drop_path_uniform, a.drop_path_seed) == (False, False, 0.0, False, 0)
    assert T._backbone_args(a) == {}
    a = p.parse_args(["--train_adapters", "--train_backbone", "--optimize_backbone", "--drop_path", "0.2", "--drop_path_uniform",
                      "--drop_path_seed", "5"])
    assert (a.train_backbone, a.optimize_backbone, a.drop_path, a.drop_path_uniform, a.drop_path_seed) == (True, True, 0.2, True, 5)
    assert T._backbone_args(a) == {"train_backbone": True, "optimize_backbone": True, "drop_path_seed": 5}


@pytest.mark.parametrize("argv", [["--train_backbone"], ["--drop_path", "0.2"], ["--train_adapters", "--drop_path", "0.2"],
                                  ["--train_adapters", "--optimize_backbone"],
                                  ["--train_adapters", "--train_backbone", "--drop_path", "1.0"]])
def test_parser_refuses_flags_no_engine_can_be_built_from(argv):
    from adaptersis_amd import train as T
    with pytest.raises(SystemExit):
        T.get_args_parser().parse_args(argv)


def test_derived_parsers_inherit_the_flags():
    from adaptersis_amd import train_mla, train_multi_class
    for mod in (train_mla, train_multi_class):
        a = mod.get_args_parser().parse_args(["--train_adapters", "--train_backbone", "--drop_path", "0.15"])
        assert a.train_backbone and a.drop_path == 0.15
        with pytest.raises(SystemExit):
            mod.get_args_parser().parse_args(["--train_backbone"])
