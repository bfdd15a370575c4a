"""CPU: the fused AdamW below the device — the C ABI of csrc/adamw.hip (exported, bound, argument errors without a GPU), the
parameter groups of the real modules, the quad codes of a flat bucket, the optimizer's state_dict and the command line."""
import ctypes

import pytest
import torch
from torch import nn

from adaptersis_amd import _lib, optim
from adaptersis_amd import train as T
from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
from adaptersis_amd.backbones.decoders import FeatureDecoder
from adaptersis_amd.dinov2.models import vision_transformer as vits
from adaptersis_amd.utils import weights as W

NEW = ("asis_grad_sumsq", "asis_grad_sumsq_blocks", "asis_adamw_prepare", "asis_adamw_step")
TOKENS = ("cls_token", "pos_embed", "mask_token", "register_tokens")


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_bound():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name


def test_grad_sumsq_blocks_is_positive_and_monotone():
    lib = _lib.lib()
    ns = [4, 8, 1024, 4096, 4100, 8192, 1 << 20, (1 << 23) - 4, 1 << 23, (1 << 23) + 4, 1 << 28, 1 << 33]
    blocks = [lib.asis_grad_sumsq_blocks(n) for n in ns]
    assert all(b >= 1 for b in blocks)
    assert blocks == sorted(blocks)
    assert blocks[0] == 1 and blocks[3] == 1 and blocks[4] == 2      # 4096 elements = one workgroup's single pass
    assert blocks[-1] == blocks[-2]                                   # capped: the grid-stride loop takes the rest


def _step_args(**over):
    """a valid asis_adamw_step call on made-up (aligned, never dereferenced) addresses; the checks return before any launch"""
    a = dict(stream=None, p=0x1000, g=0x2000, m=0x3000, v=0x4000, n=8, codes=0x5000, lr_scale=0x6000, wd=0x7000, n_groups=3,
             lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, inv_scale=1.0, guard=0x8000, rec=0x9000)
    a.update(over)
    return tuple(a.values())


@pytest.mark.parametrize("over,word", [
    (dict(p=None), b"null"), (dict(codes=None), b"null"), (dict(rec=None), b"null"),
    (dict(n=6), b"multiple of 4"), (dict(g=0x2004), b"aligned"), (dict(n_groups=257), b"n_groups"),
    (dict(beta1=1.0), b"beta"), (dict(beta2=-0.1), b"beta"), (dict(eps=0.0), b"eps"),
])
def test_adamw_step_argument_errors_without_a_device(over, word):
    lib = _lib.lib()
    rc = lib.asis_adamw_step(*_step_args(**over))
    assert rc == -1 and word in lib.asis_last_error(), lib.asis_last_error()
    with pytest.raises(ValueError):
        _lib.check(rc, "asis_adamw_step")


def test_sumsq_and_prepare_argument_errors_without_a_device():
    lib = _lib.lib()
    assert lib.asis_grad_sumsq(None, None, 8, 0x1000) == -1 and b"null" in lib.asis_last_error()
    assert lib.asis_grad_sumsq(None, 0x1000, 6, 0x2000) == -1 and b"multiple of 4" in lib.asis_last_error()
    assert lib.asis_grad_sumsq(None, 0x1008, 8, 0x2000) == -1 and b"aligned" in lib.asis_last_error()
    assert lib.asis_adamw_prepare(None, 0x1000, 4, None, 0x3000, 1.0, 1.0, 0.9, 0.999) == -1 and b"null" in lib.asis_last_error()
    assert lib.asis_adamw_prepare(None, 0x1000, 0, 0x2000, 0x3000, 1.0, 1.0, 0.9, 0.999) == -1 and b"n_partials" in lib.asis_last_error()
    assert lib.asis_adamw_prepare(None, 0x1000, 4, 0x2000, 0x3000, 1.0, 1.0, 1.0, 0.999) == -1 and b"beta" in lib.asis_last_error()
    assert lib.asis_adamw_prepare(None, 0x1000, 4, 0x2000, 0x3000, 0.0, 1.0, 0.9, 0.999) == -1 and b"inv_scale" in lib.asis_last_error()


# ---- param_groups_for on the real names -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def modules():
    D = W.VIT_CONFIGS["vit_small"][0]
    vit = vits.vit_small(patch_size=14, img_size=518, init_values=1e-5, ffn_layer="mlp", block_chunks=0)
    dec = FeatureDecoder(embed_dim=D, num_classes=2, features=[D, 512, 256, 128, 64])
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4)
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25)
    return vit, dec, cv, cn


def _named(mod, prefix=""):
    return [(prefix + n, tuple(p.shape)) for n, p in mod.named_parameters()]


def test_no_decay_rule_on_the_real_modules(modules):
    vit, dec, cv, cn = modules
    named = _named(dec) + _named(cv, "cross_vit.") + _named(cn, "cross_cnn.") + _named(vit)
    names, shapes = [n for n, _ in named], [s for _, s in named]
    index, table = optim.param_groups_for(names, shapes, weight_decay=0.05)
    assert len(index) == len(names) and sorted(set(table)) == [(1.0, 0.0), (1.0, 0.05)]
    seen = {"vector": 0, "token": 0, "matrix": 0}
    for n, s, gi in zip(names, shapes, index):
        scale, wd = table[gi]
        assert scale == 1.0
        if len(s) <= 1:
            assert wd == 0.0, n
            seen["vector"] += 1
        elif n.rsplit(".", 1)[-1] in TOKENS:
            assert wd == 0.0, n
            seen["token"] += 1
        else:
            assert wd == 0.05, n
            seen["matrix"] += 1
    assert seen["token"] >= 3 and seen["vector"] > 50 and seen["matrix"] > 50
    assert any(n.endswith("ls1.gamma") for n in names)            # LayerScale is among the 1-D parameters checked above
    assert any(len(s) == 4 for s in shapes)                      # ... and convolutions among the decayed ones
    # no_decay=False: one group, everything decays
    index, table = optim.param_groups_for(names, shapes, weight_decay=0.05, no_decay=False)
    assert table == [(1.0, 0.05)] and set(index) == {0}


def test_layer_decay_scales_on_a_12_block_vit(modules):
    vit = modules[0]
    assert len(vit.blocks) == 12
    named = _named(vit)
    names, shapes = [n for n, _ in named], [s for _, s in named]
    index, table = optim.param_groups_for(names, shapes, weight_decay=0.05, layer_decay=0.5, depth=12)
    got = {n: table[gi] for n, gi in zip(names, index)}
    for i in range(12):
        mine = [n for n in names if n.startswith(f"blocks.{i}.")]
        assert mine and all(got[n][0] == 0.5 ** (12 - i) for n in mine), i
    assert got["blocks.0.attn.qkv.weight"] == (0.5 ** 12, 0.05) and got["blocks.11.mlp.fc2.bias"] == (0.5 ** 1, 0.0)
    for n in ("cls_token", "pos_embed", "mask_token", "patch_embed.proj.weight", "patch_embed.proj.bias"):
        assert got[n][0] == 0.5 ** 13, n
    assert got["cls_token"][1] == 0.0 and got["patch_embed.proj.weight"][1] == 0.05
    assert got["norm.weight"] == (1.0, 0.0) and got["norm.bias"] == (1.0, 0.0)
    with pytest.raises(ValueError):
        optim.param_groups_for(names, shapes, weight_decay=0.05, layer_decay=0.5)          # depth missing
    with pytest.raises(ValueError):
        optim.param_groups_for(names, shapes, weight_decay=0.05, layer_decay=0.5, depth=6)   # blocks.6 .. outside


def test_more_than_256_groups_raise():
    names = [f"blocks.{i}.attn.qkv.weight" for i in range(300)]
    shapes = [(8, 8)] * 300
    index, table = optim.param_groups_for(names[:256], shapes[:256], weight_decay=0.1, layer_decay=0.99, depth=300)
    assert len(table) == 256 and index == list(range(256))
    with pytest.raises(ValueError, match="256"):
        optim.param_groups_for(names, shapes, weight_decay=0.1, layer_decay=0.99, depth=300)


# ---- quad codes and state on CPU buckets ------------------------------------------------------------------------------------------
class _Odd(nn.Module):
    """sizes that are no multiple of 4, so that the bucket holds padding"""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = nn.Parameter(torch.randn(3, 5, generator=g))       # 15 -> padded to 16
        self.b = nn.Parameter(torch.randn(5, generator=g))          # 5 -> 8
        self.cls_token = nn.Parameter(torch.randn(1, 1, 6, generator=g))   # 6 -> 8
        self.c = nn.Parameter(torch.randn(2, 2, generator=g))       # 4
        self.d = nn.Parameter(torch.randn(1, generator=g))          # 1 -> 4


def _cpu_opt(seed=0, **kw):
    m1, m2 = _Odd(seed), _Odd(seed + 1)
    b1 = optim.FlatBucket(list(m1.named_parameters()))
    b2 = optim.FlatBucket([("x." + n, p) for n, p in m2.named_parameters()][:3])
    return optim.AdamW([b1, b2], lr=1e-3, weight_decay=0.05, clip_grad=1.0, **kw), (b1, b2)


def test_quad_codes_follow_the_parameters_and_padding_is_zero():
    opt, (b1, b2) = _cpu_opt()
    for bi, b in enumerate((b1, b2)):
        codes = opt.codes[bi]
        table = opt.param_groups[bi]["group_table"]
        assert codes.dtype == torch.uint8 and codes.numel() * 4 == b.numel
        assert table[0] == (1.0, 0.05) and table[1] == (1.0, 0.0)    # order of first use: `a` decays, `b` does not
        index, _ = optim.param_groups_for(b.names, [tuple(p.shape) for p in b.params], weight_decay=0.05)
        covered = torch.zeros(codes.numel(), dtype=torch.bool)
        for off, p, gi in zip(b.offsets, b.params, index):
            q0, q1 = off // 4, (off + p.numel() + 3) // 4
            assert off % 4 == 0 and bool((codes[q0:q1] == gi).all()), b.names
            covered[q0:q1] = True
        assert bool(covered.all())                                   # this bucket has no quad of padding alone ...
    assert [int(c) for c in opt.codes[0]] == [0, 0, 0, 0, 1, 1, 1, 1, 0, 1]
    # ... a bucket longer than its parameters (not what FlatBucket builds, but what the rule says): the rest carries 0
    class _B:
        numel, offsets, params = 24, [8], [b1.params[1]]
    assert [int(c) for c in optim.quad_codes(_B, [1])] == [0, 0, 1, 1, 0, 0]


def test_state_dict_round_trip_and_foreign_states_are_refused():
    opt, (b1, b2) = _cpu_opt()
    g = torch.Generator().manual_seed(5)
    for b, v in zip((b1, b2), opt.exp_avg_sq):
        b.momentum.copy_(torch.randn(b.numel, generator=g))
        v.copy_(torch.rand(b.numel, generator=g))
    opt.guard[2] = 7
    opt.param_groups[0]["lr"] = 3e-4
    sd = opt.state_dict()
    assert sd["step"] == 7 and set(sd["state"][0]) == {"exp_avg", "exp_avg_sq"} and "params" not in sd["param_groups"][0]
    sd = torch.load(_roundtrip(sd), map_location="cpu")              # what a checkpoint does to it
    opt2, (c1, c2) = _cpu_opt(seed=10)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 7 and opt2.param_groups[0]["lr"] == 3e-4 and opt2.param_groups[1]["lr"] == 1e-3
    for b, c, v, w in zip((b1, b2), (c1, c2), opt.exp_avg_sq, opt2.exp_avg_sq):
        assert torch.equal(b.momentum, c.momentum) and torch.equal(v, w)
    assert opt2.skipped_steps == 0

    before = [t.clone() for t in (c1.momentum, c2.momentum, *opt2.exp_avg_sq, opt2.guard)]
    lr_before = [g_["lr"] for g_ in opt2.param_groups]

    def untouched():
        now = (c1.momentum, c2.momentum, *opt2.exp_avg_sq, opt2.guard)
        return all(torch.equal(a, b) for a, b in zip(before, now)) and [g_["lr"] for g_ in opt2.param_groups] == lr_before

    # an optim.SGD state over the same buckets
    d1, d2 = optim.FlatBucket(list(_Odd(3).named_parameters())), optim.FlatBucket(list(_Odd(4).named_parameters())[:3])
    with pytest.raises(ValueError):
        opt2.load_state_dict(optim.SGD([d1, d2], lr=0.5, momentum=0.9).state_dict())
    assert untouched()
    # a torch.optim.AdamW state: per-parameter tensors and steps
    mod = _Odd(6)
    topt = torch.optim.AdamW(mod.parameters(), lr=0.5)
    sum((p ** 2).sum() for p in mod.parameters()).backward()
    topt.step()
    with pytest.raises(ValueError):
        opt2.load_state_dict(topt.state_dict())
    assert untouched()
    # a state of this class over another trainable set (second bucket of another length)
    bad = opt.state_dict()
    bad["state"][1]["exp_avg_sq"] = torch.zeros(b2.numel + 4)
    with pytest.raises(ValueError):
        opt2.load_state_dict(bad)
    assert untouched()
    # SGD, in turn, refuses an AdamW state
    with pytest.raises(ValueError):
        optim.SGD([d1, d2], lr=0.5, momentum=0.9).load_state_dict(opt.state_dict())


def _roundtrip(obj):
    import io
    f = io.BytesIO()
    torch.save(obj, f)
    f.seek(0)
    return f


def test_constructor_checks():
    b = optim.FlatBucket(list(_Odd().named_parameters()))
    for kw in (dict(betas=(1.0, 0.999)), dict(eps=0.0), dict(clip_grad=0.0), dict(layer_decay=0.5)):
        with pytest.raises(ValueError):
            optim.AdamW([b], lr=1e-3, **kw)
    with pytest.raises(ValueError):
        optim.AdamW([optim.FlatBucket(list(_Odd().named_parameters()), momentum=False)], lr=1e-3)
    opt = optim.AdamW([b], lr=1e-3)
    assert opt.param_groups[0]["initial_lr"] == 1e-3 and opt.skipped_steps == 0 and opt.step_count == 0
    opt.zero_grad()
    with pytest.raises(_lib.AsisError):       # there is no CPU path
        opt.step()


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def test_parser_has_the_optimizer_flags_and_defaults_to_sgd():
    from adaptersis_amd import train_mla, train_multi_class
    for mod in (T, train_mla, train_multi_class):
        a = mod.get_args_parser().parse_args([])
        assert a.optimizer == "sgd" and a.weight_decay is None and a.clip_grad is None and a.layer_decay is None
        assert (a.adam_beta1, a.adam_beta2, a.adam_eps) == (0.9, 0.999, 1e-8)
        assert T._optimizer_args(a) == {"optimizer": "sgd", "clip_grad": None, "layer_decay": None}
        a = mod.get_args_parser().parse_args(["--optimizer", "adamw", "--weight_decay", "0.05", "--adam_beta1", "0.8", "--adam_beta2",
                                              "0.95", "--adam_eps", "1e-6", "--clip_grad", "1.0", "--layer_decay", "0.9",
                                              "--train_adapters"])
        assert a.weight_decay == 0.05 and a.train_adapters
        assert T._optimizer_args(a) == {"optimizer": "adamw", "betas": (0.8, 0.95), "eps": 1e-6, "clip_grad": 1.0, "layer_decay": 0.9}
    with pytest.raises(SystemExit):
        T.get_args_parser().parse_args(["--optimizer", "lion"])
