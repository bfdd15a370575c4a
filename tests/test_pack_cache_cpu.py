"""CPU: the one cache of derived operands (adaptersis_amd/packs.py) and what dinov2/layers/blocks.py builds on it — when a pack is
rebuilt, which key it lives under, and which packs ``Block._ls_pow2`` evicts.  Every ``fn`` here counts its calls and returns CPU
tensors; the device kernels behind the real packs are replaced by counting stand-ins."""
import pytest
import torch

from adaptersis_amd import config, lora, ops, packs
from adaptersis_amd.dinov2.layers import blocks as B


class Counter:
    def __init__(self):
        self.n = 0

    def __call__(self, *a):
        self.n += 1
        return torch.full((1,), float(self.n))


def _other_dtype():
    return torch.bfloat16 if config.operand_dtype == torch.float16 else torch.float16


def test_derived_builds_once_and_skips_none_sources():
    p, q = torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(3))
    cache, fn = {}, Counter()
    first = packs.derived(cache, "k", (p, None, q), fn)
    for _ in range(3):
        assert packs.derived(cache, "k", (p, None, q), fn) is first
    assert fn.n == 1
    assert packs.derived(cache, "k", (None, p, q, None), fn) is first and fn.n == 1        # None entries are not part of the tag
    assert packs.tag_of((p, None, q)) == packs.tag_of((p, q)) == cache["k"][0]
    assert packs.derived(cache, "k", (p,), fn) is not first and fn.n == 2                  # another set of sources
    made = []
    packs.derived({}, "g", (p,), lambda: made.append(torch.is_grad_enabled()))
    assert made == [False]                                                                # fn runs under no_grad


@pytest.mark.parametrize("second", [False, True], ids=["single", "second-of-two"])
def test_derived_rebuilds_after_every_kind_of_change(second):
    a, p = torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(4))
    srcs = (a, p) if second else (p,)
    cache, fn = {}, Counter()
    call = lambda extra=(): packs.derived(cache, "k", srcs, fn, extra)

    def rebuilt():
        n = fn.n
        call(); call()
        return fn.n - n

    assert rebuilt() == 1
    with torch.no_grad():
        p.mul_(2.0)                                                     # an in-place write through torch: _version
    assert rebuilt() == 1
    v = p._version
    p.data.fill_(3.0)                                                   # what a fused optimizer does: _version stays ...
    assert p._version == v and rebuilt() == 0
    p._asis_gen = getattr(p, "_asis_gen", 0) + 1                        # ... and the change is marked by _asis_gen alone
    assert p._version == v and rebuilt() == 1
    ptr = p.data_ptr()
    p.data = p.data.clone()                                             # a new data_ptr
    assert p.data_ptr() != ptr and rebuilt() == 1
    dt = config.operand_dtype
    try:
        config.set_operand_dtype(_other_dtype())
        assert rebuilt() == 1
    finally:
        config.set_operand_dtype(dt)
    assert rebuilt() == 1                                               # and back
    n = fn.n
    call(extra=(0.5,)); call(extra=(0.5,))
    assert fn.n == n + 1
    call(extra=(0.25,))
    assert fn.n == n + 2


def test_pack_and_lora_tag_use_the_same_builder():
    p, q = torch.nn.Parameter(torch.ones(4, 2)), torch.nn.Parameter(torch.ones(2))
    cache, seen = {}, []

    def fn(t):
        seen.append(t)
        return t * 2
    out = B._pack(cache, "k", p, fn)
    assert B._pack(cache, "k", p, fn) is out and len(seen) == 1
    assert not seen[0].requires_grad and seen[0].data_ptr() == p.data_ptr()       # fn gets param.detach()
    assert cache["k"][0] == packs.tag_of((p,)) == lora._tag(p)
    assert lora._tag(p, q) == packs.tag_of((p, q))
    assert B.derived is packs.derived                                              # blocks.py re-exports the primitive
    p._asis_gen = 5
    assert lora._tag(p) == packs.tag_of((p,)) != cache["k"][0]


def test_ls_pow2_evicts_exactly_the_retired_k():
    """retiring ls1's k = 7 deletes the ``@7`` / ``@-7`` packs and leaves the other LayerScale's ``@17`` / ``@-17`` alone"""
    blk = B.Block(64, 1, qkv_bias=True, init_values=1e-5)
    g1, g2 = blk.ls1.gamma, blk.ls2.gamma
    with torch.no_grad():
        g1.fill_(0.01)                                                  # 0.01 * 2^7 = 1.28
    assert blk._ls_pow2("ls1.k", g1) == 7 and blk._ls_pow2("ls2.k", g2) == 17
    for key in ("projT@7", "n1w@-7", "fc2T@17", "n2w@-17", "qkvT"):
        blk._cache[key] = ("x", None)
    with torch.no_grad():
        g1.fill_(0.5)
    assert blk._ls_pow2("ls1.k", g1) == 1
    assert "projT@7" not in blk._cache and "n1w@-7" not in blk._cache
    assert all(key in blk._cache for key in ("fc2T@17", "n2w@-17", "qkvT"))
    assert blk._ls_pow2("ls2.k", g2) == 17


def test_ln_split_amax_follows_the_bias(monkeypatch):
    """the MX amax bound sqrt(D - 1) max|w| + max|b| is rebuilt when norm.bias alone changes"""
    blk = B.Block(64, 1, qkv_bias=True, init_values=1e-5)
    monkeypatch.setattr(ops, "layernorm_mx", lambda x, w, b, eps, dt, amax: (x, x))
    x = torch.zeros(4, 64)
    amax0 = blk._ln_split("n1", blk.norm1, x, True)[2][1]
    assert float(amax0) == pytest.approx(63 ** 0.5)
    assert blk._ln_split("n1", blk.norm1, x, True)[2][1] is amax0
    assert blk._cache["n1.amax"][0] == packs.tag_of((blk.norm1.weight, blk.norm1.bias))
    with torch.no_grad():
        blk.norm1.bias.fill_(2.0)
    amax1 = blk._ln_split("n1", blk.norm1, x, True)[2][1]
    assert amax1 is not amax0 and float(amax1) == pytest.approx(63 ** 0.5 + 2.0)


def test_w16_has_one_key_per_key_rows_part(monkeypatch):
    calls = []

    def cast_pad(x, ld=None, dtype=None, part=0):
        calls.append(part)
        return x.clone()
    monkeypatch.setattr(ops, "cast_pad", cast_pad)
    monkeypatch.setattr(config, "precise_attention", True)
    m = B.Mlp(8, 16)
    w = m.fc1.weight
    rows = torch.arange(15, -1, -1)
    got = {(r is not None, part): m._w16("fc1", w, r, part) for r in (None, rows) for part in (0, 1)}
    assert sorted(m._cache) == ["fc1", "fc1.lo", "fc1.sg", "fc1.sg.lo"] and calls == [0, 1, 0, 1]
    assert torch.equal(got[(True, 0)], w.detach()[rows]) and torch.equal(got[(False, 1)], w.detach())
    for (has_rows, part), t in got.items():
        assert m._w16("fc1", w, rows if has_rows else None, part) is t
    assert len(calls) == 4
    # the precise_attention-gated residual is the same pack, not a second copy of the same bytes
    assert m._w16lo("fc1", w) is m._w16("fc1", w, part=1) and len(calls) == 4
    monkeypatch.setattr(config, "precise_attention", False)
    assert m._w16lo("fc1", w) is None
