"""CPU: LoRA on the q / v projections (adaptersis_amd/lora.py) — the K-augmented packs against the formula in float64, the
attachment that leaves ``state_dict`` alone, the seeded init, the checkpoint entry, ``merged()``, every argument error, the host
checks of the two new ABI entries, and the GEMM forms of the augmented shapes."""
import ctypes as C

import pytest
import torch

from adaptersis_amd import _lib, lora, ops
from adaptersis_amd.dinov2.models import vision_transformer as vits
from adaptersis_amd.utils import weights as W

ARCH = "vit_tiny_test"


def _model():
    D, depth, heads, ffn = W.VIT_CONFIGS[ARCH]
    model = vits.__dict__[ARCH](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0)
    model.load_state_dict(W.make_vit_state_dict(ARCH, layerscale="kernel"))
    return model, D


def _rand(shape, seed, scale=1.0):
    g = torch.Generator()
    g.manual_seed(seed)
    return (torch.rand(shape, generator=g, dtype=torch.float64) * 2 - 1) * scale


# ---- packs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [4, 16, 32])
def test_packs_equal_the_lora_formula(r):
    D, R, s = 128, 37, 2.5
    Wq, A, Bq, Bv = _rand((3 * D, D), 1), _rand((2 * r, D), 2), _rand((D, r), 3), _rand((D, r), 4)
    xn, dqkv = _rand((R, D), 5), _rand((R, 3 * D), 6)
    # forward: [xn | u] Wf^T, u through the padded down matrix (pad columns exactly zero)
    u = xn @ lora.pack_wd_fwd(A).t()
    assert u.shape == (R, lora.PAD) and float(u[:, 2 * r:].abs().sum()) == 0.0
    wf = lora.pack_wf(Wq, Bq, Bv, s)
    assert wf.shape == (3 * D, D + lora.PAD)
    got = torch.cat([xn, u], 1) @ wf.t()
    want = xn @ Wq.t()
    want[:, :D] += s * (xn @ A[:r].t()) @ Bq.t()
    want[:, 2 * D:] += s * (xn @ A[r:].t()) @ Bv.t()
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # everything of Wf outside W and the two placed blocks is zero
    z = wf.clone()
    z[:, :D] = 0
    z[:D, D:D + r] = 0
    z[2 * D:, D + r:D + 2 * r] = 0
    assert float(z.abs().max()) == 0.0
    # backward: du through the block-diagonal down matrix, then [dqkv | du] WbT^T = dqkv W + du A
    du = torch.cat([dqkv[:, :D], dqkv[:, 2 * D:]], 1) @ lora.pack_wd_bwd(Bq, Bv, s).t()
    want_du = torch.cat([s * dqkv[:, :D] @ Bq, s * dqkv[:, 2 * D:] @ Bv], 1)
    assert float((du[:, :2 * r] - want_du).abs().max()) <= 1e-12 * float(want_du.abs().max())
    assert float(du[:, 2 * r:].abs().sum()) == 0.0
    wbt = lora.pack_wbt(Wq, A)
    assert wbt.shape == (D, 3 * D + lora.PAD)
    got = torch.cat([dqkv, du], 1) @ wbt.t()
    want = dqkv @ Wq + want_du @ A
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # merged weight
    m = lora.merged_weight(Wq, A, Bq, Bv, s)
    want = Wq.clone()
    want[:D] += s * Bq @ A[:r]
    want[2 * D:] += s * Bv @ A[r:]
    assert float((m - want).abs().max()) <= 1e-14 * float(want.abs().max())
    assert torch.equal(m[D:2 * D], Wq[D:2 * D])              # the k rows are the base weight's


# ---- attachment, init, checkpoint ----------------------------------------------------------------------------------------------
def test_attach_leaves_the_state_dict_alone():
    model, D = _model()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    names = [n for n, _ in model.named_parameters()]
    assert model.blocks[0].attn._lora is None
    lo = lora.LoRA(model, 4)
    after = model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert [n for n, _ in model.named_parameters()] == names
    assert not any("lora" in n for n, _ in model.named_modules())
    h = model.blocks[1].attn._lora
    assert h is lo.handles[1] and h.rank == 4 and h.A.shape == (8, D) and h.Bq.shape == (D, 4) and h.Bv.shape == (D, 4)
    keys = [n for n, _ in lo.named_parameters()]
    assert keys[:3] == ["blocks.0.attn.qkv.lora_A", "blocks.0.attn.qkv.lora_B_q", "blocks.0.attn.qkv.lora_B_v"]
    assert len(keys) == 3 * len(model.blocks)
    lora.LoRA.detach(model)
    assert model.blocks[1].attn._lora is None


def test_init_is_deterministic_and_b_is_zero():
    (m1, D), (m2, _) = _model(), _model()
    a, b, c = lora.LoRA(m1, 8, seed=3), lora.LoRA(m2, 8, seed=3), lora.LoRA(_model()[0], 8, seed=4)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        assert torch.equal(p, q), n
        if "lora_B" in n:
            assert float(p.detach().abs().max()) == 0.0
        else:
            assert 0.0 < float(p.detach().abs().max()) <= D ** -0.5      # kaiming-uniform(a = sqrt(5)): +-1/sqrt(fan_in)
    assert not torch.equal(a.handles[0].A, c.handles[0].A)
    assert not torch.equal(a.handles[0].A, a.handles[1].A)
    assert a.scale == 1.0 and lora.LoRA(_model()[0], 8, alpha=4.0).scale == 0.5


def test_checkpoint_round_trip(tmp_path):
    model, D = _model()
    lo = lora.LoRA(model, 4, alpha=8.0)
    with torch.no_grad():
        for i, p in enumerate(lo.parameters()):
            p.copy_(_rand(p.shape, 100 + i).float())
    path = tmp_path / "lora.pt"
    torch.save({"lora": lo.state_dict()}, path)
    entry = torch.load(path, map_location="cpu")["lora"]
    assert entry["rank"] == 4 and entry["alpha"] == 8.0 and set(entry["params"]) == {n for n, _ in lo.named_parameters()}
    m2, _ = _model()
    lo2 = lora.LoRA.from_state(m2, entry)
    assert lo2.rank == 4 and lo2.alpha == 8.0 and m2.blocks[0].attn._lora is lo2.handles[0]
    for (n, p), (_, q) in zip(lo.named_parameters(), lo2.named_parameters()):
        assert torch.equal(p, q), n
    # a resume goes through restart_from_checkpoint like every other entry of the file
    from adaptersis_amd.utils import misc as utils
    lo3 = lora.LoRA(_model()[0], 4, alpha=8.0)
    utils.restart_from_checkpoint(str(path), lora=lo3)
    for (n, p), (_, q) in zip(lo.named_parameters(), lo3.named_parameters()):
        assert torch.equal(p, q), n
    with pytest.raises(ValueError, match="rank"):
        lora.LoRA(_model()[0], 8).load_state_dict(entry)
    bad = {**entry, "params": {k: v for k, v in list(entry["params"].items())[1:]}}
    with pytest.raises(ValueError, match="names"):
        lora.LoRA(_model()[0], 4, alpha=8.0).load_state_dict(bad)
    bad = {**entry, "params": {k: (v[:1] if k.endswith("0.attn.qkv.lora_A") else v) for k, v in entry["params"].items()}}
    with pytest.raises(ValueError, match="shape"):
        lora.LoRA(_model()[0], 4, alpha=8.0).load_state_dict(bad)


def test_merged_swaps_restores_and_bumps_the_generation():
    model, D = _model()
    lo = lora.LoRA(model, 4, alpha=8.0)
    with torch.no_grad():
        for i, p in enumerate(lo.parameters()):
            p.copy_(_rand(p.shape, 200 + i, 0.1).float())
    w = model.blocks[2].attn.qkv.weight
    h = lo.handles[2]
    base, base_ptr, cache = w.detach().clone(), w.data_ptr(), model.blocks[2].attn._cache
    gen0 = getattr(w, "_asis_gen", 0)
    with lo.merged(model) as m:
        assert m is model and w.data_ptr() != base_ptr and model.blocks[2].attn._lora is None
        assert model.blocks[2].attn._cache is not cache
        want = lora.merged_weight(base.double(), h.A.detach().double(), h.Bq.detach().double(), h.Bv.detach().double(), 2.0)
        assert float((w.detach().double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
        assert not torch.equal(w.detach(), base)
        assert list(model.state_dict()) == list(_model()[0].state_dict())
        merged_ptr = w.data_ptr()
    assert w.data_ptr() == base_ptr and torch.equal(w.detach(), base)          # bit for bit
    assert model.blocks[2].attn._lora is h and model.blocks[2].attn._cache is cache
    gen1 = getattr(w, "_asis_gen", 0)
    assert gen1 == gen0 + 1
    with lo.merged(model):                                                     # nothing changed: no re-merge, the same tensor
        assert w.data_ptr() == merged_ptr
    assert getattr(w, "_asis_gen", 0) == gen1
    with torch.no_grad():
        h.Bq.add_(0.5)                                                         # B changed: re-merged in place, generation bumped
    with lo.merged(model):
        assert w.data_ptr() == merged_ptr
        want = lora.merged_weight(base.double(), h.A.detach().double(), h.Bq.detach().double(), h.Bv.detach().double(), 2.0)
        assert float((w.detach().double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
    assert getattr(w, "_asis_gen", 0) == gen1 + 1 and torch.equal(w.detach(), base)
    h.A._asis_gen = getattr(h.A, "_asis_gen", 0) + 1                           # a fused optimizer step marks a change like this
    with lo.merged(model):
        pass
    assert getattr(w, "_asis_gen", 0) == gen1 + 2
    with pytest.raises(RuntimeError, match="boom"):                            # restored on an exception too
        with lo.merged(model):
            raise RuntimeError("boom")
    assert w.data_ptr() == base_ptr and model.blocks[2].attn._lora is h


# ---- argument errors -----------------------------------------------------------------------------------------------------------
def _engine(**kw):
    from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
    from adaptersis_amd.backbones.decoders import DecoderMLA, FeatureDecoder
    from adaptersis_amd.backbones.encoders import FeatureEncoder
    from adaptersis_amd.backbones.engines import SegEngine
    mla = kw.pop("mla", False)
    model_kw = kw.pop("model_kw", {})
    D, depth, heads, ffn = W.VIT_CONFIGS[ARCH]
    model = vits.__dict__[ARCH](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0, **model_kw)
    enc = FeatureEncoder(embed_dim=D)
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4)
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25)
    dec = DecoderMLA(img_size=224, mla_channels=D, num_classes=2) if mla else \
        FeatureDecoder(embed_dim=D, num_classes=2, features=[D, 32, 16, 16, 8])
    kw.setdefault("mode", "train_adapters")
    kw.setdefault("train_backbone", not mla)
    return SegEngine(model, enc, cv, cn, dec, **kw)


def test_engine_argument_errors():
    from adaptersis_amd.backbones.decoders import DecoderSETR
    from adaptersis_amd.backbones.engines import EndToEndEngine
    for rank in (0, 3, 5, 64, -4):
        with pytest.raises(ValueError, match="lora_rank must be one of"):
            _engine(lora_rank=rank)
        with pytest.raises(ValueError, match="rank must be one of"):
            lora.LoRA(_model()[0], rank)
    with pytest.raises(ValueError, match="optimize_backbone"):
        _engine(lora_rank=4, optimize_backbone=True)
    with pytest.raises(ValueError, match="layer_decay"):
        _engine(lora_rank=4, layer_decay=0.9, optimizer="adamw")
    with pytest.raises(ValueError, match="drop_path_rate"):
        _engine(lora_rank=4, model_kw=dict(drop_path_rate=0.2))
    with pytest.raises(ValueError, match="train_mla"):
        _engine(lora_rank=4, mla=True)
    with pytest.raises(ValueError, match="train_backbone"):
        _engine(lora_rank=4, train_backbone=False)
    with pytest.raises(ValueError, match="train_adapters"):
        _engine(lora_rank=4, mode="reference_exact", train_backbone=False)
    with pytest.raises(ValueError, match="lora_alpha needs lora_rank"):
        _engine(lora_alpha=8.0)
    with pytest.raises(ValueError, match="alpha must be positive"):
        _engine(lora_rank=4, lora_alpha=0.0)
    D = W.VIT_CONFIGS[ARCH][0]
    with pytest.raises(ValueError, match="LoRA"):
        EndToEndEngine(_model()[0], DecoderSETR(D, 2, features=[32, 16, 16, 8]), lora_rank=4)


def test_engine_with_lora_freezes_the_backbone_and_builds_no_vit_bucket():
    eng = _engine(lora_rank=4, lora_alpha=8.0)
    assert eng.vit_bucket is None and eng.lora is not None and eng.lora.scale == 2.0
    assert all(not p.requires_grad for p in eng.model.parameters())
    assert eng.lora_bucket.names == [n for n, _ in eng.lora.named_parameters()]
    assert eng.lora_bucket in eng.optimizer.buckets
    assert all(p.data_ptr() == v.data_ptr() for p, v in zip(eng.lora.parameters(), eng.lora_bucket.params))
    assert eng.model.blocks[0].attn._lora is eng.lora.handles[0]
    assert not any("lora" in k for k in eng.model.state_dict())


def test_script_argument_errors():
    import argparse
    from adaptersis_amd import train as T
    from adaptersis_amd import train_mla, train_multi_class
    full = ["--train_adapters", "--train_backbone"]
    for mod in (T, train_mla, train_multi_class):
        a = mod.get_args_parser().parse_args(full + ["--lora_rank", "8", "--lora_alpha", "16"])
        assert a.lora_rank == 8 and a.lora_alpha == 16.0
        assert mod.get_args_parser().parse_args([]).lora_rank is None
        for argv in (full + ["--lora_rank", "5"], ["--lora_rank", "4"], ["--lora_alpha", "4"]):   # a usage error like any other
            with pytest.raises(SystemExit):
                mod.get_args_parser().parse_args(argv)
    ns = lambda **kw: argparse.Namespace(**kw)
    assert "--lora_rank needs" in T.check_backbone_args(ns(lora_rank=4))
    assert "--lora_rank needs" in T.check_backbone_args(ns(lora_rank=4, train_adapters=True))
    assert "--optimize_backbone" in T.check_backbone_args(ns(lora_rank=4, train_adapters=True, train_backbone=True, optimize_backbone=True))
    assert "--drop_path 0" in T.check_backbone_args(ns(lora_rank=4, train_adapters=True, train_backbone=True, drop_path=0.2))
    assert "--lora_alpha needs" in T.check_backbone_args(ns(lora_alpha=4.0))
    ok = T.get_args_parser().parse_args(full + ["--lora_rank", "4"])
    assert T.check_backbone_args(ok) is None
    assert T._backbone_args(ok) == {"train_backbone": True, "lora_rank": 4, "lora_alpha": None}
    assert T._backbone_args(T.get_args_parser().parse_args([])) == {}


def test_block_refuses_lora_with_stochastic_depth():
    model, D = _model()
    lora.LoRA(model, 4)
    x = torch.zeros((2 * 5, D))
    with pytest.raises(ValueError, match="stochastic depth"):
        model.blocks[0].forward_train_rows(x, [(2, 5)], keep=([([0], 2.0)], None))


# ---- the ABI's host checks (nothing is launched) ----------------------------------------------------------------------------------
_keep = []


def buf(nbytes=1 << 16):
    raw = C.create_string_buffer(nbytes + 16)
    _keep.append(raw)
    return (C.addressof(raw) + 15) & ~15


def test_abi_rejects_bad_operands():
    lib = _lib.lib()
    x, wd, u, sl = buf(), buf(), buf(), buf()

    def down(**kw):
        a = dict(dtype=0, x=x, ldx=128, c0a=0, lena=64, c0b=0, lenb=0, wd=wd, u=u, ldu=64, R=4)
        a.update(kw)
        return lib.asis_lora_down(None, a["dtype"], a["x"], a["ldx"], a["c0a"], a["lena"], a["c0b"], a["lenb"], a["wd"], a["u"],
                                  a["ldu"], a["R"])

    def wgrad(**kw):
        a = dict(dtype=0, u=u, ldu=64, x=x, ldx=128, c0a=0, lena=64, c0b=0, lenb=0, slabs=sl, nblk=1, R=4)
        a.update(kw)
        return lib.asis_lora_wgrad(None, a["dtype"], a["u"], a["ldu"], a["x"], a["ldx"], a["c0a"], a["lena"], a["c0b"], a["lenb"],
                                   a["slabs"], a["nblk"], a["R"])
    bad = [(dict(x=None), b"null"), (dict(u=None), b"null"), (dict(x=x + 8), b"aligned"), (dict(u=u + 2), b"aligned"),
           (dict(lena=96), b"multiples of 64"), (dict(lena=0), b"multiples of 64"), (dict(lenb=32, c0b=64), b"multiples of 64"),
           (dict(ldx=56), b"ldx"), (dict(ldx=127), b"ldx"), (dict(c0a=64, lena=128), b"ldx"), (dict(c0a=4), b"segment columns"),
           (dict(c0b=32, lenb=64), b"segment columns"), (dict(ldu=32), b"ldu"), (dict(ldu=68), b"ldu"), (dict(R=0), b"R="),
           (dict(dtype=7), b"bad dtype 7")]
    for fn, name in ((down, b"asis_lora_down"), (wgrad, b"asis_lora_wgrad")):
        for kw, word in bad:
            assert fn(**kw) == _lib.ASIS_EINVAL, (name, kw)
            msg = lib.asis_last_error()
            assert name in msg and word in msg, (kw, msg)
    for kw, word in [(dict(wd=None), b"wd"), (dict(wd=wd + 4), b"wd")]:
        assert down(**kw) == _lib.ASIS_EINVAL and word in lib.asis_last_error(), kw
    for kw, word in [(dict(slabs=None), b"slabs"), (dict(slabs=sl + 4), b"slabs"), (dict(nblk=2), b"nblk"), (dict(nblk=0), b"nblk")]:
        assert wgrad(**kw) == _lib.ASIS_EINVAL and word in lib.asis_last_error(), kw


def test_wgrad_nblk_query():
    lib = _lib.lib()
    assert lib.asis_lora_wgrad_nblk(0, 64) == 0 and lib.asis_lora_wgrad_nblk(10, 32) == 0
    assert lib.asis_lora_wgrad_nblk(1, 64) == 1 and lib.asis_lora_wgrad_nblk(255, 384) == 1
    for R, Nt in [(33, 64), (1000, 128), (4099, 384), (42348, 1024), (42348, 2048)]:
        n = lib.asis_lora_wgrad_nblk(R, Nt)
        tiles = (Nt + 127) // 128
        assert 1 <= n and n * tiles <= 512, (R, Nt, n)
        rows_per = -(-R // n)
        assert (n - 1) * (-(-rows_per // 64) * 64) < R, (R, Nt, n)       # every block holds at least one row
    assert lib.asis_lora_wgrad_nblk(4099, 384) > 1 and lib.asis_lora_wgrad_nblk(42348, 1024) > 8


def test_ops_check_before_the_call():
    x = torch.zeros((8, 128), dtype=torch.float16)
    with pytest.raises(_lib.AsisError, match="no CPU fallback"):
        ops.lora_down(x, [(0, 64)], torch.zeros((64, 64), dtype=torch.float16))
    with pytest.raises(_lib.AsisError, match="no CPU fallback"):
        ops.lora_wgrad(torch.zeros((8, 64), dtype=torch.float16), x, [(0, 64)])


# ---- the augmented GEMMs keep their form ---------------------------------------------------------------------------------------
def test_augmented_k_keeps_the_gemm_form():
    R, D = 42348, 1024
    fwd, fwd_aug = ops._shape_plan(R, 3 * D, D), ops._shape_plan(R, 3 * D, D + 64)
    bwd, bwd_aug = ops._shape_plan(R, D, 3 * D, out_f32=True), ops._shape_plan(R, D, 3 * D + 64, out_f32=True)
    print("qkv GEMM K 1024 -> 1088:", fwd, "->", fwd_aug, "; input-gradient GEMM K 3072 -> 3136:", bwd, "->", bwd_aug)
    assert fwd is not None and fwd_aug == fwd
    assert bwd is not None and bwd_aug == bwd
