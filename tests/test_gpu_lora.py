"""GPU: LoRA on the q / v projections — the two kernels of csrc/lora.hip against float64 of the 16-bit-rounded operands (bound
scheme of tests/bound_helpers.py), ``Block.forward_train_rows`` / ``backward`` with a handle against float64 autograd of the
restated math (tests/lora_ref.py), the merged-weight eval path, a tiny ``SegEngine(lora_rank=4)`` and the ``lora`` checkpoint entry
through the training script and ``adaptersis_amd.predict``."""
import os

import pytest
import torch

from adaptersis_amd import config, lora, ops
from adaptersis_amd.dinov2.models import vision_transformer as vits
from adaptersis_amd.utils import weights as W
from tests import lora_ref as R
from tests.bound_helpers import DT, HALF, SUBN, U_SUM, _bound, _err, _gen
from tests.conftest import rel_l2

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _u(shape, *key):
    return torch.rand(shape, generator=_gen(*key), dtype=torch.float32) * 2 - 1


# ---- kernels -----------------------------------------------------------------------------------------------------------------
# (segments, columns of the X buffer): one segment behind 8 sentinel columns; two segments around a skipped middle
DOWN_LAYOUTS = [([(8, 64)], 96), ([(8, 384)], 408), ([(0, 64), (136, 64)], 200), ([(8, 128), (208, 256)], 488)]


def _x_buffer(Rn, rows_buf, segs, ldx, dt, *key):
    """16-bit [rows_buf, ldx] buffer, NaN everywhere but the segments' first ``Rn`` rows -> (buffer, float64 [Rn, Kt] of them)"""
    xb = torch.full((rows_buf, ldx), NAN, dtype=dt)
    parts = []
    for i, (c0, n) in enumerate(segs):
        xb[:Rn, c0:c0 + n] = _u((Rn, n), *key, i).to(dt)
        parts.append(xb[:Rn, c0:c0 + n].double())
    return xb, torch.cat(parts, 1)


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("Rn", [1, 15, 17, 257])
def test_lora_down(dev, Rn, dt):
    for li, (segs, ldx) in enumerate(DOWN_LAYOUTS):
        for r in (4, 16):
            Kt = sum(n for _, n in segs)
            xb, x64 = _x_buffer(Rn, Rn + 3, segs, ldx, dt, 1, Rn, li)
            wd = torch.zeros((64, Kt), dtype=dt)
            wd[:2 * r] = (_u((2 * r, Kt), 2, Rn, li, r) * 0.25).to(dt)
            ub = torch.full((Rn + 2, 88), 7.0, dtype=dt)                     # U = columns 8..72 of a wider, taller buffer
            ubd = ub.to(dev)
            out = ops.lora_down(xb.to(dev)[:Rn], segs, wd.to(dev), out=ubd[:Rn, 8:72])
            assert out.data_ptr() == ubd[:Rn, 8:72].data_ptr()
            got = ubd.cpu()
            assert bool((got[:, :8] == 7.0).all()) and bool((got[:, 72:] == 7.0).all()) and bool((got[Rn:] == 7.0).all())
            u = got[:Rn, 8:72]
            assert bool((u[:, 2 * r:] == 0).all())                           # the pad columns: exact zeros
            ref = x64 @ wd.double().t()
            f32 = xb[:Rn].float()
            f32 = torch.cat([f32[:, c0:c0 + n] for c0, n in segs], 1) @ wd.float().t()
            b32, yard = _bound(f32, ref, U_SUM)
            lim = HALF[dt] * ref.abs() + SUBN[dt] + b32
            err = (u.double() - ref).abs()
            print(f"lora_down R={Rn} segs={segs} r={r} {dt}: max err/limit {float((err / lim).max()):.3f} (fp32 yard {yard:.2e})")
            assert bool((err <= lim).all())


@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("Rn", [1, 33, 1000, 4099])
def test_lora_wgrad(dev, Rn, dt):
    for li, (segs, ldx) in enumerate([([(8, 64)], 96), ([(0, 192)], 192), ([(8, 128), (208, 256)], 488)]):
        Nt = sum(n for _, n in segs)
        xb, x64 = _x_buffer(Rn, Rn + 5, segs, ldx, dt, 3, Rn, li)
        ub = torch.full((Rn + 5, 88), NAN, dtype=dt)                          # NaN behind the rows and beside the 64 columns
        ub[:Rn, 8:72] = _u((Rn, 64), 4, Rn, li).to(dt)
        scale = 0.5
        xd, ud = xb.to(dev), ub.to(dev)
        got = ops.lora_wgrad(ud[:, 8:72], xd[:Rn], segs, scale)
        assert got.shape == (64, Nt) and got.dtype == torch.float32
        nblk = ops.lora_wgrad_nblk(Rn, Nt)
        assert (nblk > 1) == (Rn >= 1000)                                     # several slabs, the last one ragged (4099 = 16 * 256 + 3)
        ref = scale * (ub[:Rn, 8:72].double().t() @ x64)
        f32 = scale * (ub[:Rn, 8:72].float().t() @ x64.float())
        bound, yard = _bound(f32, ref, U_SUM)
        e = _err(got, ref)
        print(f"lora_wgrad R={Rn} segs={segs} {dt} nblk={nblk}: err {e:.3e} bound {bound:.3e} (fp32 yard {yard:.2e})")
        assert e <= bound
        again = ops.lora_wgrad(ud[:, 8:72], xd[:Rn], segs, scale)
        assert torch.equal(got, again)                                        # fixed summation order


def test_ops_argument_checks(dev):
    x = torch.zeros((8, 128), device=dev, dtype=torch.float16)
    wd = torch.zeros((64, 64), device=dev, dtype=torch.float16)
    u = torch.zeros((8, 64), device=dev, dtype=torch.float16)
    for segs in ([(0, 96)], [(4, 64)], [(0, 64), (32, 64)], [(64, 128)], [], [(0, 64)] * 3):
        with pytest.raises(ValueError):
            ops.lora_down(x, segs, wd, out=u)
        with pytest.raises(ValueError):
            ops.lora_wgrad(u, x, segs)
    with pytest.raises(ValueError, match="wd"):
        ops.lora_down(x, [(0, 64)], wd[:, :32].contiguous(), out=u)
    with pytest.raises(ValueError, match="u must be"):
        ops.lora_down(x, [(0, 64)], wd, out=u[:4])
    with pytest.raises(ValueError):
        ops.lora_wgrad(u.float(), x, [(0, 64)])
    with pytest.raises(ValueError, match="aligned"):
        ops.lora_down(x[:, 4:], [(0, 64)], wd, out=u)


# ---- block -------------------------------------------------------------------------------------------------------------------
ARCH, SEGS, RANK, ALPHA = "vit_tiny_test", [(2, 17), (2, 16)], 4, 8.0


def _model(dev):
    D, depth, heads, ffn = W.VIT_CONFIGS[ARCH]
    sd = W.make_vit_state_dict(ARCH, layerscale="kernel")
    model = vits.__dict__[ARCH](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0)
    model.load_state_dict(sd)
    return model.to(dev), sd, D, heads


def _lora_model(dev):
    model, sd, D, heads = _model(dev)
    lo = lora.LoRA(model, RANK, ALPHA)
    with torch.no_grad():          # B random and non-zero: with B = 0 the gradient of A is vacuous
        for i, h in enumerate(lo.handles):
            h.Bq.copy_(W.tensor(f"lora.bq.{i}", tuple(h.Bq.shape), 0.05))
            h.Bv.copy_(W.tensor(f"lora.bv.{i}", tuple(h.Bv.shape), 0.05))
    return model, lo, sd, D, heads


def _inputs(D):
    rows = sum(b * n for b, n in SEGS)
    return W.tensor("lora.x", (rows, D), 1.0), W.tensor("lora.dy", (rows, D), 1.0)


def _run(blk, x2, dy2, dt, dev, grads):
    old = config.operand_dtype
    config.set_operand_dtype(dt)
    try:
        y, saved = blk.forward_train_rows(x2.to(dev), SEGS)
        S = 1024.0
        dx = blk.backward(saved, (dy2 * S).to(dev).contiguous(), 1.0 / S, grads, "blocks.1")
    finally:
        config.set_operand_dtype(old)
    return y, dx / S


@pytest.fixture(scope="module")
def block_ref():
    """float64 autograd of the block with LoRA, computed once"""
    sd = W.make_vit_state_dict(ARCH, layerscale="kernel")
    D, _, heads, _ = W.VIT_CONFIGS[ARCH]
    model, lo, _, _, _ = _lora_model(torch.device("cpu"))
    h = lo.handles[1]
    x2, dy2 = _inputs(D)
    return R.run(sd, "blocks.1", x2, dy2, SEGS, heads, h.A.detach(), h.Bq.detach(), h.Bv.detach(), lo.scale)


@pytest.mark.parametrize("dt", DT)
def test_block_with_lora_against_float64(dev, dt, block_ref):
    model, lo, sd, D, heads = _lora_model(dev)
    blk, h = model.blocks[1], lo.handles[1]
    x2, dy2 = _inputs(D)
    names = ["blocks.1.attn.qkv.lora_A", "blocks.1.attn.qkv.lora_B_q", "blocks.1.attn.qkv.lora_B_v"]
    grads = {n: torch.full_like(p, 7.0) for n, p in zip(names, h.params)}
    y, dx = _run(blk, x2, dy2, dt, dev, grads)
    y_ref, dx_ref, dA, dBq, dBv = block_ref
    f16 = dt == torch.float16
    errs = {n.rsplit(".", 1)[1]: rel_l2(grads[n], g) for n, g in zip(names, (dA, dBq, dBv))}
    e_y, e_dx = rel_l2(y, y_ref), rel_l2(dx, dx_ref)
    print(dt, "LoRA block: y %.2e dx %.2e" % (e_y, e_dx), {k: "%.1e" % v for k, v in errs.items()})
    assert float(dA.norm()) > 0 and float(dBq.norm()) > 0 and float(dBv.norm()) > 0
    assert e_y < (5e-4 if f16 else 4e-3)
    tol = 3e-3 if f16 else 2.5e-2
    assert e_dx < tol and max(errs.values()) < tol, errs
    # the LoRA terms are in the output at all: the base block differs by far more than the bar
    base, _, _, _ = _model(dev)
    y0, _ = _run(base.blocks[1], x2, dy2, dt, dev, None)
    assert rel_l2(y0, y_ref) > 4 * (5e-4 if f16 else 4e-3)
    # input gradient alone: the same dx, no parameter work
    _, dx_only = _run(blk, x2, dy2, dt, dev, None)
    assert torch.equal(dx_only, dx)
    # the frozen forward under merged() against the LoRA training forward: training form vs eval kernels (test_gpu_vit_bwd.py)
    old = config.operand_dtype
    config.set_operand_dtype(dt)
    try:
        with lo.merged(model):
            y_eval = blk.forward_rows(x2.to(dev), SEGS)
        y_base = blk.forward_rows(x2.to(dev), SEGS)
    finally:
        config.set_operand_dtype(old)
    e_eval = rel_l2(y, y_eval)
    print(dt, "training forward vs merged eval forward: %.2e (base eval forward: %.2e)" % (e_eval, rel_l2(y, y_base)))
    assert e_eval < (5e-4 if f16 else 4e-3)
    assert blk.attn._lora is h and rel_l2(y, y_base) > 4 * (5e-4 if f16 else 4e-3)


@pytest.mark.parametrize("dt", DT)
def test_block_without_a_handle_is_bit_identical(dev, dt):
    """a block that had a handle attached and taken off again against a block that never saw lora.py"""
    plain, _, D, _ = _model(dev)
    model, lo, _, _, _ = _lora_model(dev)
    lora.LoRA.detach(model)
    x2, dy2 = _inputs(D)
    y0, dx0 = _run(plain.blocks[1], x2, dy2, dt, dev, None)
    y1, dx1 = _run(model.blocks[1], x2, dy2, dt, dev, None)
    assert torch.equal(y0, y1) and torch.equal(dx0, dx1)
    g0 = {"blocks.1." + k: torch.zeros_like(p, dtype=torch.float32) for k, p in plain.blocks[1].named_parameters()}
    g1 = {k: torch.zeros_like(v) for k, v in g0.items()}
    _run(plain.blocks[1], x2, dy2, dt, dev, g0)
    _run(model.blocks[1], x2, dy2, dt, dev, g1)
    assert all(torch.equal(g0[k], g1[k]) for k in g0)


# ---- engine ------------------------------------------------------------------------------------------------------------------
def _seg_engine(dev, **kw):
    from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
    from adaptersis_amd.backbones.decoders import FeatureDecoder
    from adaptersis_amd.backbones.encoders import FeatureEncoder
    from adaptersis_amd.backbones.engines import SegEngine
    feats = (128, 32, 16, 16, 8)
    model, _, D, _ = _model(dev)
    enc = FeatureEncoder(embed_dim=D); enc.load_state_dict(W.make_encoder_state_dict(D))
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4); cv.load_state_dict(W.make_cavit_state_dict(D, mode="kernel"))
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25); cn.load_state_dict(W.make_cacnn_state_dict(D, mode="kernel"))
    dec = FeatureDecoder(embed_dim=D, num_classes=2, features=list(feats)); dec.load_state_dict(W.make_feature_decoder_state_dict(D, 2, features=feats))
    return SegEngine(model, enc.to(dev), cv.to(dev), cn.to(dev), dec.to(dev), lr=0.05, mode="train_adapters", train_encoder=True,
                     train_backbone=True, **kw)


@pytest.mark.parametrize("optimizer", ["sgd", "adamw"])
def test_seg_engine_two_steps_with_lora(dev, optimizer):
    eng = _seg_engine(dev, lora_rank=4, optimizer=optimizer)
    assert eng.vit_bucket is None and eng.lora_bucket is not None and eng.lora_bucket in eng.optimizer.buckets
    before = {k: v.detach().clone() for k, v in eng.model.state_dict().items()}
    A0 = [h.A.detach().clone() for h in eng.lora.handles]
    img, tgt = W.synthetic_batch(3, 224)
    img, tgt = img.to(dev), tgt.to(dev)
    l1 = float(eng.train_step(img, tgt))
    assert l1 == l1 and abs(l1) < float("inf") and eng.optimizer.skipped_steps == 0
    for i, h in enumerate(eng.lora.handles):
        assert float(h.A.grad.abs().max()) == 0.0, i            # B = 0 in step 1: dL/dA = s B^T (...) is exactly zero
        assert float(h.Bq.detach().abs().max()) > 0.0 and float(h.Bv.detach().abs().max()) > 0.0, i     # B has moved
    l2 = float(eng.train_step(img, tgt))
    assert l2 == l2 and abs(l2) < float("inf") and l2 != l1 and eng.optimizer.skipped_steps == 0
    for i, h in enumerate(eng.lora.handles):                                                          # after step 2 A has moved
        assert float(h.A.grad.abs().max()) > 0.0 and not torch.equal(h.A.detach(), A0[i]), i
    after = eng.model.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)        # the backbone: bit-identical
    # validation runs on the merged weights: it differs from the same engine with the handle ignored, and restores the base
    wt = torch.tensor([0.1, 10.0], device=dev)
    v = eng.validate_step(img, tgt, wt)
    lo, eng.lora = eng.lora, None
    v0 = eng.validate_step(img, tgt, wt)
    eng.lora = lo
    assert not torch.equal(v[0], v0[0])
    assert all(torch.equal(after[k], before[k]) for k in before) and eng.model.blocks[0].attn._lora is lo.handles[0]


# ---- script ------------------------------------------------------------------------------------------------------------------
def test_lora_checkpoint_entry_through_train_and_predict(dev, tmp_path):
    from adaptersis_amd import predict as P
    from adaptersis_amd import train as T
    model_args = ["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4", "--output_dir", str(tmp_path)]
    T._ENGINES.clear()
    T.train_seg(T.get_args_parser().parse_args(model_args + ["--epochs", "1", "--lr", "0.05", "--data_path", "synthetic", "--train_adapters",
                                                             "--train_encoder", "--train_backbone", "--lora_rank", "4", "--lora_alpha", "8"]))
    (eng_tr,) = T._ENGINES.values()
    T._ENGINES.clear()
    assert eng_tr.lora is not None and eng_tr.lora.rank == 4 and eng_tr.lora.alpha == 8.0 and eng_tr.optimizer.skipped_steps == 0
    ck = torch.load(os.path.join(tmp_path, "checkpoint.pth.tar"), map_location="cpu")
    assert "backbone" not in ck and ck["lora"]["rank"] == 4 and ck["lora"]["alpha"] == 8.0
    assert set(ck["lora"]["params"]) == {n for n, _ in eng_tr.lora.named_parameters()}
    for n, p in eng_tr.lora.named_parameters():
        assert torch.equal(ck["lora"]["params"][n], p.detach().cpu()), n
        assert float(p.detach().abs().max()) > 0.0, n
    eng = P.build_engine(P.get_args_parser().parse_args(model_args + ["--input", "unused"]))
    assert eng.lora is not None and eng.lora.rank == 4
    img, _ = W.synthetic_batch(3, 224)
    img = img.to(dev)
    assert torch.equal(eng.predict(img), eng_tr.predict(img))               # the engine's masks, reproduced from the file
    # ... through the merged weights, made of the entry's parameters (with the scripts' LayerScale init of 1e-5 and a few steps of
    # training the update itself is far below the 16-bit operand rounding: test_seg_engine_two_steps_with_lora shows its effect)
    for (n, p), (_, q) in zip(eng.lora.named_parameters(), eng_tr.lora.named_parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    w, h = eng.model.blocks[0].attn.qkv.weight, eng.lora.handles[0]
    base = w.detach().clone()
    with eng.lora.merged(eng.model):
        want = lora.merged_weight(base.double(), h.A.detach().double(), h.Bq.detach().double(), h.Bv.detach().double(), 2.0)
        assert float((w.detach().double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
    assert torch.equal(w.detach(), base)
