"""GPU: stochastic depth of the unfrozen ViT in DINOv2's subset form — the four row kernels of csrc/droppath.hip against the
existing ops on a torch gather / scatter of the same operands, ``Block.forward_train_rows`` / ``backward`` with explicit kept
lists against float64 autograd of the restated rule (tests/droppath_ref.py), eval paths that ignore the rate, the two engines,
and the ``backbone`` checkpoint entry."""
import os

import pytest
import torch

from adaptersis_amd import config, droppath, ops
from adaptersis_amd.dinov2.models import vision_transformer as vits
from adaptersis_amd.utils import weights as W
from tests import droppath_ref as R
from tests.conftest import rel_l2

pytestmark = pytest.mark.gpu

# ---- kernels -----------------------------------------------------------------------------------------------------------------
SEGS2, SEGS1 = [(3, 7), (3, 6)], [(5, 33)]
KERNEL_CASES = [
    ("two-all", SEGS2, [([0, 1, 2], 1.0), ([0, 1, 2], 1.0)]),
    ("two-one", SEGS2, [([1], 3.0), ([], 3.0)]),
    ("two-perm", SEGS2, [([2, 0], 1.5), ([1], 3.0)]),
    ("two-first-empty", SEGS2, [([], 1.5), ([2, 1], 1.5)]),
    ("two-none", SEGS2, [([], 1.5), ([], 1.5)]),
    ("one-all", SEGS1, [([0, 1, 2, 3, 4], 1.0)]),
    ("one-one", SEGS1, [([3], 5.0)]),
    ("one-perm", SEGS1, [([4, 0, 2], 5.0 / 3.0)]),
    ("one-none", SEGS1, [([], 1.25)]),
]


def _case(dev, D, segs, spec):
    rows_n = sum(b * n for b, n in segs)
    tag = f"{D}.{segs}"
    t = {k: W.tensor(f"dp.{k}.{tag}", (rows_n, D), s, sh) for k, s, sh in (("x", 1.5, 0.3), ("dres", 1.0, 0.0))}
    t["w"] = 1.0 + W.tensor(f"dp.w.{D}", (D,), 0.3)
    t["b"] = W.tensor(f"dp.b.{D}", (D,), 0.3)
    keep = droppath.pack([(spec, spec)], segs, dev)[0][0]
    rows = R.kept_rows(segs, spec)
    assert keep.rows == rows_n and keep.rows_c == rows.numel()
    t["y"] = W.tensor(f"dp.y.{tag}", (rows_n, D), 1.0)[: rows.numel()].contiguous()      # a compact [R', D] operand
    return t, keep, rows


@pytest.mark.parametrize("D", [128, 1024])
@pytest.mark.parametrize("name,segs,spec", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_layernorm_gather(dev, D, name, segs, spec):
    t, keep, rows = _case(dev, D, segs, spec)
    for dt in (torch.float16, torch.bfloat16):
        out = ops.layernorm_gather(t["x"].to(dev), t["w"].to(dev), t["b"].to(dev), 1e-6, dt, keep)
        assert out.shape == (rows.numel(), D) and out.dtype == dt
        if rows.numel():
            want = ops.layernorm(t["x"][rows].contiguous().to(dev), t["w"].to(dev), t["b"].to(dev), 1e-6, dt)
            assert torch.equal(out, want)


@pytest.mark.parametrize("D", [128, 1024])
@pytest.mark.parametrize("name,segs,spec", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_scaled_index_add(dev, D, name, segs, spec):
    t, keep, rows = _case(dev, D, segs, spec)
    x, y = t["x"], t["y"]
    out = ops.scaled_index_add(x.to(dev), y.to(dev), keep).cpu()
    dropped = torch.ones(x.shape[0], dtype=torch.bool)
    dropped[rows] = False
    assert torch.equal(out[dropped], x[dropped])                        # bit-equal where nothing is added
    if rows.numel():
        ay = R.row_alphas(segs, spec)[:, None] * y.double()
        err = (out[rows].double() - (x[rows].double() + ay)).abs()
        bound = 2.0 ** -22 * (x[rows].double().abs() + ay.abs())       # two fp32 roundings, a factor of two of margin
        print(name, D, "scaled_index_add max err / bound: %.3f" % float((err / bound.clamp_min(1e-300)).max()))
        assert bool((err <= bound).all())
    again = ops.scaled_index_add(x.to(dev), y.to(dev), keep).cpu()
    assert torch.equal(out, again)


@pytest.mark.parametrize("D", [128, 1024])
@pytest.mark.parametrize("name,segs,spec", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_gather_cast_colsum(dev, D, name, segs, spec):
    t, keep, rows = _case(dev, D, segs, spec)
    dres = t["dres"]
    for dt in (torch.float16, torch.bfloat16):
        out, part = ops.gather_cast_colsum(dres.to(dev), dt, keep)
        cast_only, none = ops.gather_cast_colsum(dres.to(dev), dt, keep, colsum=False)
        assert none is None and torch.equal(out, cast_only)
        assert out.shape == (rows.numel(), D) and part.shape == (ops.lib().asis_rowblock_nblk(rows.numel()), D)
        for c0, c1, alpha in R.segment_chunks(segs, spec):
            want = ops.cast_colsum(dres[rows[c0:c1]].contiguous().to(dev), dt, scale=alpha)[0]
            assert torch.equal(out[c0:c1], want)
        cs = ops.reduce_rows(part)
        want_cs = (R.row_alphas(segs, spec)[:, None] * dres[rows].double()).sum(0)
        if rows.numel():
            e = rel_l2(cs, want_cs)
            print(name, D, dt, "colsum rel-L2 %.2e" % e)
            assert e < 1e-6
        else:
            assert float(cs.abs().max()) == 0.0


@pytest.mark.parametrize("D", [128, 1024])
@pytest.mark.parametrize("name,segs,spec", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_layernorm_bwd_scatter(dev, D, name, segs, spec):
    t, keep, rows = _case(dev, D, segs, spec)
    x, dres, dy, w = t["x"], t["dres"], t["y"], t["w"]
    dx, part = ops.layernorm_bwd_scatter(dy.to(dev), x.to(dev), w.to(dev), 1e-6, dres.to(dev), keep)
    dxc = dx.cpu()
    dropped = torch.ones(x.shape[0], dtype=torch.bool)
    dropped[rows] = False
    assert torch.equal(dxc[dropped], dres[dropped])
    red = ops.reduce_rows(part.view(part.shape[0], 2 * D))
    if not rows.numel():
        assert float(red.abs().max()) == 0.0
        return
    want, _ = ops.layernorm_bwd(dy.to(dev), x[rows].contiguous().to(dev), w.to(dev), 1e-6, res=dres[rows].contiguous().to(dev))
    assert torch.equal(dx[rows.to(dev)], want)
    xr = x[rows].double().requires_grad_(True)
    wr, br = w.double().requires_grad_(True), t["b"].double().requires_grad_(True)
    (torch.nn.functional.layer_norm(xr, (D,), wr, br, 1e-6) * dy.double()).sum().backward()
    e_w, e_b = rel_l2(red[:D], wr.grad), rel_l2(red[D:], br.grad)
    print(name, D, "d weight %.2e d bias %.2e" % (e_w, e_b))
    assert e_w < 1e-5 and e_b < 1e-5


# ---- block -------------------------------------------------------------------------------------------------------------------
def _model(arch, dev, **kw):
    D, depth, heads, ffn = W.VIT_CONFIGS[arch]
    sd = W.make_vit_state_dict(arch, layerscale="kernel")
    model = vits.__dict__[arch](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0, **kw)
    model.load_state_dict(sd)
    return model.to(dev), sd, D, heads


def _block_run(blk, x2, dy2, segs, keep, dt, dev, with_grads=True):
    old = config.operand_dtype
    config.set_operand_dtype(dt)
    try:
        y, saved = blk.forward_train_rows(x2.to(dev), segs) if keep is None else blk.forward_train_rows(x2.to(dev), segs, keep=keep)
        S = 1024.0
        grads = {"blocks.1." + k: torch.full_like(p, 7.0, dtype=torch.float32) for k, p in blk.named_parameters()} if with_grads else None
        dx = blk.backward(saved, (dy2 * S).to(dev).contiguous(), 1.0 / S, grads, "blocks.1")
    finally:
        config.set_operand_dtype(old)
    return y, dx / S, grads


def _ref_run(sd, x2, dy2, segs, keep, heads):
    osd = {k: v.double().clone().requires_grad_(True) for k, v in sd.items() if k.startswith("blocks.1.")}
    xr = x2.double().clone().requires_grad_(True)
    D = x2.shape[1]
    xs, r0 = [], 0
    for b, n in segs:
        xs.append(xr[r0:r0 + b * n].view(b, n, D))
        r0 += b * n
    y = torch.cat([o.reshape(-1, D) for o in R.block(xs, osd, "blocks.1", heads, keep)])
    (y * dy2.double()).sum().backward()
    zero = lambda k: torch.zeros_like(osd[k])
    return y.detach(), xr.grad, {k: (v.grad if v.grad is not None else zero(k)) for k, v in osd.items()}


def _check(y, dx, grads, y_ref, dx_ref, gref, dt, what, rows=slice(None), amp=1.0):
    """the bars of test_block_forward_train_and_backward.  ``rows`` / ``amp``: y and dx compared on those rows only, at ``amp``
    times the bar (see test_block_sample_dropped_in_both_branches); the parameter gradients always at the bar itself"""
    f16 = dt == torch.float16
    e_y, e_dx = rel_l2(y[rows], y_ref[rows]) / amp, rel_l2(dx[rows], dx_ref[rows]) / amp
    errs = {}
    for k in grads:
        if float(gref[k].norm()) == 0.0:
            assert float(grads[k].abs().max()) == 0.0, k       # a skipped branch: exactly zero
        else:
            errs[k] = rel_l2(grads[k], gref[k])
    print(what, dt, "y %.2e dx %.2e" % (e_y, e_dx), {k.replace("blocks.1.", ""): "%.1e" % v for k, v in errs.items()})
    assert e_y < (5e-4 if f16 else 4e-3)
    tol = 3e-3 if f16 else 2.5e-2
    assert e_dx < tol and max(errs.values()) < tol, errs


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("arch", ["vit_tiny_test", "vit_tiny_swiglu"])
def test_block_subset_forward_backward(dev, arch, dt):
    """attention on samples [2, 0] (alpha 1.5), FFN on [1] (alpha 3): every sample drops one branch"""
    B, N = 3, 70
    model, sd, D, heads = _model(arch, dev)
    x2, dy2 = W.tensor("dpb.x", (B * N, D), 1.0), W.tensor("dpb.dy", (B * N, D), 1.0)
    segs, keep = [(B, N)], ([([2, 0], 1.5)], [([1], 3.0)])
    y, dx, grads = _block_run(model.blocks[1], x2, dy2, segs, keep, dt, dev)
    _check(y, dx, grads, *_ref_run(sd, x2, dy2, segs, keep, heads), dt, arch)
    # without grads: the same input gradient, no parameter work
    _, dx_only, _ = _block_run(model.blocks[1], x2, dy2, segs, keep, dt, dev, with_grads=False)
    assert torch.equal(dx_only, dx)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_block_sample_dropped_in_both_branches(dev, dt):
    B, N = 3, 70
    model, sd, D, heads = _model("vit_tiny_test", dev)
    x2, dy2 = W.tensor("dpb.x", (B * N, D), 1.0), W.tensor("dpb.dy", (B * N, D), 1.0)
    segs, keep = [(B, N)], ([([0], 3.0)], [([0], 3.0)])
    y, dx, grads = _block_run(model.blocks[1], x2, dy2, segs, keep, dt, dev)
    assert torch.equal(y[N:].cpu(), x2[N:])                          # samples 1 and 2: untouched
    assert torch.equal((dx * 1024.0)[N:].cpu(), dy2[N:] * 1024.0)    # dx = dres there (the power-of-two scale is exact)
    # sample 0 against autograd.  The other rows carry no error at all, and the kernels' error sits in the branch outputs (16-bit
    # operands), which enter sample 0 times alpha = 3 where the bars were set for alpha = 1: y = x + alpha * branch and
    # dx = dres + alpha * J^T(...) are compared on sample 0's rows at alpha times the bar; a parameter gradient is linear in
    # alpha on both sides, so its relative error keeps the bar
    _check(y, dx, grads, *_ref_run(sd, x2, dy2, segs, keep, heads), dt, "both", rows=slice(0, N), amp=3.0)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_block_full_keep_lists_agree_with_no_keep(dev, dt):
    B, N = 3, 70
    model, sd, D, heads = _model("vit_tiny_test", dev)
    x2, dy2 = W.tensor("dpb.x", (B * N, D), 1.0), W.tensor("dpb.dy", (B * N, D), 1.0)
    segs, keep = [(B, N)], ([([0, 1, 2], 1.0)], [([0, 1, 2], 1.0)])
    y, dx, grads = _block_run(model.blocks[1], x2, dy2, segs, keep, dt, dev)
    y0, dx0, grads0 = _block_run(model.blocks[1], x2, dy2, segs, None, dt, dev)
    _check(y, dx, grads, y0, dx0, grads0, dt, "full")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
def test_block_two_stacked_segments(dev, dt):
    """different kept lists per segment; the second segment's FFN list is empty; then a block whose FFN branch keeps nothing"""
    model, sd, D, heads = _model("vit_tiny_test", dev)
    segs = [(2, 71), (2, 70)]
    rows = sum(b * n for b, n in segs)
    x2, dy2 = W.tensor("dpb2.x", (rows, D), 1.0), W.tensor("dpb2.dy", (rows, D), 1.0)
    keep = ([([1], 2.0), ([1, 0], 1.0)], [([0, 1], 1.0), ([], 2.0)])
    y, dx, grads = _block_run(model.blocks[1], x2, dy2, segs, keep, dt, dev)
    _check(y, dx, grads, *_ref_run(sd, x2, dy2, segs, keep, heads), dt, "two segs")
    keep = ([([0], 2.0), ([], 2.0)], [([], 2.0), ([], 2.0)])
    y, dx, grads = _block_run(model.blocks[1], x2, dy2, segs, keep, dt, dev)
    _check(y, dx, grads, *_ref_run(sd, x2, dy2, segs, keep, heads), dt, "ffn skipped")


# ---- eval ignores the rate -------------------------------------------------------------------------------------------------------
def test_eval_paths_ignore_the_rate(dev):
    from adaptersis_amd.dinov2.layers.blocks import run_blocks
    m0, _, D, _ = _model("vit_tiny_test", dev)
    m1, _, _, _ = _model("vit_tiny_test", dev, drop_path_rate=0.4, drop_path_uniform=True)
    assert m1.blocks[1].sample_drop_ratio == 0.4
    x = W.tensor("dpe.x", (3, 70, D), 1.0).to(dev)
    assert torch.equal(m1.blocks[1](x), m0.blocks[1](x))
    segs = [(3, 70)]
    assert torch.equal(run_blocks(m1.blocks, x.view(-1, D), segs), run_blocks(m0.blocks, x.view(-1, D), segs))
    y1, _ = m1.blocks[1].forward_train(x)          # no keep: nothing is dropped whatever the rate
    y0, _ = m0.blocks[1].forward_train(x)
    assert torch.equal(y1, y0)


# ---- engines ---------------------------------------------------------------------------------------------------------------------
def _seg_engine(dev, rate, seed=0, **kw):
    from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
    from adaptersis_amd.backbones.decoders import FeatureDecoder
    from adaptersis_amd.backbones.encoders import FeatureEncoder
    from adaptersis_amd.backbones.engines import SegEngine
    arch, feats = "vit_tiny_test", (128, 32, 16, 16, 8)
    model, _, D, _ = _model(arch, dev, drop_path_rate=rate, drop_path_uniform=True)
    enc = FeatureEncoder(embed_dim=D); enc.load_state_dict(W.make_encoder_state_dict(D))
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4); cv.load_state_dict(W.make_cavit_state_dict(D, mode="kernel"))
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25); cn.load_state_dict(W.make_cacnn_state_dict(D, mode="kernel"))
    dec = FeatureDecoder(embed_dim=D, num_classes=2, features=list(feats)); dec.load_state_dict(W.make_feature_decoder_state_dict(D, 2, features=feats))
    kw.setdefault("train_backbone", True)
    kw.setdefault("optimize_backbone", kw["train_backbone"])
    return SegEngine(model, enc.to(dev), cv.to(dev), cn.to(dev), dec.to(dev), lr=0.05, mode="train_adapters", train_encoder=True,
                     drop_path_seed=seed, **kw)


def test_seg_engine_refuses_a_rate_without_train_backbone(dev):
    with pytest.raises(ValueError, match="train_backbone"):
        _seg_engine(dev, 0.3, train_backbone=False)


def test_seg_engine_step_with_drop_path(dev):
    img, tgt = W.synthetic_batch(3, 224)
    img, tgt = img.to(dev), tgt.to(dev)
    wt = torch.tensor([0.1, 10.0], device=dev)
    a, b, c, z = _seg_engine(dev, 0.3, 0), _seg_engine(dev, 0.3, 0), _seg_engine(dev, 0.3, 1), _seg_engine(dev, 0.0)
    assert z.drop_path is None and a.drop_path.rates == [0.3] * 4
    segs = [(3, 257), (3, 256)]
    assert droppath.DropPathSampler([0.3] * 4, 0).plan(segs) != droppath.DropPathSampler([0.3] * 4, 1).plan(segs)
    # validation ignores the rate: bit-equal to the rate-0 engine on the same weights
    va, vz = a.validate_step(img, tgt, wt), z.validate_step(img, tgt, wt)
    assert torch.equal(va[0], vz[0]) and torch.equal(torch.as_tensor(va[1]), torch.as_tensor(vz[1]))
    la, lb, lc, lz = (float(e.train_step(img, tgt)) for e in (a, b, c, z))
    print("losses: seed 0 %.8f / %.8f, seed 1 %.8f, rate 0 %.8f" % (la, lb, lc, lz))
    assert la == la and abs(la) < float("inf")
    assert la == lb                 # same seed: the same samples, and no atomics in the forward
    assert la != lc and la != lz
    assert a.optimizer.skipped_steps == 0
    l2 = float(a.train_step(img, tgt))      # a second step: new draws, updated backbone
    assert l2 == l2 and l2 != la


def test_end_to_end_engine_step_with_drop_path(dev):
    from adaptersis_amd.backbones.decoders import DecoderSETR
    from adaptersis_amd.backbones.engines import EndToEndEngine
    feats = [32, 16, 16, 8]

    def build(rate, seed):
        model, _, D, _ = _model("vit_tiny_test", dev, drop_path_rate=rate, drop_path_uniform=True)
        dec = DecoderSETR(D, 2, features=feats)
        dec.load_state_dict(W.make_setr_state_dict(D, 2, feats))
        return EndToEndEngine(model, dec.to(dev), lr=0.05, blocks_per_bucket=2, drop_path_seed=seed)
    img, tgt = W.synthetic_batch(3, 224)
    img, tgt = img.to(dev), tgt.to(dev)
    la, lb, lc, lz = (float(build(r, s).train_step(img, tgt)) for r, s in ((0.3, 0), (0.3, 0), (0.3, 1), (0.0, 0)))
    print("e2e losses: %.8f %.8f %.8f rate 0 %.8f" % (la, lb, lc, lz))
    assert la == la and abs(la) < float("inf")
    assert la == lb and la != lc and la != lz


# ---- checkpoint ------------------------------------------------------------------------------------------------------------------
def test_backbone_checkpoint_entry(dev, tmp_path):
    from adaptersis_amd import predict as P
    from adaptersis_amd import train as T
    from adaptersis_amd.utils import misc as utils
    argv = ["--arch", "vit_tiny_test", "--imsize", "224", "--batch_size_per_gpu", "4", "--epochs", "1", "--lr", "0.05",
            "--data_path", "synthetic", "--output_dir", str(tmp_path), "--train_adapters", "--train_encoder", "--train_backbone",
            "--optimize_backbone", "--drop_path", "0.3", "--drop_path_uniform", "--drop_path_seed", "2"]
    T._ENGINES.clear()
    T.train_seg(T.get_args_parser().parse_args(argv))
    (eng,) = T._ENGINES.values()
    assert eng.train_backbone and eng.drop_path is not None and eng.drop_path.seed == 2 and eng.optimizer.skipped_steps == 0
    trained = {k: v.detach().cpu().clone() for k, v in eng.model.state_dict().items()}
    init = W.make_vit_state_dict("vit_tiny_test", patch_size=14, layerscale="init")
    assert not torch.equal(trained["blocks.0.attn.qkv.weight"], init["blocks.0.attn.qkv.weight"])       # the backbone trained
    path = os.path.join(tmp_path, "checkpoint.pth.tar")
    ck = torch.load(path, map_location="cpu")
    assert "backbone" in ck and all(k.startswith("module.") for k in ck["backbone"])
    assert {k[len("module."):] for k in ck["backbone"]} == set(trained)
    assert all(torch.equal(ck["backbone"]["module." + k], v) for k, v in trained.items())
    T._ENGINES.clear()

    def perturbed():
        m, _, _, _ = _model("vit_tiny_test", dev)
        with torch.no_grad():
            for p in m.parameters():
                p.add_(0.25)
        return m
    m1 = perturbed()
    utils.restart_from_checkpoint(path, backbone=m1)
    assert all(torch.equal(v.cpu(), trained[k]) for k, v in m1.state_dict().items())
    m2 = perturbed()
    P.load_checkpoint(path, eng.seg_decoder, {"backbone": m2})
    assert all(torch.equal(v.cpu(), trained[k]) for k, v in m2.state_dict().items())
    bad = dict(ck)
    bad["backbone"] = {k: (v[:1] if k.endswith("norm.weight") else v) for k, v in ck["backbone"].items()}
    with pytest.raises(ValueError, match="backbone"):
        P.load_checkpoint(path, eng.seg_decoder, {"backbone": perturbed()}, ck=bad)
    # a resume through the script restores it too
    args = T.get_args_parser().parse_args(argv)
    args.evaluate = True
    T.train_seg(args)
    (eng2,) = T._ENGINES.values()
    assert eng2 is not eng
    assert all(torch.equal(v.cpu(), trained[k]) for k, v in eng2.model.state_dict().items())
    T._ENGINES.clear()
