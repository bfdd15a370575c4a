"""SHA-256 of every output of a fixed, seeded list of calls into the host layer of the ViT and adapter blocks (dinov2/layers/
blocks.py, backbones/masktrans_block.py, backbones/ops/modules/ms_deform_attn.py), one line per output.  The host layer decides
which kernel sees which operand, so two trees with the same built library compute the same thing exactly when the listings
are equal (run it twice on one tree first: a line that differs there comes from a kernel that is not run-to-run reproducible):
    python scripts/block_hashes.py [--tree PATH] > hashes.txt
``--tree`` is put in front of ``sys.path``: the package of another checkout (with a built library) under the same list of calls.
The list takes each host route once, at the smallest shapes of tests/test_gpu_{lnfold,block_precise,vit_bwd,droppath,lora}.py:
``Block.forward_rows`` (Mlp / SwiGLU, one / two token batches) under every combination of fold_attn_scale, fused_qkv, vt_stream,
precise_attention and split_attn_out; ``_forward_rows_precise`` on the precise_parts subsets of config.py's A/B table with one,
two and three batches; ``run_blocks`` on the LayerNorm-fold chain; ``forward_train_rows`` + ``backward`` (LayerScale at 1e-5 and
mixed, input gradient only, stochastic depth, LoRA); the MaskTransformer head (plain, split, dropout) and ``MSDeformAttn``.
``--packs`` instead counts the pack builds (``ops.cast_pad`` calls under no_grad: what the pack caches run) of two rounds of
the same calls: the second round must build nothing."""
import argparse
import contextlib
import hashlib
import itertools
import os
import sys
import types

import torch

KNOBS = ("precise_level", "precise_parts", "fold_attn_scale", "fused_qkv", "vt_stream", "precise_attention", "split_attn_out",
         "split_conv", "ln_fold", "mx_dense", "_pa")
SEGS = {1: [(1, 257)], 2: [(2, 301), (1, 300)], 3: [(1, 197), (2, 145), (1, 257)]}
PARTS = ("qkv,proj,fc1,fc2", "qkv,proj,fc1", "proj,fc1,fc2", "proj,fc1", "qkv,proj", "proj")


@contextlib.contextmanager
def knobs(config, **kw):
    keep = {k: getattr(config, k) for k in KNOBS}
    base = dict(precise_level=0, precise_parts=frozenset(PARTS[0].split(",")), fold_attn_scale=True, fused_qkv=False, vt_stream=True,
                precise_attention=False, split_attn_out=False, split_conv=True, ln_fold=True, mx_dense=True, _pa="0")
    try:
        for k, v in {**base, **kw}.items():
            setattr(config, k, v)
        yield
    finally:
        for k, v in keep.items():
            setattr(config, k, v)


def randn(g, shape, dev, scale=1.0):
    return (scale * torch.randn(shape, generator=g)).to(dev)


def make_block(BL, D, H, ffn, dev, seed, init=0.3, **kw):
    """a seeded block with non-trivial LayerNorm affines; LayerScale: ``init`` everywhere ("mixed": ls1 = 1e-5, ls2 in [0.05, 0.3])"""
    torch.manual_seed(seed)
    blk = BL.Block(D, H, qkv_bias=True, init_values=1e-5 if init == "mixed" else init, ffn_layer=ffn, **kw)
    with torch.no_grad():
        for n in (blk.norm1, blk.norm2):
            n.weight.add_(0.1 * torch.randn(D)); n.bias.add_(0.1 * torch.randn(D))
        if init == "mixed":
            blk.ls2.gamma.copy_(0.05 + 0.25 * torch.rand(D))
    return blk.to(dev).eval()


def grads_of(mod, prefix):
    return {prefix + "." + k: torch.full_like(p, 7.0, dtype=torch.float32) for k, p in mod.named_parameters()}


def train_bwd(blk, x, dy, segs, grads, keep=None, S=1024.0):
    y, saved = blk.forward_train_rows(x, segs) if keep is None else blk.forward_train_rows(x, segs, keep=keep)
    dx = blk.backward(saved, (dy * S).contiguous(), 1.0 / S, grads, "blocks.0")
    return dict(y=y, dx=dx, **{n: grads[n] for n in sorted(grads or ())})


def calls(dev):
    """-> (name, thunk) pairs; a thunk returns a tensor or a dict of named tensors."""
    from adaptersis_amd import config, lora
    from adaptersis_amd.backbones import masktrans_block as MT
    from adaptersis_amd.backbones.ops.modules.ms_deform_attn import MSDeformAttn
    from adaptersis_amd.dinov2.layers import blocks as BL
    config.set_operand_dtype(torch.float16)
    g = torch.Generator().manual_seed(20261020)
    K = lambda **kw: knobs(config, **kw)

    def under(kw, fn):
        def thunk():
            with K(**kw):
                return fn()
        return thunk

    # ---- Block.forward_rows: every switch of the level-0 host path ----
    fwd = {"mlp256": make_block(BL, 256, 4, BL.Mlp, dev, 11), "sg256": make_block(BL, 256, 4, BL.SwiGLUFFNFused, dev, 12),
           "sg384": make_block(BL, 384, 6, BL.SwiGLUFFNFused, dev, 13)}
    xs = {(name, n): randn(g, (sum(b * t for b, t in SEGS[n]), blk.attn.qkv.in_features), dev) for name, blk in fwd.items() for n in SEGS}
    names = ("fold_attn_scale", "fused_qkv", "vt_stream", "precise_attention", "split_attn_out")
    for name in ("mlp256", "sg256"):
        for n in (1, 2):
            for bits in itertools.product((True, False), repeat=5):
                kw = dict(zip(names, bits))
                tag = "".join("FQVPS"[i] if b else "-" for i, b in enumerate(bits))
                yield f"forward_rows {name} segs={n} {tag}", under(kw, lambda b=fwd[name], x=xs[(name, n)], n=n: b.forward_rows(x, SEGS[n]))
    yield "forward_rows mlp256 segs=3", under({}, lambda: fwd["mlp256"].forward_rows(xs[("mlp256", 3)], SEGS[3]))
    yield "forward_rows mlp256 segs=3 P", under(dict(precise_attention=True), lambda: fwd["mlp256"].forward_rows(xs[("mlp256", 3)], SEGS[3]))
    # ---- _forward_rows_precise ----
    for name in ("mlp256", "sg384"):
        for parts in PARTS:
            for n in SEGS:
                for mx in (True, False) if parts in (PARTS[0], "proj,fc1") else (True,):
                    kw = dict(precise_level=2, precise_parts=frozenset(parts.split(",")), mx_dense=mx)
                    yield (f"precise {name} {parts} segs={n} mx={int(mx)}",
                           under(kw, lambda b=fwd[name], x=xs[(name, n)], n=n: b.forward_rows(x, SEGS[n])))
    # ---- run_blocks on the LayerNorm-fold chain (ViT-L width: the shapes the chain's GEMM forms take) ----
    chain = [make_block(BL, 1024, 16, BL.Mlp, dev, 20 + i, init=1e-5, attn_class=BL.MemEffAttention) for i in range(3)]
    for segs in ([(5, 1765), (5, 1764)], [(5, 1765), (5, 1764), (5, 1764)], [(10, 1765)]):    # the V^T GEMM's form needs 5 images
        x = randn(g, (sum(b * t for b, t in segs), 1024), dev)
        for fs in (True, False):
            def fold(x=x, segs=segs):
                if not all(b.fold_ok(x.shape[0], segs) for b in chain):
                    raise ValueError(f"run_blocks: {segs} is not on the LayerNorm-fold chain")
                return BL.run_blocks(chain, x, segs)
            yield f"run_blocks fold {len(segs)} segs fold_attn_scale={int(fs)}", under(dict(fold_attn_scale=fs), fold)
    del chain
    # ---- forward_train_rows + backward ----
    for ffn_name, ffn in (("mlp", BL.Mlp), ("swiglu", BL.SwiGLUFFNFused)):
        for init in (1e-5, "mixed"):
            blk = make_block(BL, 128, 2, ffn, dev, 31, init=init)
            for segs in ([(2, 150)], [(2, 76), (2, 75)], [(1, 100), (1, 101), (1, 102)]):
                R = sum(b * t for b, t in segs)
                x, dy = randn(g, (R, 128), dev), randn(g, (R, 128), dev)
                for pa in (False, True):
                    yield (f"train+bwd {ffn_name} init={init} segs={len(segs)} P={int(pa)}", under(dict(precise_attention=pa, split_attn_out=pa),
                           lambda blk=blk, x=x, dy=dy, segs=segs: train_bwd(blk, x, dy, segs, grads_of(blk, "blocks.0"))))
                yield f"train+bwd {ffn_name} init={init} segs={len(segs)} dx only", under({}, lambda blk=blk, x=x, dy=dy, segs=segs: train_bwd(blk, x, dy, segs, None))
            segs, R = [(3, 100)], 300
            x, dy = randn(g, (R, 128), dev), randn(g, (R, 128), dev)
            for kname, keep in (("subset", ([([2, 0], 1.5)], [([1], 3.0)])), ("both", ([([0], 3.0)], [([0], 3.0)])), ("none-attn", ([([], 1.0)], [([1, 2], 1.5)]))):
                yield (f"train+bwd {ffn_name} init={init} keep={kname}",
                       under({}, lambda blk=blk, x=x, dy=dy, segs=segs, keep=keep: train_bwd(blk, x, dy, segs, grads_of(blk, "blocks.0"), keep=keep)))
    blk = make_block(BL, 128, 2, BL.Mlp, dev, 32, init=0.3)
    lo = lora.LoRA(types.SimpleNamespace(blocks=[blk]), 4, 8.0)
    h = lo.handles[0]
    with torch.no_grad():
        h.Bq.copy_(randn(g, tuple(h.Bq.shape), dev, 0.05)); h.Bv.copy_(randn(g, tuple(h.Bv.shape), dev, 0.05))
    for segs in ([(2, 17), (2, 16)], [(2, 150)]):
        R = sum(b * t for b, t in segs)
        x, dy = randn(g, (R, 128), dev), randn(g, (R, 128), dev)
        for pa in (False, True):
            lg = lambda: {n: torch.full_like(p, 7.0) for n, p in zip(h.names(), h.params)}
            yield (f"train+bwd lora segs={segs} P={int(pa)}", under(dict(precise_attention=pa),
                   lambda x=x, dy=dy, segs=segs, lg=lg: train_bwd(blk, x, dy, segs, lg())))
        yield f"train+bwd lora segs={segs} dx only", under({}, lambda x=x, dy=dy, segs=segs: train_bwd(blk, x, dy, segs, None))

    def merged(x=x, segs=segs):
        with lo.merged(types.SimpleNamespace(blocks=[blk])):
            return blk.forward_rows(x, segs)
    yield "forward_rows under lora.merged", under({}, merged)
    # ---- the MaskTransformer head: its blocks plain / split / with dropout, and the projections around them ----
    for dropout in (0.0, 0.1):
        torch.manual_seed(41)
        head = MT.MaskTransformer(n_cls=2, patch_size=14, d_encoder=128, n_layers=2, n_heads=2, d_model=128, d_ff=256, drop_path_rate=0.0,
                                  dropout=dropout).to(dev)
        tok, dl = randn(g, (2, 256, 128), dev), randn(g, (2 * 256, 2), dev)
        for sp in (False, True):
            def core(head=head, tok=tok, dl=dl, save=True):
                head.train(save)
                head.drop_step = 0
                logits, saved = head._forward_core(tok, save=save)
                if not save:
                    return logits
                grads = {n: torch.full_like(p, 7.0) for n, p in head.named_parameters()}
                head._backward_core(saved, dl * head.loss_scale, 1.0 / head.loss_scale, grads)
                return dict(logits=logits, **{n: grads[n] for n in sorted(grads)})
            yield f"masktrans dropout={dropout} split_conv={int(sp)} train", under(dict(split_conv=sp), core)
            if not dropout:
                yield f"masktrans split_conv={int(sp)} eval", under(dict(split_conv=sp), lambda core=core: core(save=False))
    # ---- MSDeformAttn ----
    torch.manual_seed(51)
    shapes = [(12, 12), (6, 6), (3, 3)]
    msda = MSDeformAttn(d_model=128, n_levels=3, n_heads=8, n_points=4)
    with torch.no_grad():
        msda.sampling_offsets.weight.copy_(0.02 * torch.randn(msda.sampling_offsets.weight.shape))
        msda.attention_weights.weight.copy_(0.1 * torch.randn(msda.attention_weights.weight.shape))
        msda.attention_weights.bias.copy_(0.1 * torch.randn(msda.attention_weights.bias.shape))
    msda = msda.to(dev)
    B, Lq, Lin = 2, 300, sum(a * b for a, b in shapes)
    q16, f16 = randn(g, (B * Lq, 128), dev).half(), randn(g, (B * Lin, 128), dev).half()
    ref = torch.rand((Lq, 2), generator=g).to(dev)
    sh = torch.tensor(shapes, dtype=torch.int32, device=dev)
    st = torch.tensor([0, 144, 180], dtype=torch.int32, device=dev)
    res, gam, dout = randn(g, (B * Lq, 128), dev), randn(g, (128,), dev, 0.3), randn(g, (B * Lq, 128), dev)
    gamma = torch.nn.Parameter(gam.clone())
    for pa in ("0", "1"):
        yield f"msda forward16 precise_adapters={pa}", under(dict(_pa=pa), lambda: msda.forward16(q16, f16, ref, sh, st, B, Lq, Lin, res=res, scale_n=gam))

        def train():
            out, saved = msda.forward16_train(q16, f16, ref, sh, st, B, Lq, Lin, res=res, scale_n=gam)
            grads = grads_of(msda, "m")
            grads["m.gamma"] = torch.full_like(gam, 7.0)
            dq, dfeat = msda.backward16(saved, dout * 1024.0, 1.0 / 1024.0, grads, "m", gamma=gamma, gamma_name="m.gamma")
            return dict(out=out, dq=dq, dfeat=dfeat, **{n: grads[n] for n in sorted(grads)})
        yield f"msda forward16_train+backward16 precise_adapters={pa}", under(dict(_pa=pa), train)


def pack_counts(dev):
    """pack builds of two rounds of: forward_rows with precise_attention, the same block at precise_level 2 (the weights' rounding
    residuals again), forward_train_rows + backward with gradients"""
    from adaptersis_amd import config, ops
    from adaptersis_amd.dinov2.layers import blocks as BL
    config.set_operand_dtype(torch.float16)
    count = [0]
    real = ops.cast_pad

    def counting(*a, **kw):
        count[0] += not torch.is_grad_enabled()
        return real(*a, **kw)
    ops.cast_pad = counting
    g = torch.Generator().manual_seed(7)
    blk = make_block(BL, 256, 4, BL.Mlp, dev, 11)
    x, dy = randn(g, (902, 256), dev), randn(g, (902, 256), dev)
    steps = (("forward_rows precise_attention", dict(precise_attention=True), lambda: blk.forward_rows(x, SEGS[2])),
             ("forward_rows precise_level 2", dict(precise_level=2, mx_dense=False), lambda: blk.forward_rows(x, SEGS[2])),
             ("forward_train_rows + backward", {}, lambda: train_bwd(blk, x, dy, SEGS[2], grads_of(blk, "blocks.0"))))
    for rnd in (1, 2):
        for what, kw, fn in steps:
            n0 = count[0]
            with knobs(config, **kw):
                fn()
            print(f"packs round {rnd}: {count[0] - n0:3d}  {what}")
            if rnd == 2 and count[0] != n0:
                raise SystemExit(f"{what}: the second round built {count[0] - n0} packs")
    torch.cuda.synchronize()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose adaptersis_amd package (with its built library) runs the list")
    ap.add_argument("--packs", action="store_true", help="count pack builds instead of hashing outputs")
    ap.add_argument("--only", default="", help="run only the calls whose name contains this")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    dev = torch.device("cuda:0")
    if a.packs:
        pack_counts(dev)
        sys.exit(0)
    n = 0
    for name, thunk in calls(dev):
        if a.only not in name:
            continue
        try:
            out = thunk()
        except ValueError as e:     # a refused argument is a result too: the other tree must refuse the same call
            print(f"ValueError  {name}: {e}", flush=True)
            continue
        for k, t in (out if isinstance(out, dict) else {"out": out}).items():
            print(f"{hashlib.sha256(t.detach().float().cpu().numpy().tobytes()).hexdigest()}  {name} [{k}] {t.dtype} {list(t.shape)}", flush=True)
            n += 1
    print(f"# {n} outputs", file=sys.stderr)
