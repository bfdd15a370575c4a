"""SHA-256 of every output of a fixed, seeded list of ``train_step`` calls into the two engines (backbones/engines.py), one line
per output.  The engines decide which kernel sees which tensor, so two trees with the same built library take the same steps
exactly when the listings are equal (run it twice on one tree first: a line that differs there comes from a kernel that is not
run-to-run reproducible):
    python scripts/step_hashes.py [--tree PATH] > hashes.txt
``--tree`` is put in front of ``sys.path``: the package of another checkout (with a built library) under the same list of calls.
The engine is the tiny one of tests/test_gpu_mean_teacher.py (``vit_tiny_test``, 224 x 224, batch 3, FeatureDecoder widths
(128, 32, 16, 16, 8)); the MLA, UNet and SETR heads as tests/test_gpu_mla.py, tests/test_gpu_e2e.py and tests/test_gpu_droppath.py
build them, at that width.  Every case takes two steps from seeded weights and lists, after each: the loss, ``taps["logits"]``,
``flat`` and ``grad`` of every bucket the optimizer steps, and the BatchNorm buffers of encoder and head.  A ``SegEngine`` on the
`train.py` flow skips the last stage's CACNN only when no taps are asked for, so those cases run once more without taps (no
logits line).  ``reference_exact`` with the FeatureDecoder lists step 2's logits with ``config.dual_stream`` on and off."""
import argparse
import hashlib
import os
import sys

import torch

ARCH, SIZE, BATCH, FEATS = "vit_tiny_test", 224, 3, (128, 32, 16, 16, 8)


def seg_engine(dev, head="feature", drop_path_rate=0.0, **kw):
    from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
    from adaptersis_amd.backbones.decoders import DecoderMLA, FeatureDecoder
    from adaptersis_amd.backbones.encoders import FeatureEncoder
    from adaptersis_amd.backbones.engines import SegEngine
    from adaptersis_amd.backbones.unet_parts import UNet
    from adaptersis_amd.dinov2.models import vision_transformer as vits
    from adaptersis_amd.utils import weights as W
    D, _, _, ffn = W.VIT_CONFIGS[ARCH]
    vkw = dict(drop_path_rate=drop_path_rate, drop_path_uniform=True) if drop_path_rate else {}
    model = vits.__dict__[ARCH](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0, **vkw)
    model.load_state_dict(W.make_vit_state_dict(ARCH, layerscale="kernel"))
    enc = FeatureEncoder(embed_dim=D); enc.load_state_dict(W.make_encoder_state_dict(D))
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4); cv.load_state_dict(W.make_cavit_state_dict(D, mode="kernel"))
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25); cn.load_state_dict(W.make_cacnn_state_dict(D, mode="kernel"))
    if head == "feature":
        dec = FeatureDecoder(embed_dim=D, num_classes=2, features=list(FEATS)); dec.load_state_dict(W.make_feature_decoder_state_dict(D, 2, features=FEATS))
    elif head == "unet":
        dec = UNet(D, 2); dec.load_state_dict(W.make_unet_state_dict(D, 2))
        kw.setdefault("loss", "ce_dc")
    else:
        dec = DecoderMLA(img_size=SIZE, mla_channels=D, mlahead_channels=32, num_classes=2); dec.load_state_dict(W.make_decoder_mla_state_dict(D, 32, 2))
    return SegEngine(model.to(dev), enc.to(dev), cv.to(dev), cn.to(dev), dec.to(dev), lr=0.05, **kw)


def e2e_engine(dev, drop_path_rate=0.0):
    from adaptersis_amd.backbones.decoders import DecoderSETR
    from adaptersis_amd.backbones.engines import EndToEndEngine
    from adaptersis_amd.dinov2.models import vision_transformer as vits
    from adaptersis_amd.utils import weights as W
    D, _, _, ffn = W.VIT_CONFIGS[ARCH]
    vkw = dict(drop_path_rate=drop_path_rate, drop_path_uniform=True) if drop_path_rate else {}
    model = vits.__dict__[ARCH](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0, **vkw)
    model.load_state_dict(W.make_vit_state_dict(ARCH, layerscale="kernel"))
    feats = list(FEATS[1:])
    dec = DecoderSETR(D, 2, features=feats); dec.load_state_dict(W.make_setr_state_dict(D, 2, feats))
    return EndToEndEngine(model.to(dev), dec.to(dev), lr=0.05, blocks_per_bucket=2)


TA = dict(mode="train_adapters")
TB = dict(mode="train_adapters", train_encoder=True, train_backbone=True, blocks_per_bucket=2)
CASES = [   # name, builder, keywords
    ("reference_exact feature", seg_engine, dict()),
    ("reference_exact unet", seg_engine, dict(head="unet")),
    ("reference_exact mla", seg_engine, dict(head="mla")),
    ("train_adapters feature", seg_engine, dict(TA)),
    ("train_adapters feature train_encoder", seg_engine, dict(TA, train_encoder=True)),
    ("train_adapters mla", seg_engine, dict(TA, head="mla")),
    ("train_adapters mla train_encoder", seg_engine, dict(TA, head="mla", train_encoder=True)),
    ("train_backbone", seg_engine, dict(TB)),
    ("train_backbone optimize adamw layer_decay", seg_engine, dict(TB, optimize_backbone=True, optimizer="adamw", layer_decay=0.75)),
    ("train_backbone unet", seg_engine, dict(TB, head="unet")),
    ("train_backbone lora_rank=4", seg_engine, dict(TB, lora_rank=4)),
    ("train_backbone drop_path", seg_engine, dict(TB, optimize_backbone=True, drop_path_rate=0.3)),
    ("teacher=ema distill_flip", seg_engine, dict(TA, train_encoder=True, ema_decay=0.5, teacher="ema", distill_threshold=0.6, distill_flip=True)),
    ("mix=classmix teacher=ema", seg_engine, dict(TA, train_encoder=True, ema_decay=0.5, teacher="ema", distill_threshold=0.6, mix="classmix", mix_seed=3)),
    ("EndToEndEngine", e2e_engine, dict()),
    ("EndToEndEngine drop_path", e2e_engine, dict(drop_path_rate=0.3)),
]


def outputs(eng, loss, taps):
    out = {"loss": loss}
    if taps is not None:
        out["logits"] = taps["logits"]
    for i, b in enumerate(eng.optimizer.buckets):
        out[f"bucket{i}.flat"], out[f"bucket{i}.grad"] = b.flat, b.grad
    for mname in ("backbone_encoder", "seg_decoder"):
        for n, v in getattr(eng, mname, torch.nn.Module()).named_buffers():
            out[f"{mname}.{n}"] = v
    return out


def calls(dev):
    """-> (name, thunk) pairs; a thunk returns a dict of named tensors."""
    from adaptersis_amd import config
    from adaptersis_amd.utils import weights as W
    img, tgt = (t.to(dev) for t in W.synthetic_batch(BATCH, SIZE))
    for name, build, kw in CASES:
        train_py_flow = build is seg_engine and kw.get("head") != "mla"
        for with_taps in (True, False) if train_py_flow else (True,):
            eng = []                                # built by the first step's thunk, so that a refused keyword is that call's result

            def step(eng=eng, build=build, kw=kw, with_taps=with_taps):
                if not eng:
                    eng.append(build(dev, **kw))
                taps = {} if with_taps else None
                return outputs(eng[0], eng[0].train_step(img, tgt, taps), taps)
            for i in (1, 2):
                yield f"{name}{'' if with_taps else ' no taps'} step {i}", step
    for dual in (True, False):                      # step 2 is the first on the dual-stream trunk: step 1 fills the operand caches

        def second_logits(dual=dual):
            keep, config.dual_stream = config.dual_stream, dual
            try:
                eng, taps = seg_engine(dev), {}
                eng.train_step(img, tgt)
                eng.train_step(img, tgt, taps)
                return {"logits": taps["logits"]}
            finally:
                config.dual_stream = keep
        yield f"reference_exact feature dual_stream={int(dual)} step 2", second_logits


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose adaptersis_amd package (with its built library) runs the list")
    ap.add_argument("--only", default="", help="run only the calls whose name contains this")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    dev = torch.device("cuda:0")
    n = 0
    for name, thunk in calls(dev):
        if a.only not in name:
            continue
        try:
            out = thunk()
        except ValueError as e:     # a refused argument is a result too: the other tree must refuse the same call
            print(f"ValueError  {name}: {e}", flush=True)
            continue
        for k, t in out.items():
            print(f"{hashlib.sha256(t.detach().float().cpu().numpy().tobytes()).hexdigest()}  {name} [{k}] {t.dtype} {list(t.shape)}", flush=True)
            n += 1
    print(f"# {n} outputs", file=sys.stderr)
