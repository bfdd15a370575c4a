"""GPU: the weight average — the two kernels of csrc/ema.hip element by element against float64, the skip they take over from
the optimizers' on-device guard, ``optim.EMA`` behind ``optim.SGD`` / ``optim.AdamW``, a tiny ``SegEngine(ema_decay=...)`` with
its ``ema_weights()`` swap (also with LoRA), and the ``ema`` checkpoint entry through the training script and
``adaptersis_amd.predict``.

The one-step bound.  With ``w`` the device's own ``rec[0]``, ``e`` and ``p`` the fp32 inputs and ``ref = e + w (p - e)`` in
float64, the kernel rounds twice: the difference (relative 2^-24, which reaches the result scaled by w) and the fused
multiply-add (relative 2^-24 of the result, or half the smallest subnormal):

    |got - ref| <= 1.01 * 2^-24 * (|w (p - e)| + |ref|) + 2^-149
"""
import os

import numpy as np
import pytest
import torch

from adaptersis_amd import ops, optim
from adaptersis_amd.dinov2.models import vision_transformer as vits
from adaptersis_amd.utils import weights as W

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
TINY = 2.0 ** -149
BIG_N = 2 * ops.EMA_GRID_CAP * ops.EMA_TILE + 5       # the capped grid walks its tiles more than twice, plus an n % 4 tail
LENGTHS = [1, 3, 4, 5, 1023, 4097, BIG_N]


def _spread(n, seed):
    """fp32 [n], signs mixed, magnitudes spread over the binades 2^-20 .. 2^20"""
    g = torch.Generator().manual_seed(seed)
    mant = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
    expo = torch.randint(-20, 21, (n,), generator=g).double()
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (sign * mant * torch.pow(torch.tensor(2.0, dtype=torch.float64), expo)).float()


def _pair(n, seed):
    """(e, p): unrelated magnitudes, every 5th p within a few ulps .. 1e-3 of e (cancellation), every 7th p == e"""
    e, p = _spread(n, seed), _spread(n, seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    near = e * (1.0 + (torch.rand(n, generator=g) - 0.5) * 2e-3)
    idx = torch.arange(n)
    p = torch.where(idx % 5 == 0, near, p)
    p = torch.where(idx % 7 == 0, e, p)
    return e, p


def _check_step(got, e, p, w, what):
    """the one-step bound of the module docstring; got / e / p fp32 CPU tensors, w the float32 weight as a Python float"""
    e64, p64 = e.double(), p.double()
    delta = w * (p64 - e64)
    ref = e64 + delta
    lim = 1.01 * U * (delta.abs() + ref.abs()) + TINY
    err = (got.double() - ref).abs()
    worst = float((err / lim).max())
    print(f"{what}: max err / limit {worst:.3f}")
    assert bool((err <= lim).all()), what
    same = p == e
    assert torch.equal(got[same], e[same]), what        # p == e: the average does not move, exactly


def _state(dev):
    return torch.zeros(1, device=dev, dtype=torch.int32), torch.zeros(2, device=dev, dtype=torch.float32)


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", LENGTHS)
def test_update_against_float64(dev, n, offset):
    """offset 1: both bases one float off a 16-byte boundary (the scalar path); 7.0 sentinels around both buffers stay"""
    e, p = _pair(n, 100 + n % 1000)
    ebuf = torch.full((offset + n + 4,), 7.0)
    pbuf = torch.full((offset + n + 4,), 7.0)
    ebuf[offset:offset + n] = e
    pbuf[offset:offset + n] = p
    ed, pd = ebuf.to(dev), pbuf.to(dev)
    assert ed.data_ptr() % 16 == 0 and pd.data_ptr() % 16 == 0
    state, rec = _state(dev)
    ops.ema_prepare(None, state, rec, 0.9, True)
    ops.ema_update(ed[offset:offset + n], pd[offset:offset + n], rec)
    w = float(rec[0].item())
    assert int(state.item()) == 1 and float(rec[1].item()) == 1.0
    assert w == float(np.float32(1.0 - optim.ema_decay_at(1, 0.9, True)))
    got = ed.cpu()
    assert torch.equal(pd.cpu(), pbuf)                                           # p is read only
    assert bool((got[:offset] == 7.0).all()) and bool((got[offset + n:] == 7.0).all())
    _check_step(got[offset:offset + n], e, p, w, f"ema_update n={n} offset={offset}")


def test_update_with_one_misaligned_base(dev):
    """only one of the two bases off the boundary still takes the scalar path"""
    n = 1023
    e, p = _pair(n, 7)
    state, rec = _state(dev)
    ops.ema_prepare(None, state, rec, 0.75, False)
    for eo, po in ((1, 0), (0, 1)):
        ed = torch.cat([torch.zeros(eo), e]).to(dev)
        pd = torch.cat([torch.zeros(po), p]).to(dev)
        ops.ema_update(ed[eo:], pd[po:], rec)
        _check_step(ed[eo:].cpu(), e, p, 0.25, f"ema_update offsets e={eo} p={po}")


@pytest.mark.parametrize("warmup", [True, False])
def test_prepare_writes_the_schedule_exactly(dev, warmup):
    decay = 0.9
    state, rec = _state(dev)
    for t in range(1, 21):
        ops.ema_prepare(None, state, rec, decay, warmup)        # guard None: every call applies
        assert int(state.item()) == t
        r = rec.cpu()
        assert float(r[1]) == 1.0
        assert float(r[0]) == float(np.float32(1.0 - optim.ema_decay_at(t, decay, warmup))), t


def test_skipped_step_leaves_the_average_alone(dev):
    n = 4097
    e, p = _pair(n, 11)
    ed, pd = e.to(dev), p.to(dev)
    state, rec = _state(dev)
    guard = torch.tensor([1, 0], device=dev, dtype=torch.int32)
    ops.ema_prepare(guard, state, rec, 0.9, True)
    ops.ema_update(ed, pd, rec)
    assert int(state.item()) == 0 and float(rec[1].item()) == 0.0
    assert torch.equal(ed.cpu(), e)
    guard[0] = 0
    ops.ema_prepare(guard, state, rec, 0.9, True)
    ops.ema_update(ed, pd, rec)
    assert int(state.item()) == 1 and float(rec[1].item()) == 1.0
    _check_step(ed.cpu(), e, p, float(rec[0].item()), "first applied update after a skipped one")
    before = ed.cpu()
    guard[0] = 1                                                    # skipped again: rec[0] of the last applied update stays, unused
    ops.ema_prepare(guard, state, rec, 0.9, True)
    ops.ema_update(ed, pd, rec)
    assert int(state.item()) == 1 and torch.equal(ed.cpu(), before)


def test_twenty_consecutive_updates(dev):
    """a fresh p every time, no host read between prepare and update: a wrong t, a wrong schedule or a record read before it is
    written shows as a step outside the one-step bound from the device's own previous average"""
    n, decay = 4097, 0.9
    e0, _ = _pair(n, 21)
    ed = e0.to(dev)
    state, rec = _state(dev)
    prev = e0
    for t in range(1, 21):
        p = _spread(n, 1000 + t)
        pd = p.to(dev)
        ops.ema_prepare(None, state, rec, decay, True)
        ops.ema_update(ed, pd, rec)
        w = float(rec[0].item())
        assert w == float(np.float32(1.0 - optim.ema_decay_at(t, decay, True))), t
        got = ed.cpu()
        _check_step(got, prev, p, w, f"update {t} of 20")
        prev = got
    assert int(state.item()) == 20


# ---- optimizer level ---------------------------------------------------------------------------------------------------------
def _buckets(dev):
    g = torch.Generator().manual_seed(5)
    mk = lambda *shape: torch.nn.Parameter(torch.randn(shape, generator=g).to(dev))
    return [optim.FlatBucket([("a.weight", mk(33, 7)), ("a.bias", mk(33))]), optim.FlatBucket([("b.weight", mk(130, 5))])]


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_average_follows_the_optimizers_skip(dev, kind):
    buckets = _buckets(dev)
    opt = optim.SGD(buckets, lr=0.1, momentum=0.9) if kind == "sgd" else optim.AdamW(buckets, lr=0.01)
    ema = optim.EMA(buckets, 0.5, warmup=False, guard=opt.guard)
    assert all(torch.equal(e, b.flat) for e, b in zip(ema.shadows, buckets)) and ema.updates == 0
    g = torch.Generator().manual_seed(6)
    for b in buckets:
        b.grad.copy_(torch.randn(b.numel, generator=g))
    buckets[1].grad[17] = float("inf")
    flat0 = [b.flat.clone() for b in buckets]
    shadow0 = [e.clone() for e in ema.shadows]
    opt.step()
    ema.update()
    assert opt.skipped_steps == 1 and ema.updates == 0
    assert all(torch.equal(b.flat, f) for b, f in zip(buckets, flat0))
    assert all(torch.equal(e, s) for e, s in zip(ema.shadows, shadow0))
    buckets[1].grad[17] = 0.25
    opt.step()
    ema.update()
    assert opt.skipped_steps == 1 and ema.updates == 1
    for b, e, s in zip(buckets, ema.shadows, shadow0):
        assert not torch.equal(b.flat, s) and not torch.equal(e, s)
        _check_step(e.cpu(), s.cpu(), b.flat.cpu(), 0.5, f"{kind}: first applied update")
    # state_dict round trip, validated before anything is written
    sd = ema.state_dict()
    other = optim.EMA(buckets, 0.5, warmup=False, guard=opt.guard)
    with pytest.raises(ValueError):
        other.load_state_dict({"updates": 1, "state": {0: sd["state"][0]}})
    with pytest.raises(ValueError):
        other.load_state_dict({"updates": 1, "state": {0: sd["state"][0], 1: {"shadow": sd["state"][1]["shadow"][:-4]}}})
    assert other.updates == 0 and all(torch.equal(e, b.flat) for e, b in zip(other.shadows, buckets))
    other.load_state_dict(sd)
    assert other.updates == 1 and all(torch.equal(a, b) for a, b in zip(other.shadows, ema.shadows))


def test_gradient_only_bucket_is_left_out(dev):
    p = torch.nn.Parameter(torch.ones(8, device=dev))
    q = torch.nn.Parameter(torch.ones(8, device=dev))
    stepped, grad_only = optim.FlatBucket([("p", p)]), optim.FlatBucket([("q", q)], momentum=False)
    ema = optim.EMA([grad_only, stepped], 0.9)
    assert ema.buckets == [stepped] and len(ema.shadows) == 1


# ---- engine ------------------------------------------------------------------------------------------------------------------
ARCH = "vit_tiny_test"


def _model(dev):
    D, depth, heads, ffn = W.VIT_CONFIGS[ARCH]
    sd = W.make_vit_state_dict(ARCH, layerscale="kernel")
    model = vits.__dict__[ARCH](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0)
    model.load_state_dict(sd)
    return model.to(dev), sd, D, heads


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
    return SegEngine(model, enc.to(dev), cv.to(dev), cn.to(dev), dec.to(dev), lr=0.05, mode="train_adapters", train_encoder=True, **kw)


def _batch(dev):
    img, tgt = W.synthetic_batch(3, 224)
    return img.to(dev), tgt.to(dev)


def test_engine_keeps_no_average_by_default(dev):
    eng = _seg_engine(dev)
    assert eng.ema is None
    with pytest.raises(ValueError, match="no average"):
        with eng.ema_weights():
            pass


@pytest.mark.parametrize("optimizer", ["sgd", "adamw"])
def test_engine_average_is_the_recursion_over_the_weights(dev, optimizer):
    eng = _seg_engine(dev, optimizer=optimizer, ema_decay=0.5, ema_warmup=False)
    buckets = eng.optimizer.buckets
    assert eng.ema.buckets == buckets and len(buckets) == 3         # decoder, adapters, encoder
    assert eng.ema.guard is eng.optimizer.guard
    assert all(torch.equal(e, b.flat) for e, b in zip(eng.ema.shadows, buckets))
    img, tgt = _batch(dev)
    prev = [e.cpu() for e in eng.ema.shadows]
    for k in range(1, 4):
        loss = float(eng.train_step(img, tgt))
        assert loss == loss and eng.optimizer.skipped_steps == 0
        for i, (b, e) in enumerate(zip(buckets, eng.ema.shadows)):
            got, flat = e.cpu(), b.flat.cpu()
            assert not torch.equal(flat, prev[i])
            _check_step(got, prev[i], flat, 0.5, f"{optimizer} step {k} bucket {i}")
            prev[i] = got
    assert eng.ema.updates == 3


def _eval(eng, img):
    """eval_logits as validation takes them: decoder in eval mode, restored afterwards"""
    was = eng.seg_decoder.training
    eng.seg_decoder.eval()
    try:
        return eng.eval_logits(img)
    finally:
        eng.seg_decoder.train(was)


def _bump(eng):
    """what the optimizers do after writing the flat buffers behind torch's back: the packed copies go stale"""
    for b in eng.optimizer.buckets:
        for p in b.params:
            p._asis_gen = getattr(p, "_asis_gen", 0) + 1


def _check_swap(eng, img, tgt):
    """``ema_weights()`` against the same engine with the average copied into its live parameters, bit for bit"""
    params = [p for b in eng.optimizer.buckets for p in b.params]
    ptrs = [p.data_ptr() for p in params]
    live = _eval(eng, img)
    with eng.ema_weights():
        assert all(p.data_ptr() != q for p, q in zip(params, ptrs))
        for _, p, view in eng.ema.named_shadows():
            assert p.data_ptr() == view.data_ptr()
        averaged = _eval(eng, img)
        with pytest.raises(RuntimeError, match="ema_weights"):
            eng.train_step(img, tgt)
    assert [p.data_ptr() for p in params] == ptrs
    assert torch.equal(_eval(eng, img), live)                                   # a stale pack of the average would show here
    assert not torch.equal(averaged, live)
    saved = [b.flat.clone() for b in eng.optimizer.buckets]
    for b, e in zip(eng.ema.buckets, eng.ema.shadows):
        b.flat.copy_(e)
    _bump(eng)
    copied = _eval(eng, img)
    for b, f in zip(eng.optimizer.buckets, saved):
        b.flat.copy_(f)
    _bump(eng)
    assert torch.equal(averaged, copied)
    assert torch.equal(_eval(eng, img), live)
    with pytest.raises(KeyError):                                               # the body raises: the views still come back
        with eng.ema_weights():
            assert params[0].data_ptr() != ptrs[0]
            raise KeyError("body")
    assert [p.data_ptr() for p in params] == ptrs and not eng.ema.swapped_in
    assert torch.equal(_eval(eng, img), live)
    with eng.ema_weights():                                                     # a second visit: the same average, rebuilt packs
        assert torch.equal(_eval(eng, img), averaged)
    return live, averaged


def test_ema_weights_swaps_the_average_in_and_out(dev):
    eng = _seg_engine(dev, ema_decay=0.5, ema_warmup=False)
    img, tgt = _batch(dev)
    for _ in range(2):
        eng.train_step(img, tgt)
    shadows = [e.clone() for e in eng.ema.shadows]
    flats = [b.flat.clone() for b in eng.optimizer.buckets]
    _check_swap(eng, img, tgt)
    assert all(torch.equal(a, b) for a, b in zip(shadows, eng.ema.shadows))     # evaluating writes neither the average ...
    assert all(torch.equal(a, b.flat) for a, b in zip(flats, eng.optimizer.buckets))   # ... nor the live weights
    eng.train_step(img, tgt)                                                    # and training goes on afterwards
    assert eng.ema.updates == 3


def test_ema_weights_merges_lora_from_the_averaged_factors(dev):
    from adaptersis_amd import lora
    eng = _seg_engine(dev, train_backbone=True, lora_rank=4, ema_decay=0.5, ema_warmup=False)
    assert eng.lora_bucket in eng.ema.buckets
    img, tgt = _batch(dev)
    for _ in range(2):
        eng.train_step(img, tgt)
    _check_swap(eng, img, tgt)
    # inside the context the merged weight is made of the averaged factors
    h, w = eng.lora.handles[0], eng.model.blocks[0].attn.qkv.weight
    shadow = {n: v for n, _, v in eng.ema.named_shadows()}
    A, Bq, Bv = (shadow[n].detach().double() for n in h.names())
    assert not torch.equal(Bq.float(), h.Bq.detach())
    base = w.detach().clone()
    want = lora.merged_weight(base.double(), A, Bq, Bv, h.scale)
    with eng.ema_weights():
        assert h.Bq.data_ptr() == shadow[h.names()[1]].data_ptr()
        with eng.lora.merged(eng.model):
            assert float((w.detach().double() - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max())
    assert torch.equal(w.detach(), base)


# ---- scripts -----------------------------------------------------------------------------------------------------------------
def test_ema_checkpoint_entry_through_train_and_predict(dev, tmp_path, capsys):
    from adaptersis_amd import predict as P
    from adaptersis_amd import train as T
    run, plain = tmp_path / "ema", tmp_path / "plain"
    common = ["--arch", ARCH, "--imsize", "224", "--batch_size_per_gpu", "4"]
    train_flags = ["--epochs", "1", "--lr", "0.05", "--data_path", "synthetic", "--train_adapters", "--train_encoder"]
    T._ENGINES.clear()
    T.train_seg(T.get_args_parser().parse_args(common + train_flags + ["--output_dir", str(run), "--ema_decay", "0.9",
                                                                       "--ema_validate_live"]))
    (eng_tr,) = T._ENGINES.values()
    T._ENGINES.clear()
    steps = eng_tr.optimizer._steps
    assert steps > 1 and eng_tr.ema.updates == steps - eng_tr.optimizer.skipped_steps
    ck = torch.load(os.path.join(run, "checkpoint.pth.tar"), map_location="cpu")
    assert set(ck["ema"]) == {"decay", "warmup", "updates", "state_dict", "cross_vit", "cross_cnn", "backbone_encoder"}
    assert ck["ema"]["decay"] == 0.9 and ck["ema"]["warmup"] is True and ck["ema"]["updates"] == eng_tr.ema.updates
    mods = {"state_dict": eng_tr.seg_decoder, "cross_vit": eng_tr.cross_vit, "cross_cnn": eng_tr.cross_cnn,
            "backbone_encoder": eng_tr.backbone_encoder}
    shadow = {id(p): v for _, p, v in eng_tr.ema.named_shadows()}
    for key, mod in mods.items():
        assert list(ck["ema"][key]) == list(ck[key]), key                       # the live entry's keys, "module." prefix included
        params = dict(mod.named_parameters())
        for n, v in mod.state_dict().items():
            got = ck["ema"][key]["module." + n]
            if n in params:                                                     # parameters from the average ...
                assert torch.equal(got, shadow[id(params[n])].cpu()), (key, n)
            else:                                                               # ... buffers from the live module
                assert torch.equal(got, v.cpu()), (key, n)
    assert any(not torch.equal(ck["ema"]["state_dict"][k], v) for k, v in ck["state_dict"].items())   # it is not the live entry
    log = open(os.path.join(run, "log.txt")).read()
    assert "test_live_acc1" in log and "test_acc1" in log
    # a resume restores the average and its count bit for bit (epoch 1 of 1 is done: nothing trains)
    T.train_seg(T.get_args_parser().parse_args(common + train_flags + ["--output_dir", str(run), "--ema_decay", "0.9"]))
    (eng_rs,) = T._ENGINES.values()
    T._ENGINES.clear()
    assert eng_rs.ema.updates == eng_tr.ema.updates
    assert all(torch.equal(a, b) for a, b in zip(eng_rs.ema.shadows, eng_tr.ema.shadows))
    assert all(torch.equal(a.flat, b.flat) for a, b in zip(eng_rs.optimizer.buckets, eng_tr.optimizer.buckets))
    # predict --ema: the masks engine.predict gives under ema_weights(), reproduced from the file
    eng = P.build_engine(P.get_args_parser().parse_args(common + ["--output_dir", str(run), "--input", "unused", "--ema"]))
    img, _ = W.synthetic_batch(3, 224)
    img = img.to(dev)
    with eng_tr.ema_weights():
        want = eng_tr.predict(img)
    assert torch.equal(eng.predict(img), want)
    eng_live = P.build_engine(P.get_args_parser().parse_args(common + ["--output_dir", str(run), "--input", "unused"]))
    assert torch.equal(eng_live.predict(img), eng_tr.predict(img))
    # a run without --ema_decay writes no entry, and predict --ema on it is an error, not the live weights
    T.train_seg(T.get_args_parser().parse_args(common + train_flags + ["--output_dir", str(plain)]))
    T._ENGINES.clear()
    ck_plain = torch.load(os.path.join(plain, "checkpoint.pth.tar"), map_location="cpu")
    assert "ema" not in ck_plain and set(ck_plain) == set(ck) - {"ema"}
    with pytest.raises(ValueError, match="holds no 'ema' entry"):
        P.build_engine(P.get_args_parser().parse_args(common + ["--output_dir", str(plain), "--input", "unused", "--ema"]))
    # resuming that checkpoint with the flag set starts the average from the restored live weights, and says so
    capsys.readouterr()
    T.train_seg(T.get_args_parser().parse_args(common + train_flags + ["--output_dir", str(plain), "--ema_decay", "0.9"]))
    (eng_new,) = T._ENGINES.values()
    T._ENGINES.clear()
    assert "the average starts from the restored live weights" in capsys.readouterr().out
    assert eng_new.ema.updates == 0 and all(torch.equal(e, b.flat) for e, b in zip(eng_new.ema.shadows, eng_new.ema.buckets))
    for key in ("state_dict", "cross_vit"):
        mod = {"state_dict": eng_new.seg_decoder, "cross_vit": eng_new.cross_vit}[key]
        for n, p in mod.named_parameters():
            assert torch.equal(p.detach().cpu(), ck_plain[key]["module." + n]), (key, n)
