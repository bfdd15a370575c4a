"""GPU: backward kernels and module backward of the adapters (`train_adapters` mode) against autograd of the oracle."""
import pytest
import torch
import torch.nn.functional as F

from adaptersis_amd import ops
from adaptersis_amd.utils import weights as W
from oracle import ref_torch as O
from tests.conftest import rel_l2

pytestmark = pytest.mark.gpu
DT = torch.float16


@pytest.mark.parametrize("case", [(2, 50, 4, 16, [(6, 7), (3, 4), (2, 2)], 4), (1, 37, 8, 32, [(9, 5)], 4),
                                  (2, 20, 2, 24, [(4, 4), (3, 3)], 2)])
def test_msda_backward(dev, case):
    """d value, d offsets, d attention logits of the sampling core vs autograd through grid_sample + softmax."""
    B, Lq, M, Dh, shapes, P = case
    L, D = len(shapes), M * Dh
    Lin = sum(a * b for a, b in shapes)
    value = W.tensor(f"msb.v{case}", (B, Lin, D), 1.0).to(DT)
    off = W.tensor(f"msb.o{case}", (B, Lq, M, L, P, 2), 2.5)
    logit = W.tensor(f"msb.l{case}", (B, Lq, M, L * P), 1.0)
    ref = W.tensor(f"msb.r{case}", (Lq, 2), 0.5, 0.5)
    dout = W.tensor(f"msb.d{case}", (B, Lq, D), 1.0)
    sp = torch.tensor(shapes)
    # oracle autograd
    v_r = value.float().view(B, Lin, M, Dh).clone().requires_grad_(True)
    off_r, lg_r = off.clone().requires_grad_(True), logit.clone().requires_grad_(True)
    normalizer = torch.stack([sp[:, 1], sp[:, 0]], -1).float()
    loc = ref[None, :, None, None, None, :] + off_r / normalizer[None, None, None, :, None, :]
    aw = F.softmax(lg_r, -1).view(B, Lq, M, L, P)
    out = O.ms_deform_attn_core(v_r, sp, loc, aw)
    (out * dout).sum().backward()
    # HIP
    offaw = torch.cat([off.reshape(B * Lq, -1), logit.reshape(B * Lq, -1)], 1).contiguous().to(dev)
    starts = [0]
    for a, b in shapes[:-1]:
        starts.append(starts[-1] + a * b)
    sh = torch.tensor(shapes, dtype=torch.int32, device=dev)
    st = torch.tensor(starts, dtype=torch.int32, device=dev)
    fwd = ops.msda_fwd(value.to(dev), offaw, ref.to(dev), sh, st, B, Lq, M, L, P)
    assert rel_l2(fwd.view(B, Lq, D), out) < 2e-3
    n_off = M * L * P * 2
    # scatter kernels (fp32 throughout) / taps bucketed by pixel + 64-bit fixed-point sums (the default, round 4) / the dense
    # sampling matrix + 16-bit MFMA GEMMs of round 2
    dout_d = dout.reshape(B * Lq, D).contiguous().to(dev)
    for form in ("scatter", "sorted", "matrix"):
        old = ops.MSDA_SORTED
        ops.MSDA_SORTED = form == "sorted"
        try:
            dvalue, doffaw = ops.msda_bwd(value.to(dev), offaw, ref.to(dev), sh, st, dout_d, B, Lq, M, L, P, dense=form != "scatter")
            if form == "sorted":
                dv2, _ = ops.msda_bwd(value.to(dev), offaw, ref.to(dev), sh, st, dout_d, B, Lq, M, L, P, dense=True)
                assert torch.equal(dvalue, dv2), "sorted form is not reproducible run to run"
        finally:
            ops.MSDA_SORTED = old
        e = (rel_l2(dvalue.view(B, Lin, M, Dh), v_r.grad), rel_l2(doffaw[:, :n_off].reshape(off.shape), off_r.grad),
             rel_l2(doffaw[:, n_off:].reshape(logit.shape), lg_r.grad))
        print(case, form, "dvalue doff dlogit:", ["%.1e" % v for v in e])
        assert e[0] < (1e-3 if form != "scatter" and D % 64 == 0 else 1e-4) and max(e[1:]) < 1e-4, e


def test_msda_value_grad_sorted_at_the_adapter_geometry(dev):
    """the two MSDeformAttn geometries of the step at ViT-L width (CAViT: 1764 queries on the 73^2 / 36^2 / 18^2 pyramid; CACNN:
    6949 queries on the 42^2 map), two images: sorted form == dense-matrix form up to the matrix's 16-bit rounding, and bit for
    bit reproducible."""
    for Lq, shapes in ((1764, [(73, 73), (36, 36), (18, 18)]), (6949, [(42, 42)])):
        B, M, Dh, P = 2, 8, 128, 4
        L, D = len(shapes), M * Dh
        Lin = sum(a * b for a, b in shapes)
        value = W.tensor(f"msg.v{Lq}", (B, Lin, D), 1.0).to(DT).to(dev)
        off = W.tensor(f"msg.o{Lq}", (B * Lq, M * L * P * 2), 2.5)
        logit = W.tensor(f"msg.l{Lq}", (B * Lq, M * L * P), 1.0)
        offaw = torch.cat([off, logit], 1).contiguous().to(dev)
        g = torch.arange(Lq, dtype=torch.float32)
        ref = torch.stack([(g % 42 + 0.5) / 42 % 1.0, ((g // 42) % 42 + 0.5) / 42], -1).to(dev)
        dout = W.tensor(f"msg.d{Lq}", (B * Lq, D), 1e-3).to(dev)          # gradient-sized values
        starts, acc = [], 0
        for a, b in shapes:
            starts.append(acc); acc += a * b
        sh = torch.tensor(shapes, dtype=torch.int32, device=dev)
        st = torch.tensor(starts, dtype=torch.int32, device=dev)
        outs = {}
        for form in ("sorted", "sorted2", "matrix"):
            old = ops.MSDA_SORTED
            ops.MSDA_SORTED = form != "matrix"
            try:
                outs[form], doffaw = ops.msda_bwd(value, offaw, ref, sh, st, dout, B, Lq, M, L, P)
            finally:
                ops.MSDA_SORTED = old
        assert torch.equal(outs["sorted"], outs["sorted2"])
        e = rel_l2(outs["sorted"], outs["matrix"])
        print(f"MSDA d value, Lq {Lq}: sorted vs dense matrix rel-L2 {e:.2e}")
        assert e < 1e-3
        _check_doffaw_sample(value, offaw, ref, shapes, dout, doffaw, B, Lq, M, Dh, L, P)


def _check_doffaw_sample(value, offaw, ref, shapes, dout, doffaw, B, Lq, M, Dh, L, P, per_image=32):
    """d offsets / d logits at this geometry (D = 1024, M = 8: the xor-shuffle reduction of msda_bwd_kernel) against the float64
    restatement, element by element with the bounds of tests/test_gpu_msda_routes.py, on 64 rows: the first 32 queries of each
    image all of whose sampling coordinates lie 2^-8 px or more from a cell boundary (about one query in five), where the kernel's
    fp32 position and the reference choose the same cell."""
    from tests import msda_ref as R
    n = M * L * P * 2
    oc, rc = offaw.cpu(), ref.cpu()
    px, py = R._positions(rc, oc[:, :n].reshape(B, Lq, M, L, P, 2), shapes, torch.float64)
    p = torch.stack([px, py])
    clear = ((p - p.round()).abs() >= 2.0 ** -8).flatten(3).all(-1).all(0)          # [B, Lq]
    qsel = [torch.nonzero(clear[b]).flatten()[:per_image] for b in range(B)]
    assert all(len(q) == per_image for q in qsel)
    for b in range(B):       # one image at a time, its sampled queries as a problem of their own (rows are independent)
        rows = b * Lq + qsel[b]
        r = R.msda_reference(value[b:b + 1].cpu(), oc[rows], rc[qsel[b]], shapes, M, P, dout=dout.cpu()[rows])
        got = doffaw.cpu()[rows]
        R.assert_within(f"Lq {Lq} image {b} d off", got[:, :n], r["ref"]["doff"], R.tol_doff(r, Dh), "sampled row, (m,l,p,xy)")
        R.assert_within(f"Lq {Lq} image {b} d logit", got[:, n:], r["ref"]["dlogit"], R.tol_dlogit(r, Dh, L * P), "sampled row, (m,l,p)")


def test_dwconv_gelu_backward(dev):
    B, C = 2, 64
    grids = [(7, 9), (4, 5), (2, 3)]
    Ntok = sum(a * b for a, b in grids)
    x = W.tensor("dwb.x", (B, Ntok, C), 1.0)
    w = W.tensor("dwb.w", (C, 1, 3, 3), 0.4)
    b = W.tensor("dwb.b", (C,), 0.3)
    dy = W.tensor("dwb.dy", (B, Ntok, C), 1.0)
    xr, wr, br = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.gelu(O.dwconv(xr, {"p.dwconv.weight": wr, "p.dwconv.bias": br}, "p", grids))
    (y * dy).sum().backward()
    starts = [0]
    for a, bb in grids[:-1]:
        starts.append(starts[-1] + a * bb)
    sh = torch.tensor(grids, dtype=torch.int32, device=dev)
    st = torch.tensor(starts, dtype=torch.int32, device=dev)
    w9 = w.reshape(C, 9).t().contiguous().to(dev)
    dx, partial = ops.dwconv_gelu_bwd(x.to(dev), w9, b.to(dev), sh, st, dy.to(dev), DT)
    red = ops.reduce_rows(partial.view(partial.shape[0], 10 * C)).view(10, C)
    assert rel_l2(dx, xr.grad) < 1e-3
    assert rel_l2(red[:9].t().reshape(C, 1, 3, 3), wr.grad) < 1e-5
    assert rel_l2(red[9], br.grad) < 1e-5


def _geometry(H, Wd, shapes, dev):
    from adaptersis_amd.backbones.adapter_blocks import deform_inputs
    d1, d2 = deform_inputs(torch.zeros(1, 3, H, Wd), 14, shapes)
    g = {"ref1": d1[0][0, :, 0, :].contiguous().to(dev), "shapes1": d1[1].to(torch.int32).to(dev),
         "starts1": d1[2].to(torch.int32).to(dev), "ref2": d2[0][0, :, 0, :].contiguous().to(dev),
         "shapes2": d2[1].to(torch.int32).to(dev), "starts2": d2[2].to(torch.int32).to(dev)}
    return g, d1, d2


def _check(errs):
    """Everything that does not pass through d(sampling offsets) agrees to the 16-bit operand level.  The offset
    gradient is the derivative of a piecewise-bilinear interpolant: it jumps when a sampling point crosses a pixel
    boundary, and the offsets of the 16-bit forward differ from the fp32 oracle's by ~2e-3 px, so ~0.5 % of the points
    sit in another cell -> ~5 % relative difference on d offsets and on what is upstream of them (query LayerNorm, the
    query input).  The sampling kernel itself is exact on identical inputs (test_msda_backward: 1.5e-7)."""
    loose = ("sampling_offsets", "query_norm", "dx", "dc")
    for k, v in errs.items():
        assert v < (1e-1 if any(t in k for t in loose) else 5e-3), (k, v, errs)


def test_cavit_cacnn_module_backward(dev):
    """CAViT and CACNN (LayerNorms, MSDeformAttn with all four projections, ConvFFN with the depthwise conv, gamma)
    forward in training form + backward of every parameter and both inputs vs autograd of the oracle modules."""
    from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
    D, B, size = 128, 2, 224
    shapes = [(28, 28), (14, 14), (7, 7)]
    N, Lc = (size // 14) ** 2, sum(a * b for a, b in shapes)
    g, d1, d2 = _geometry(size, size, shapes, dev)
    csd, nsd = W.make_cavit_state_dict(D, mode="kernel"), W.make_cacnn_state_dict(D, mode="kernel")
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4)
    cv.load_state_dict(csd)
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25)
    cn.load_state_dict(nsd)
    cv, cn = cv.to(dev), cn.to(dev)
    x = W.tensor("adb.x", (B, N, D), 1.0)
    c = W.tensor("adb.c", (B, Lc, D), 1.0)
    dy1 = W.tensor("adb.dy1", (B, N, D), 1.0)
    dy2 = W.tensor("adb.dy2", (B, Lc, D), 1.0)
    S = 64.0
    # ---- CAViT
    ocs = {k: v.clone().requires_grad_(True) for k, v in csd.items()}
    xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    y_ref = O.cavit(xr, d1[0], cr, d1[1], ocs)
    (y_ref * dy1).sum().backward()
    y, saved = cv.forward16_train(x.view(B * N, D).to(dev), c.view(B * Lc, D).to(dev), g, B, N, Lc)
    assert rel_l2(y.view(B, N, D), y_ref) < 1e-3
    grads = {k: torch.zeros_like(p, dtype=torch.float32) for k, p in cv.named_parameters()}
    dx, dc = cv.backward16(saved, (dy1 * S).view(B * N, D).contiguous().to(dev), 1.0 / S, grads)
    errs = {k: rel_l2(grads[k], ocs[k].grad) for k in grads}
    errs["dx"], errs["dc"] = rel_l2(dx.view(B, N, D) / S, xr.grad), rel_l2(dc.view(B, Lc, D) / S, cr.grad)
    print("CAViT:", {k: "%.1e" % v for k, v in errs.items()})
    _check(errs)
    # ---- CACNN
    ons = {k: v.clone().requires_grad_(True) for k, v in nsd.items()}
    xr, cr = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
    z_ref = O.cacnn(cr, d2[0], xr, d2[1], shapes, ons)
    (z_ref * dy2).sum().backward()
    z, saved = cn.forward16_train(c.view(B * Lc, D).to(dev), x.view(B * N, D).to(dev), g, B, Lc, N, shapes)
    assert rel_l2(z.view(B, Lc, D), z_ref) < 1e-3
    grads = {k: torch.zeros_like(p, dtype=torch.float32) for k, p in cn.named_parameters()}
    dc, dx = cn.backward16(saved, (dy2 * S).view(B * Lc, D).contiguous().to(dev), 1.0 / S, grads)
    errs = {k: rel_l2(grads[k], ons[k].grad) for k in grads}
    errs["dx"], errs["dc"] = rel_l2(dx.view(B, N, D) / S, xr.grad), rel_l2(dc.view(B, Lc, D) / S, cr.grad)
    print("CACNN:", {k: "%.1e" % v for k, v in errs.items()})
    _check(errs)


@pytest.mark.parametrize("train_encoder", [False, True])
def test_engine_train_adapters_step_vs_oracle(dev, train_encoder):
    """`train_adapters` mode: the step of `train.py:268-436` with the autograd graph left intact (no `no_grad` around
    the adapter stream): gradients of every CAViT / CACNN parameter and of the decoder against autograd of the oracle,
    then one SGD step over both buckets."""
    from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
    from adaptersis_amd.backbones.decoders import FeatureDecoder
    from adaptersis_amd.backbones.encoders import FeatureEncoder
    from adaptersis_amd.backbones.engines import SegEngine
    from adaptersis_amd.dinov2.models import vision_transformer as vits
    arch, size, B = "vit_tiny_test", 224, 2
    D, depth, heads, ffn = W.VIT_CONFIGS[arch]
    feats = (128, 32, 16, 16, 8)
    sds = dict(vit=W.make_vit_state_dict(arch, layerscale="kernel"), enc=W.make_encoder_state_dict(D),
               cv=W.make_cavit_state_dict(D, mode="kernel"), cn=W.make_cacnn_state_dict(D, mode="kernel"),
               dec=W.make_feature_decoder_state_dict(D, 2, features=feats))
    model = vits.__dict__[arch](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0)
    model.load_state_dict(sds["vit"])
    enc = FeatureEncoder(embed_dim=D); enc.load_state_dict(sds["enc"])
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4); cv.load_state_dict(sds["cv"])
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25); cn.load_state_dict(sds["cn"])
    dec = FeatureDecoder(embed_dim=D, num_classes=2, features=list(feats)); dec.load_state_dict(sds["dec"])
    eng = SegEngine(model.to(dev).eval(), enc.to(dev), cv.to(dev), cn.to(dev), dec.to(dev), lr=0.05, mode="train_adapters",
                    train_encoder=train_encoder)
    img, tgt = W.synthetic_batch(B, size)
    # oracle with the graph intact
    ocv = {k: v.clone().requires_grad_(True) for k, v in sds["cv"].items()}
    ocn = {k: v.clone().requires_grad_(True) for k, v in sds["cn"].items()}
    odec = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k and "num_batches" not in k)
            for k, v in sds["dec"].items()}
    oenc = {k: v.clone().requires_grad_(train_encoder and v.is_floating_point() and "running" not in k)
            for k, v in sds["enc"].items()}
    ocat = O.adapter_forward(img, sds["vit"], oenc, ocv, ocn, heads, update_bn=not train_encoder)
    oloss = O.train_step_loss(ocat, tgt, odec, 2, update_bn=True)
    oloss.backward()
    taps = {}
    loss = eng.train_step(img.to(dev), tgt.to(dev), taps)
    assert abs(float(loss) - float(oloss)) < 1e-4
    aerr = {}
    for k, v in eng.adapter_bucket.views.items():
        mod, name = k.split(".", 1)
        ref = (ocv if mod == "cross_vit" else ocn)[name].grad
        if ref is not None and float(ref.norm()) > 0:
            aerr[k] = rel_l2(v, ref)
    worst = sorted(aerr.items(), key=lambda kv: -kv[1])[:5]
    print("train_adapters: adapter grads worst:", [(k, "%.1e" % v) for k, v in worst], "n =", len(aerr))
    # step-level bound (forward differences move ReLU branches in the decoder and sampling cells in the adapters)
    assert max(aerr.values()) < 2.5e-1, worst
    assert sorted(aerr.values())[len(aerr) // 2] < 5e-2
    derr = {k: rel_l2(v, odec[k].grad) for k, v in eng.bucket.views.items() if not k.endswith(".0.bias")}
    assert max(derr.values()) < 1e-1, derr
    # the last stage's CACNN output is unused downstream: its own last-call contribution is zero, earlier calls are not
    assert float(eng.adapter_bucket.views["cross_cnn.ffn.fc2.weight"].abs().sum()) > 0
    if train_encoder:
        eerr = {k: rel_l2(v, oenc[k[len("backbone_encoder."):]].grad) for k, v in eng.encoder_bucket.views.items()
                if oenc[k[len("backbone_encoder."):]].grad is not None and float(oenc[k[len("backbone_encoder."):]].grad.norm()) > 0}
        print("train_encoder: encoder grads max %.2e median %.2e (%d tensors)" %
              (max(eerr.values()), sorted(eerr.values())[len(eerr) // 2], len(eerr)))
        assert max(eerr.values()) < 2.5e-1 and sorted(eerr.values())[len(eerr) // 2] < 1e-1, eerr
    # every trainable bucket is optimised
    assert len(eng.optimizer.param_groups) == (3 if train_encoder else 2)
    p_after = dict(eng.cross_vit.named_parameters())["attn.value_proj.weight"].detach().cpu()
    assert not torch.equal(p_after, sds["cv"]["attn.value_proj.weight"])


def test_encoder_backward(dev):
    """FeatureEncoder (stem with MaxPool, three stride-2 conv stages, SyncBN in train mode, 1x1 projections) in training
    form + backward of every parameter against autograd of the oracle encoder."""
    from adaptersis_amd.backbones.encoders import FeatureEncoder
    D, B, size = 128, 2, 224
    sd = W.make_encoder_state_dict(D)
    enc = FeatureEncoder(embed_dim=D)
    enc.load_state_dict(sd)
    enc = enc.to(dev)
    img = W.synthetic_batch(B, size)[0]
    osd = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in sd.items()}
    c1, c2, c3, c4, shapes = O.feature_encoder(img, osd)
    c_ref = torch.cat([c2, c3, c4], 1)
    dc = W.tensor("encb.dc", tuple(c_ref.shape), 1.0)
    (c_ref * dc).sum().backward()
    c, shp, saved = enc.forward_tokens_train(img.to(dev), sync_bn=False)
    assert [tuple(s) for s in shp] == [tuple(s) for s in shapes]
    assert rel_l2(c, c_ref) < 1e-4
    S = 16.0
    grads = {k: torch.full_like(p, float("nan"), dtype=torch.float32) for k, p in enc.named_parameters()}
    enc.backward_tokens(saved, (dc * S).to(dev), 1.0 / S, grads, sync_bn=False)
    errs = {k: rel_l2(grads[k], osd[k].grad) for k in grads if osd[k].grad is not None and float(osd[k].grad.norm()) > 0}
    print("encoder grads:", {k: "%.1e" % v for k, v in errs.items()})
    assert float(grads["fc1.weight"].abs().sum()) == 0      # c1 is unused by the step
    assert set(errs) >= {"stem.0.weight", "stem.7.weight", "conv2.0.weight", "conv3.0.weight", "conv4.0.weight", "fc4.bias"}
    # ReLU / MaxPool branch flips on the small maps set the floor for everything upstream (tests/test_gpu_unet.py)
    assert max(errs.values()) < 5e-2, errs
    assert sorted(errs.values())[len(errs) // 2] < 1e-2
