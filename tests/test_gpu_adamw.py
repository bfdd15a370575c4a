"""GPU: the fused AdamW (csrc/adamw.hip, optim.AdamW) against ``torch.optim.AdamW`` behind ``torch.nn.utils.clip_grad_norm_`` in
float64 on the CPU, over per-group tensors cut from the same flat data (their param groups carry the table's lr and decay).

Bound (tests/bound_helpers.py): with Y the error of torch's own float32 AdamW + clip on the CPU against float64 over the same steps,
p, exp_avg and exp_avg_sq are within max(4 Y, U_ELEM ulp32 max|ref|), the gradient norm within max(4 Y, U_SUM ulp32 |ref|).

Sizes: one workgroup of adamw_step covers 2048 elements in a single pass (256 lanes x 2 quads), one of grad_sumsq 4096 (4 quads); both
grids are capped at 2048 workgroups: above 2048 x 2048 elements a workgroup of adamw_step walks a contiguous range of several
passes, above 2048 x 4096 the grid-stride loop of grad_sumsq starts."""
import copy
import functools
import io

import pytest
import torch

from adaptersis_amd import optim
from tests.bound_helpers import U_ELEM, U_SUM, _bound, _err, _gen

pytestmark = pytest.mark.gpu

BETAS, EPS = (0.9, 0.999), 1e-8
STEP_PASS, SUMSQ_PASS, GRID_CAP = 2048, 4096, 2048
BIG = GRID_CAP * SUMSQ_PASS + SUMSQ_PASS + STEP_PASS + 4      # 33.6 MB per array: both loops take several passes, the paired and the single tail run
SIZES = [4, 8, STEP_PASS - 4, STEP_PASS + 4, SUMSQ_PASS - 4, SUMSQ_PASS + 4, 2 * SUMSQ_PASS + 4, BIG]
LRS = (1e-3, 7e-4, 2e-3)                                        # three steps with a changing learning rate
TABLE3 = [(1.0, 0.05), (0.5, 0.0), (0.25, 0.1)]                 # three groups, distinct lr_scale and decay


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def codes3(n4: int) -> torch.Tensor:
    """group 0 = quad 0, group 1 = quads 1 .. k - 1 with k odd, group 2 = the rest: boundaries at quad 1 and at an odd quad index"""
    k = (n4 // 2) | 1
    c = torch.full((n4,), 2, dtype=torch.uint8)
    c[1:k] = 1
    c[0] = 0
    return c


def _runs(codes: torch.Tensor):
    c = codes.to(torch.int16)
    b = [0, *(torch.nonzero(c[1:] != c[:-1]).flatten() + 1).tolist(), c.numel()]
    return [(b[i], b[i + 1], int(c[b[i]])) for i in range(len(b) - 1)]


def reference(buckets, grads, lrs, dtype, max_norm, state0=None, t0=0):
    """torch.optim.AdamW + clip_grad_norm_ on the CPU in ``dtype``.  buckets: [(p0 fp32 [n], codes uint8 [n / 4], table)];
    grads[step][bucket]: fp32, unscaled; state0: [(exp_avg, exp_avg_sq)] per bucket with t0 steps behind them.
    -> ([(p, m, v)] per bucket as flat tensors, [norm per step])"""
    pieces = []
    for bi, (p0, codes, table) in enumerate(buckets):
        for q0, q1, c in _runs(codes):
            pieces.append((bi, 4 * q0, 4 * q1, _f32(table[c][0]), _f32(table[c][1]),
                           torch.nn.Parameter(p0[4 * q0:4 * q1].to(dtype).clone())))
    opt = torch.optim.AdamW([{"params": [pc[5]], "lr": 0.0, "weight_decay": pc[4]} for pc in pieces], lr=0.0, betas=BETAS, eps=EPS)
    if state0 is not None:
        for bi, e0, e1, _, _, par in pieces:
            opt.state[par] = {"step": torch.tensor(float(t0)), "exp_avg": state0[bi][0][e0:e1].to(dtype).clone(),
                              "exp_avg_sq": state0[bi][1][e0:e1].to(dtype).clone()}
    norms = []
    for lr, gs in zip(lrs, grads):
        for grp, (bi, e0, e1, scale, _, par) in zip(opt.param_groups, pieces):
            grp["lr"] = lr * scale
            par.grad = gs[bi][e0:e1].to(dtype).clone()
        norms.append(float(torch.nn.utils.clip_grad_norm_([pc[5] for pc in pieces], max_norm if max_norm else float("inf"))))
        opt.step()
    out = []
    for bi in range(len(buckets)):
        mine = [pc[5] for pc in pieces if pc[0] == bi]
        out.append((torch.cat([p.detach() for p in mine]), torch.cat([opt.state[p]["exp_avg"] for p in mine]),
                    torch.cat([opt.state[p]["exp_avg_sq"] for p in mine])))
    return out, norms


def device_opt(buckets, dev, max_norm):
    """optim.AdamW over one flat bucket per entry, with the entry's quad codes and group table in place of the ones the
    constructor derives from parameter names (the kernels see nothing else of them)"""
    fbs = [optim.FlatBucket([("w", torch.nn.Parameter(p0.to(dev)))]) for p0, _, _ in buckets]
    opt = optim.AdamW(fbs, lr=LRS[0], betas=BETAS, eps=EPS, weight_decay=0.0, clip_grad=max_norm)
    for i, (_, codes, table) in enumerate(buckets):
        opt.codes[i] = codes.to(dev)
        opt.lr_scale[i] = torch.tensor([t[0] for t in table], dtype=torch.float32, device=dev)
        opt.weight_decay[i] = torch.tensor([t[1] for t in table], dtype=torch.float32, device=dev)
        opt.param_groups[i]["group_table"] = [tuple(t) for t in table]
    return opt, fbs


def device_run(buckets, grads, lrs, dev, max_norm, inv_scale=1.0):
    opt, fbs = device_opt(buckets, dev, max_norm)
    norms = []
    for lr, gs in zip(lrs, grads):
        for g, fb, x in zip(opt.param_groups, fbs, gs):
            g["lr"] = lr
            fb.grad.copy_(x if inv_scale == 1.0 else x / inv_scale)
        opt.step(inv_scale)
        norms.append(opt.record[3].clone())
    return opt, fbs, norms


def check(tag, fbs, opt, norms, r64, r32):
    (ref, nref), (f32, n32) = r64, r32
    for bi, fb in enumerate(fbs):
        for what, got, k in (("p", fb.flat, 0), ("exp_avg", fb.momentum, 1), ("exp_avg_sq", opt.exp_avg_sq[bi], 2)):
            bound, yard = _bound(f32[bi][k], ref[bi][k], U_ELEM)
            err = _err(got, ref[bi][k])
            print(f"{tag} bucket {bi} {what}: err {err:.3e}  Y {yard:.3e}  bound {bound:.3e}")
            assert err <= bound, (tag, bi, what, err, bound)
    for s, (got, a, b) in enumerate(zip(norms, nref, n32)):
        bound, yard = _bound(torch.tensor(b), torch.tensor(a, dtype=torch.float64), U_SUM)
        err = abs(float(got) - a)
        print(f"{tag} step {s} norm {a:.6e}: err {err:.3e}  Y {yard:.3e}  bound {bound:.3e}")
        assert err <= bound, (tag, s, err, bound)


@functools.lru_cache(maxsize=None)
def case(*ns):
    """inputs of one run over buckets of ``ns`` elements, made once: ([(p0, codes, table)], grads[step][bucket])"""
    buckets = tuple((torch.randn(n, generator=_gen(n, 1)), codes3(n // 4), TABLE3) for n in ns)
    grads = tuple(tuple(torch.randn(n, generator=_gen(n, 2, s)) for n in ns) for s in range(len(LRS)))
    return buckets, grads


@functools.lru_cache(maxsize=None)
def refs(ns, max_norm):
    buckets, grads = case(*ns)
    return reference(buckets, grads, LRS, torch.float64, max_norm), reference(buckets, grads, LRS, torch.float32, max_norm)


@pytest.mark.parametrize("n", SIZES)
def test_three_steps_match_float64_at_every_size(dev, n):
    buckets, grads = case(n)
    assert len(set(buckets[0][1].tolist())) == min(3, n // 4)
    opt, fbs, norms = device_run(buckets, grads, LRS, dev, None)
    assert opt.step_count == 3 and opt.skipped_steps == 0
    check(f"n={n}", fbs, opt, norms, *refs((n,), None))


def _norm0(ns) -> float:
    _, grads = case(*ns)
    return float(torch.cat([g.double() for g in grads[0]]).norm())


@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["active", "inactive"])
def test_clipping_over_two_buckets_sharing_one_norm(dev, factor):
    ns = (SUMSQ_PASS + 4, 1028)                               # different lengths, both with three groups
    max_norm = factor * _norm0(ns)                            # half (active) or twice (inactive) the reference's norm: never near 1
    buckets, grads = case(*ns)
    opt, fbs, norms = device_run(buckets, grads, LRS, dev, max_norm)
    r64, r32 = refs(ns, max_norm)
    for s, a in enumerate(r64[1]):                            # float64 norm of BOTH buckets together
        both = float(torch.cat([g.double() for g in grads[s]]).norm())
        assert abs(a - both) <= 1e-12 * both
        coef = min(1.0, max_norm / (a + 1e-6))
        assert (coef < 0.6) if factor < 1 else (coef == 1.0)
    check(f"clip x{factor}", fbs, opt, norms, r64, r32)
    assert abs(opt.last_grad_norm - r64[1][-1]) <= _bound(torch.tensor(r32[1][-1]), torch.tensor(r64[1][-1], dtype=torch.float64), U_SUM)[0]


def test_inv_scale_unscales_gradient_and_norm(dev):
    """gradients pre-multiplied by 64 and inv_scale = 1/64: the unscaled run, within the same bound (clipping active, so a
    norm taken on the scaled gradients would show)"""
    ns = (SUMSQ_PASS + 4, 1028)
    max_norm = 0.5 * _norm0(ns)
    buckets, grads = case(*ns)
    opt, fbs, norms = device_run(buckets, grads, LRS, dev, max_norm, inv_scale=1.0 / 64.0)
    check("inv_scale 1/64", fbs, opt, norms, *refs(ns, max_norm))


def _clone_opt(opt, fbs, dev, max_norm):
    """a second optimizer over copies of the buckets, in the same state (through state_dict, as a checkpoint would)"""
    buckets = [(fb.flat.cpu(), c.cpu(), g["group_table"]) for fb, c, g in zip(fbs, opt.codes, opt.param_groups)]
    opt2, fbs2 = device_opt(buckets, dev, max_norm)
    f = io.BytesIO()
    torch.save(opt.state_dict(), f)
    f.seek(0)
    opt2.load_state_dict(torch.load(f, map_location="cpu"))
    return opt2, fbs2


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_non_finite_gradient_skips_the_step_exactly(dev, bad):
    ns = (SUMSQ_PASS + 4, 1028)
    buckets, grads = case(*ns)
    opt, fbs, _ = device_run(buckets, grads[:1], LRS[:1], dev, 1.0)       # one clean step: moments and step count are non-trivial
    twin, tfbs = _clone_opt(opt, fbs, dev, 1.0)
    before = [(fb.flat.clone(), fb.momentum.clone(), v.clone()) for fb, v in zip(fbs, opt.exp_avg_sq)]
    norm_before = opt.last_grad_norm
    for fb, g in zip(fbs, grads[1]):
        fb.grad.copy_(g)
    fbs[1].grad[-1] = bad                                                  # last element of the second bucket
    opt.step()
    for (p, m, v), fb, vv in zip(before, fbs, opt.exp_avg_sq):
        assert torch.equal(p, fb.flat) and torch.equal(m, fb.momentum) and torch.equal(v, vv)
    assert opt.step_count == 1 and opt.skipped_steps == 1 and opt.last_grad_norm == norm_before
    # the next clean step = a clean step from a copy of the untouched state, bit for bit
    for o, bs in ((opt, fbs), (twin, tfbs)):
        for g, fb, x in zip(o.param_groups, bs, grads[2]):
            g["lr"] = LRS[2]
            fb.grad.copy_(x)
        o.step()
    for fb, tb, v, tv, (p0, _, _) in zip(fbs, tfbs, opt.exp_avg_sq, twin.exp_avg_sq, before):
        assert torch.equal(fb.flat, tb.flat) and torch.equal(fb.momentum, tb.momentum) and torch.equal(v, tv)
        assert not torch.equal(fb.flat, p0)                                  # ... and it did move
    assert opt.step_count == twin.step_count == 2 and opt.skipped_steps == 1 and twin.skipped_steps == 0
    assert opt.last_grad_norm == twin.last_grad_norm != norm_before


@pytest.mark.parametrize("ns", [(2 * SUMSQ_PASS + 4, 1028), (BIG,)], ids=["two-buckets", "grid-stride"])
def test_same_inputs_twice_give_the_same_bits(dev, ns):
    buckets, grads = case(*ns)
    max_norm = 0.5 * _norm0(ns)
    a, afb, an = device_run(buckets, grads, LRS, dev, max_norm)
    b, bfb, bn = device_run(buckets, grads, LRS, dev, max_norm)
    for x, y, v, w in zip(afb, bfb, a.exp_avg_sq, b.exp_avg_sq):
        assert torch.equal(x.flat, y.flat) and torch.equal(x.momentum, y.momentum) and torch.equal(v, w)
    assert all(torch.equal(x, y) for x, y in zip(an, bn)) and torch.equal(a.record, b.record)


# ---- engine wiring ----------------------------------------------------------------------------------------------------------------
def _engine(dev, **kw):
    """the smallest geometry tests/test_gpu_train_script.py builds (vit_tiny_test, decoder widths 128-32-16-16-8), adapters trained"""
    from adaptersis_amd.backbones.adapter_blocks import CACNN, CAViT
    from adaptersis_amd.backbones.decoders import FeatureDecoder
    from adaptersis_amd.backbones.encoders import FeatureEncoder
    from adaptersis_amd.backbones.engines import SegEngine
    from adaptersis_amd.dinov2.models import vision_transformer as vits
    from adaptersis_amd.utils import weights as W
    arch, feats = "vit_tiny_test", (128, 32, 16, 16, 8)
    D, depth, heads, ffn = W.VIT_CONFIGS[arch]
    model = vits.__dict__[arch](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0)
    model.load_state_dict(W.make_vit_state_dict(arch, layerscale="kernel"))
    enc = FeatureEncoder(embed_dim=D); enc.load_state_dict(W.make_encoder_state_dict(D))
    cv = CAViT(dim=D, n_levels=3, num_heads=8, init_values=0.0, n_points=4); cv.load_state_dict(W.make_cavit_state_dict(D, mode="kernel"))
    cn = CACNN(dim=D, n_levels=1, num_heads=8, n_points=4, with_cffn=True, cffn_ratio=0.25)
    cn.load_state_dict(W.make_cacnn_state_dict(D, mode="kernel"))
    dec = FeatureDecoder(embed_dim=D, num_classes=2, features=list(feats)); dec.load_state_dict(W.make_feature_decoder_state_dict(D, 2, features=feats))
    return SegEngine(model.to(dev).eval(), enc.to(dev), cv.to(dev), cn.to(dev), dec.to(dev), mode="train_adapters", **kw)


def _snapshot(opt):
    return [(b.flat.cpu().clone(), b.momentum.cpu().clone(), v.cpu().clone()) for b, v in zip(opt.buckets, opt.exp_avg_sq)]


def test_engine_trains_with_adamw_and_resumes_bit_for_bit(dev):
    from adaptersis_amd.utils import weights as W
    kw = dict(optimizer="adamw", lr=1e-3, weight_decay=0.05, clip_grad=0.05)
    eng = _engine(dev, **kw)
    opt = eng.optimizer
    assert isinstance(opt, optim.AdamW) and len(opt.buckets) == 2 and opt.buckets[1] is eng.adapter_bucket
    assert all(len(g["group_table"]) == 2 for g in opt.param_groups)           # decayed matrices / convs, undecayed 1-D parameters
    batches = [W.synthetic_batch(2, 224, seed=s) for s in range(3)]
    for s in range(2):
        before, t0 = _snapshot(opt), opt.step_count
        loss = eng.train_step(batches[s][0].to(dev), batches[s][1].to(dev))
        assert bool(torch.isfinite(loss)) and opt.step_count == t0 + 1
        grads = [[b.grad.cpu().clone() for b in opt.buckets]]                    # zero_grad is a no-op: still there
        buckets = [(p, c.cpu(), g["group_table"]) for (p, _, _), c, g in zip(before, opt.codes, opt.param_groups)]
        state0 = [(m, v) for _, m, v in before]
        r64 = reference(buckets, grads, [1e-3], torch.float64, 0.05, state0, t0)
        r32 = reference(buckets, grads, [1e-3], torch.float32, 0.05, state0, t0)
        print(f"engine step {s}: loss {float(loss):.5f} grad norm {r64[1][0]:.4e} clip coefficient {min(1.0, 0.05 / (r64[1][0] + 1e-6)):.4f}")
        check(f"engine step {s}", opt.buckets, opt, [opt.record[3].clone()], r64, r32)
    assert opt.skipped_steps == 0
    # checkpoint -> rebuild -> load -> one more step = the uninterrupted run
    f = io.BytesIO()
    torch.save({"optimizer": opt.state_dict(), **{k: copy.deepcopy(getattr(eng, k).state_dict())
                                                  for k in ("seg_decoder", "cross_vit", "cross_cnn", "backbone_encoder")}}, f)
    f.seek(0)
    ck = torch.load(f, map_location="cpu")
    eng.train_step(batches[2][0].to(dev), batches[2][1].to(dev))
    eng2 = _engine(dev, **kw)
    for k in ("seg_decoder", "cross_vit", "cross_cnn", "backbone_encoder"):
        getattr(eng2, k).load_state_dict(ck[k])
    eng2.optimizer.load_state_dict(ck["optimizer"])
    assert eng2.optimizer.step_count == 2
    eng2.train_step(batches[2][0].to(dev), batches[2][1].to(dev))
    for (p, m, v), (q, n, w) in zip(_snapshot(opt), _snapshot(eng2.optimizer)):
        assert torch.equal(p, q) and torch.equal(m, n) and torch.equal(v, w)
    assert eng2.optimizer.step_count == 3 and eng2.optimizer.last_grad_norm == opt.last_grad_norm


def test_engine_default_is_still_sgd_and_sgd_does_not_clip(dev):
    eng = _engine(dev)
    assert type(eng.optimizer) is optim.SGD and eng.optimizer.param_groups[0]["momentum"] == 0.99
    with pytest.raises(ValueError, match="adamw"):
        _engine(dev, clip_grad=1.0)
    with pytest.raises(ValueError):
        _engine(dev, optimizer="adamw", layer_decay=0.9)                       # no optimised backbone to decay over
