"""GPU: the precise_level-2 forward of the ViT block (``Block._forward_rows_precise``: split-precision hi + lo operands, or
the 16-bit part + one block-scaled fp8 pass on the MX form) against the oracle block in float64, one token batch at a time,
over the branches it has: Mlp (erf-GELU in the fc1 epilogue or ``gelu_split``) and SwiGLU (gate in the w12 epilogue or
``swiglu(split=...)``; hidden 688 keeps w3 off the MX form, hidden 1024 puts it on), every ``config.precise_parts`` subset of
the A/B table plus {fc2} and {qkv}, one / two / three stacked token batches (folded q in one launch / per-batch pre-scaled
kernel) and a batch below the MX form's 256 rows, float16 and bfloat16 (three-part form only).

Errors are rel-L2 against float64; BOUND holds, per (dtype, parts), twice the largest value measured on the MI355X over the
three FFN geometries and the segment lists, on one MI355X:

    dtype parts         mlp256    sg256     sg384     bound
    f16   all           5.06e-06     -      4.90e-06   1.0e-05
    f16   qkv,proj,fc1  3.17e-05  1.91e-05  1.67e-05   6.3e-05
    f16   proj,fc1,fc2  7.63e-06     -      7.42e-06   1.5e-05
    f16   proj,fc1      3.22e-05  1.99e-05  1.76e-05   6.4e-05
    f16   qkv,proj      4.48e-05  3.04e-05  2.91e-05   8.9e-05
    f16   proj          4.51e-05  3.09e-05  2.96e-05   9.0e-05
    f16   fc2           3.33e-05     -      2.59e-05   6.6e-05
    f16   qkv           4.54e-05  3.12e-05  2.99e-05   9.0e-05
    f16   qkv,fc1,fc2   8.52e-06     -      8.86e-06   1.7e-05
    f16   qkv,proj,fc2  3.21e-05     -      2.43e-05   6.4e-05
    f16   level 0       4.57e-05  3.17e-05  3.05e-05   9.1e-05
    bf16  all           3.61e-05     -      3.63e-05   7.2e-05
    bf16  qkv,proj,fc1  2.51e-04  1.52e-04  1.33e-04   5.0e-04
    bf16  proj,fc1,fc2  5.71e-05     -      5.97e-05   1.1e-04
    bf16  proj,fc1      2.55e-04  1.59e-04  1.41e-04   5.0e-04
    bf16  qkv,proj      3.58e-04  2.44e-04  2.31e-04   7.1e-04
    bf16  proj          3.60e-04  2.47e-04  2.37e-04   7.2e-04
    bf16  fc2           2.66e-04     -      2.06e-04   5.3e-04
    bf16  qkv           3.62e-04  2.50e-04  2.38e-04   7.2e-04
    bf16  qkv,fc1,fc2   6.62e-05     -      6.70e-05   1.3e-04
    bf16  qkv,proj,fc2  2.56e-04     -      1.93e-04   5.1e-04
    bf16  level 0       3.65e-04  2.54e-04  2.44e-04   7.2e-04

(max over the segment lists; "-": w3 at hidden 688 has K % 64 != 0 and cannot run split, see
test_precise_refuses_what_it_cannot_split.)  Measured ratios behind the other constants: level 0 / level 2 on all four parts
6.2 .. 12.5 (L0_GAIN 4); all four but one / all four 1.42 .. 1.89 (DROP_ONE 1.25); adding layers to ``parts`` changed the error
by a factor of at most 0.996 (MONOTONE 1.1).
"""
import contextlib

import pytest
import torch

from adaptersis_amd import config, ops
from adaptersis_amd.dinov2.layers import blocks as BL
from adaptersis_amd.utils import weights as W
from oracle import ref_torch as O
from tests.conftest import rel_l2

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
FFNS = {"mlp256": (256, 4, BL.Mlp), "sg256": (256, 4, BL.SwiGLUFFNFused), "sg384": (384, 6, BL.SwiGLUFFNFused)}
SEGS = {"one": [(1, 257)], "two": [(2, 301), (1, 300)], "three": [(1, 197), (2, 145), (1, 257)], "small": [(1, 197)]}
PARTS = {"all": ("qkv", "proj", "fc1", "fc2"), "qkv,proj,fc1": ("qkv", "proj", "fc1"), "proj,fc1,fc2": ("proj", "fc1", "fc2"),
         "proj,fc1": ("proj", "fc1"), "qkv,proj": ("qkv", "proj"), "proj": ("proj",), "fc2": ("fc2",), "qkv": ("qkv",),
         # all four but one: each layer's residual must take its share of the error away (DROP_ONE)
         "qkv,fc1,fc2": ("qkv", "fc1", "fc2"), "qkv,proj,fc2": ("qkv", "proj", "fc2")}
# (smaller, larger): adding layers to ``parts`` must not raise the error by more than MONOTONE
SUBSETS = [("proj", "proj,fc1"), ("proj", "qkv,proj"), ("qkv", "qkv,proj"), ("fc2", "proj,fc1,fc2"), ("proj,fc1", "qkv,proj,fc1"),
           ("proj,fc1", "proj,fc1,fc2"), ("qkv,proj", "qkv,proj,fc1"), ("qkv,proj,fc1", "all"), ("proj,fc1,fc2", "all")]

BOUND = {
    ("f16", "all"): 1.0e-05, ("f16", "qkv,proj,fc1"): 6.3e-05, ("f16", "proj,fc1,fc2"): 1.5e-05, ("f16", "proj,fc1"): 6.4e-05,
    ("f16", "qkv,proj"): 8.9e-05, ("f16", "proj"): 9.0e-05, ("f16", "fc2"): 6.6e-05, ("f16", "qkv"): 9.0e-05,
    ("f16", "qkv,fc1,fc2"): 1.7e-05, ("f16", "qkv,proj,fc2"): 6.4e-05,
    ("bf16", "all"): 7.2e-05, ("bf16", "qkv,proj,fc1"): 5.0e-04, ("bf16", "proj,fc1,fc2"): 1.1e-04, ("bf16", "proj,fc1"): 5.0e-04,
    ("bf16", "qkv,proj"): 7.1e-04, ("bf16", "proj"): 7.2e-04, ("bf16", "fc2"): 5.3e-04, ("bf16", "qkv"): 7.2e-04,
    ("bf16", "qkv,fc1,fc2"): 1.3e-04, ("bf16", "qkv,proj,fc2"): 5.1e-04,
}
LEVEL0_BOUND = {"f16": 9.1e-05, "bf16": 7.2e-04}
L0_GAIN, DROP_ONE, MONOTONE = 4.0, 1.25, 1.1
FORMS_TOL = {"f16": 2e-4, "bf16": 2e-4}     # measured: at most 1.55e-05 (f16) and 1.30e-04 (bf16: folded / unfolded q)

_KNOBS = ("precise_level", "precise_parts", "operand_dtype", "mx_dense", "fold_attn_scale", "split_attn_out",
          "precise_attention")


@contextlib.contextmanager
def knobs(level=2, parts="all", dt="f16", mx_dense=True, fold_attn_scale=True, fold_q=True, attn_mx_out=True, swiglu_fused=True):
    """every process-wide switch the precise path reads, set for one call and restored after it"""
    keep = tuple(getattr(config, k) for k in _KNOBS) + (BL._PRECISE_FOLD_Q, BL._ATTN_MX_OUT, ops._SWIGLU_FUSED)
    try:
        config.precise_level = level
        config.precise_parts = frozenset(PARTS[parts])
        config.set_operand_dtype(DTYPES[dt])
        config.mx_dense, config.fold_attn_scale = mx_dense, fold_attn_scale
        config.split_attn_out = config.precise_attention = False
        BL._PRECISE_FOLD_Q, BL._ATTN_MX_OUT, ops._SWIGLU_FUSED = fold_q, attn_mx_out, swiglu_fused
        yield
    finally:
        for k, v in zip(_KNOBS, keep[:len(_KNOBS)]):
            setattr(config, k, v)
        BL._PRECISE_FOLD_Q, BL._ATTN_MX_OUT, ops._SWIGLU_FUSED = keep[len(_KNOBS):]


_BLOCKS, _CASES = {}, {}


def block(name, dev):
    """a block with a non-trivial LayerScale and LayerNorm affine (test_gpu_vit.py's SwiGLU case), one per FFN geometry"""
    if name not in _BLOCKS:
        D, H, ffn = FFNS[name]
        torch.manual_seed(11)
        blk = BL.Block(D, H, qkv_bias=True, init_values=0.3, ffn_layer=ffn).to(dev).eval()
        with torch.no_grad():
            for p_ in blk.parameters():
                if p_.dim() == 1 and p_.numel() == D and float(p_.std()) == 0:
                    p_.add_(0.1 * torch.randn_like(p_))
        _BLOCKS[name] = blk
    return _BLOCKS[name]


def case(name, segname, dev):
    """(block, fp32 input on the device, float64 oracle output): the oracle runs once per (FFN, segments)"""
    key = (name, segname)
    if key not in _CASES:
        D, H, _ = FFNS[name]
        blk = block(name, dev)
        segs = SEGS[segname]
        R = sum(b * n for b, n in segs)
        x = W.tensor(f"bprec.x.{name}.{segname}", (R, D), 1.0)
        sd = {"b." + k: v.detach().cpu().double() for k, v in blk.state_dict().items()}
        xd, refs, r0 = x.double(), [], 0
        with torch.no_grad():
            for b, n in segs:
                refs.append(O.block(xd[r0:r0 + b * n].view(b, n, D), sd, "b", H).reshape(b * n, D))
                r0 += b * n
        _CASES[key] = (blk, x.to(dev), torch.cat(refs))
    return _CASES[key]


def run(name, segname, dev, segs=None, **kw):
    blk, x, _ = case(name, segname, dev)
    with knobs(**kw):
        return blk.forward_rows(x, SEGS[segname] if segs is None else segs)


def err(name, segname, dev, **kw):
    return rel_l2(run(name, segname, dev, **kw), case(name, segname, dev)[2])


def matrix(name, dt, dev):
    """{(parts | "level0", segments): rel-L2 against the float64 oracle} of one FFN geometry and dtype"""
    out = {}
    for segname in SEGS:
        out[("level0", segname)] = err(name, segname, dev, level=0, dt=dt)
        if segname == "small":
            continue
        for parts in PARTS:
            if runs(name, parts):
                out[(parts, segname)] = err(name, segname, dev, parts=parts, dt=dt)
    return out


def runs(name, parts):
    """the split GEMM forms need K % 64 == 0: w3 at hidden 688 cannot run split (test_precise_refuses_what_it_cannot_split)"""
    D, _, ffn = FFNS[name]
    return not ("fc2" in PARTS[parts] and ffn is not BL.Mlp and W.swiglu_hidden(D) % 64)


def forms(name, dt, dev):
    """launch forms that must agree, for the same parts: [(what, y, y_other, bit-identical promised)]"""
    out = []
    sg = FFNS[name][2] is not BL.Mlp
    f16 = dt == "f16"
    for segname in ("two", "three"):
        for parts in ("proj,fc1", "proj"):
            y = run(name, segname, dev, parts=parts, dt=dt)
            out.append((f"fold q / unfolded q {parts} {segname}", y, run(name, segname, dev, parts=parts, dt=dt, fold_q=False), False))
            out.append((f"fold_attn_scale off == _PRECISE_FOLD_Q off {parts} {segname}",
                        run(name, segname, dev, parts=parts, dt=dt, fold_attn_scale=False),
                        run(name, segname, dev, parts=parts, dt=dt, fold_q=False), True))
    if f16:     # bfloat16 never takes the MX form (config.mx_dense_on)
        for parts in [p for p in ("all", "proj,fc1", "qkv,proj") if runs(name, p)]:
            out.append((f"MX / three-part {parts}", run(name, "two", dev, parts=parts, dt=dt),
                        run(name, "two", dev, parts=parts, dt=dt, mx_dense=False), False))
        for segname in ("one", "two"):
            out.append((f"attention writes o_lo as MX on / off {segname}", run(name, segname, dev, parts="proj,fc1", dt=dt),
                        run(name, segname, dev, parts="proj,fc1", dt=dt, attn_mx_out=False), False))
    if sg:
        for parts in ("proj,fc1", "proj"):
            # on the MX split form the epilogue and the two-kernel form share one main loop: bit-identical
            # (bfloat16: a split fc1 never takes the epilogue, one code path)
            same = "fc1" in PARTS[parts]
            out.append((f"SwiGLU epilogue / swiglu kernel {parts}", run(name, "two", dev, parts=parts, dt=dt),
                        run(name, "two", dev, parts=parts, dt=dt, swiglu_fused=False), same))
    for parts in ("all", "proj,fc1", "proj,fc1,fc2"):
        if not runs(name, parts):
            continue
        stacked = run(name, "three", dev, parts=parts, dt=dt)
        blk, x, _ = case(name, "three", dev)
        r0 = 0
        with knobs(parts=parts, dt=dt):
            for b, n in SEGS["three"]:
                if b * n >= 256:    # (1, 197) alone is below the split forms' 256 rows: test_precise_refuses_...
                    alone = blk.forward_rows(x[r0:r0 + b * n].contiguous(), [(b, n)])
                    out.append((f"three batches stacked / {(b, n)} alone {parts}", stacked[r0:r0 + b * n], alone, False))
                r0 += b * n
    return out


def gelu_epilogue(dt, dev):
    """the `ge` branch's fc1 GEMM (erf-GELU in the epilogue, one 16-bit output) on the split / MX / plain operand forms against
    the same GEMM written in fp32 followed by the GELU kernel: [(what, h, h_two_kernel)]"""
    blk, x, _ = case("mlp256", "two", dev)
    m = blk.mlp
    out = []
    forms_ = [("split MX", True, True), ("split three-part", True, False), ("plain", False, False)]
    for what, split, mx in forms_:
        if mx and dt != "f16":
            continue
        with knobs(dt=dt, mx_dense=mx):
            assert blk._mx_ok(m, "fc1", m.fc1, x.shape[0]) == mx
            b = m._f32("fc1_b", m.fc1.bias)
            if split:
                hi, lo, pl = blk._ln_split("n2", blk.norm2, x, mx)
                h = blk._split_lin(m, "fc1", m.fc1, hi, lo, pl, bias_n=b, act=ops.ACT_GELU)
                pre = blk._split_lin(m, "fc1", m.fc1, hi, lo, pl, bias_n=b, out_f32=True)
            else:
                xn = ops.layernorm(x, blk._f32("n2w", blk.norm2.weight), blk._f32("n2b", blk.norm2.bias), blk.norm2.eps,
                                   config.operand_dtype)
                w = m._w16("fc1", m.fc1.weight)
                h = ops.gemm(xn, w, bias_n=b, act=ops.ACT_GELU)
                pre = ops.gemm(xn, w, bias_n=b, out_f32=True)
            out.append((what, h, ops.gelu_split(pre, config.operand_dtype, split=False)[0]))
    return out


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(FFNS))
def test_precise_forward_vs_float64_oracle(dev, name, dt):
    """1. every (parts, segments) cell within BOUND[(dtype, parts)]; 2. the lo halves are consumed: level 2 on all four parts
    beats level 0 by L0_GAIN, taking any one layer out of all four raises the error by DROP_ONE, and adding layers to
    ``parts`` never raises it by more than MONOTONE"""
    m = matrix(name, dt, dev)
    print(name, dt, {f"{p}|{s}": "%.2e" % v for (p, s), v in m.items()})
    for (parts, segname), e in m.items():
        bound = LEVEL0_BOUND[dt] if parts == "level0" else BOUND[(dt, parts)]
        assert e < bound, (parts, segname, e, bound)
    for segname in ("one", "two", "three"):
        if ("all", segname) not in m:
            continue
        e_all = m[("all", segname)]
        assert m[("level0", segname)] > L0_GAIN * e_all, segname
        for minus_one in ("proj,fc1,fc2", "qkv,fc1,fc2", "qkv,proj,fc2", "qkv,proj,fc1"):
            assert m[(minus_one, segname)] > DROP_ONE * e_all, (minus_one, segname)
        for smaller, larger in SUBSETS:
            if (smaller, segname) in m and (larger, segname) in m:
                assert m[(larger, segname)] < MONOTONE * m[(smaller, segname)], (smaller, larger, segname)


def test_precise_bounds_are_no_looser_than_level0():
    for (dt, parts), b in BOUND.items():
        assert b <= (5e-4 if dt == "f16" else LEVEL0_BOUND["bf16"]), (dt, parts, b)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("name", list(FFNS))
def test_precise_launch_forms_agree(dev, name, dt):
    """3. folded / unfolded q, MX / three-part, attention-written MX o_lo on / off, SwiGLU epilogue / two kernels, three batches
    stacked / alone: within FORMS_TOL of each other, bit-identical where the code runs one main loop either way"""
    for what, a, b, same in forms(name, dt, dev):
        e = rel_l2(a, b)
        print(name, dt, what, "%.2e" % e, bool(torch.equal(a, b)))
        if same:
            assert torch.equal(a, b), what
        assert e < FORMS_TOL[dt], (what, e)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_precise_gelu_epilogue_is_the_two_kernel_form(dev, dt):
    """the Mlp ``ge`` branch: erf-GELU in the fc1 GEMM's epilogue on split / MX / plain operands writes exactly what the fp32
    GEMM followed by the GELU kernel writes"""
    for what, h, h2 in gelu_epilogue(dt, dev):
        assert torch.equal(h, h2), what


@pytest.mark.parametrize("dt", list(DTYPES))
def test_precise_refuses_what_it_cannot_split(dev, dt):
    """no silent fall-back: fewer than 256 rows (the split GEMM forms are the large-tile ones), and w3 at hidden 688 (K % 64
    != 0), raise instead of running some other arithmetic; level 0 runs both"""
    assert err("mlp256", "small", dev, level=0, dt=dt) < LEVEL0_BOUND[dt]
    for parts in ("proj", "qkv", "fc2", "all"):
        with pytest.raises(ValueError, match="large-tile path"):
            run("mlp256", "small", dev, parts=parts, dt=dt)
    for parts in ("fc2", "proj,fc1,fc2"):
        assert not runs("sg256", parts)
        with pytest.raises(ValueError, match="large-tile path"):
            run("sg256", "two", dev, parts=parts, dt=dt)
