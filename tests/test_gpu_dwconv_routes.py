"""GPU: the ConvFFN depthwise 3x3 conv + erf GELU (dwconv_gelu_kernel, csrc/msda.hip) and its backward (dwconv_gelu_bwd_kernel,
dwconv_t_kernel, csrc/adapter_bwd.hip) against the float64 reference of tests/msda_ref.py, element by element, in both 16-bit
output types, over the thread layouts of the backward: C = 4 (256 row lanes per channel chunk), 16, 64, 1024 (one row lane), more
than 64 rows per block, a block that ends before `rows`, blocks that straddle images and levels, levels one pixel high or wide.

Bounds (u = 2^-24, u16 = 2^-11 fp16 / 2^-8 bf16, the most a round-to-nearest 16-bit store is off by; tests/msda_ref.py):
  out, dx        u16 |ref| + 2^-18 S_abs + 2^-20 P (+ 2^-25 for fp16, half the spacing of its subnormals)
                 at most 10 products on the path (64 u = 2^-18 with room to spare); the erf-GELU and its gradient are allotted 2^-20
                 absolute, far above the few ulp of erff / __expf and 2^9 under fp16's own rounding.  P = |pre| for out,
                 conv^T(|dy| (1 + |pre|), |w|) for dx.  S_abs of dx carries g = dy gelu'(pre) without cancellation AND what the
                 recomputed pre's own rounding does to it through gelu''.
  d w9, d bias   after ops.reduce_rows: (rows + nblk + 16) 2 u S_abs
tests/test_msda_ref_cpu.py holds the float32 evaluation of the reference inside these bounds, and a mirrored tap outside."""
import functools

import pytest
import torch

from adaptersis_amd import ops
from adaptersis_amd._lib import AsisError
from tests import msda_ref as R

pytestmark = pytest.mark.gpu
_ID = {torch.float16: "fp16", torch.bfloat16: "bf16"}
CASES = R.DW_CASES + [R.DW_BIG]


@functools.lru_cache(maxsize=None)
def _case(i):
    name, B, C, grids, bwd = CASES[i]
    c = R.make_dwconv_case(name, B, C, grids)
    return c, R.dwconv_reference(c["x"], c["w"], c["bias"], grids, c["dy"])


def _dev_inputs(c, dev):
    sh = torch.tensor(c["grids"], dtype=torch.int32, device=dev)
    st = torch.tensor(R.starts_of(c["grids"]), dtype=torch.int32, device=dev)
    w9 = c["w"].reshape(c["C"], 9).t().contiguous().to(dev)
    return c["x"].to(dev), w9, c["bias"].to(dev), sh, st


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_ID.get)
@pytest.mark.parametrize("i", range(len(CASES)), ids=[c[0] for c in CASES])
def test_dwconv_gelu_forward_and_backward(dev, i, dtype):
    c, r = _case(i)
    bwd = CASES[i][4]
    C, rows = c["C"], c["B"] * c["x"].shape[1]
    tag = f"{c['name']} {_ID[dtype]}"
    args = _dev_inputs(c, dev)
    out = ops.dwconv_gelu(*args, dtype)
    R.assert_within(f"{tag} out", out, r["ref"]["out"], R.tol_dw_out(r, dtype), "b, token, c")
    if not bwd:                       # C = 12: the forward takes any C % 4 == 0, the backward's thread layout needs C = 4 * 2^k
        with pytest.raises((ValueError, AsisError)):
            ops.dwconv_gelu_bwd(*args, c["dy"].to(dev), dtype)
        return
    dx, partial = ops.dwconv_gelu_bwd(*args, c["dy"].to(dev), dtype)
    nblk = R.dwconv_nblk(rows)
    assert partial.shape[0] == nblk
    red = ops.reduce_rows(partial.view(nblk, 10 * C)).view(10, C)
    R.assert_within(f"{tag} dx", dx, r["ref"]["dx"], R.tol_dw_out(r, dtype, "dx"), "b, token, c")
    R.assert_within(f"{tag} d w9", red[:9], r["ref"]["dw9"], R.tol_dw_param(r, "dw9", rows, nblk), "tap, c")
    R.assert_within(f"{tag} d bias", red[9], r["ref"]["dbias"], R.tol_dw_param(r, "dbias", rows, nblk), "c")
