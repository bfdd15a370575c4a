"""The bound scheme shared by the kernel-against-float64 tests (test_gpu_bn_bwd.py documents it, test_gpu_loss_kernels.py uses it
too): fp32 outputs err <= max(4 Y, U ulp32 max|ref|) with Y the error of torch's own float32 evaluation on the CPU; 16-bit
outputs add half an ulp of the type (hi) or of the pair (hi + lo), fp16 also half a subnormal ulp."""
import torch

ULP32 = 2.0 ** -23
U_ELEM, U_SUM = 4, 16
DT = [torch.float16, torch.bfloat16]
HALF = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
PAIR = {torch.float16: 2.0 ** -21, torch.bfloat16: 2.0 ** -15}
SUBN = {torch.float16: 2.0 ** -25, torch.bfloat16: 0.0}


def _gen(*key) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (1 << 31))
    return g


def _bound(f32: torch.Tensor, ref: torch.Tensor, ulps: int):
    yard = float((f32.double() - ref).abs().max())
    return max(4 * yard, ulps * ULP32 * float(ref.abs().max())), yard


def _err(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.detach().double().cpu() - ref).abs().max())
