"""LoRA on the config-4 stacking: ViT-L blocks (vit_large_d4) on segs = [(12, 1765), (12, 1764)], forward + backward three ways —
(i) full parameter gradients, (ii) input gradient only (``grads=None``), (iii) LoRA r = 16 on q / v — all arms interleaved in one
process after warm-up, device events around each pass; ms per block (median over the rounds) and the ratios (iii)/(i), (iii)/(ii).
Then the two kernels of csrc/lora.hip alone next to what the step would otherwise pay (``torch.matmul``; ``ops.wgrad`` on
contiguous copies, the copies timed) with their HBM byte counts over time, and the qkv / input-gradient GEMMs at K and K + 64.
    python scripts/bench_lora.py [--rounds 12] [--batch 12] [--rank 16]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from adaptersis_amd import config, lora, ops
from adaptersis_amd.dinov2.models import vision_transformer as vits
from adaptersis_amd.utils import weights as W

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=12)
ap.add_argument("--batch", type=int, default=12)
ap.add_argument("--rank", type=int, default=16)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_lora needs an MI355X: there is no CPU path")
dev = torch.device("cuda:0")
config.split_attn_out = True                      # what SegEngine(train_backbone=True) runs
arch = "vit_large_d4"
D, depth, heads, ffn = W.VIT_CONFIGS[arch]
model = vits.__dict__[arch](patch_size=14, img_size=518, init_values=1e-5, ffn_layer=ffn, block_chunks=0)
model.load_state_dict(W.make_vit_state_dict(arch, layerscale="kernel"))
model = model.to(dev)
B, r = args.batch, args.rank
segs = [(B, 1765), (B, 1764)]
R = sum(b * n for b, n in segs)
x = torch.randn((R, D), device=dev)
dres = torch.randn((R, D), device=dev) * 64.0
full = {f"blocks.{i}.{k}": torch.empty_like(p, dtype=torch.float32) for i, blk in enumerate(model.blocks) for k, p in blk.named_parameters()}
lo = lora.LoRA(model, r)
with torch.no_grad():
    for p in lo.parameters():
        p.copy_(torch.randn_like(p) * 0.02)
lgrads = {n: torch.empty_like(p) for n, p in lo.named_parameters()}
lora.LoRA.detach(model)
ARMS = ("full gradients", "input gradient only", f"LoRA r={r}")


def one_pass(arm):
    if arm == 2:
        lo.attach(model)
    grads = (full, None, lgrads)[arm]
    xx, saved = x, []
    for blk in model.blocks:
        xx, s = blk.forward_train_rows(xx, segs)
        saved.append(s)
    d = dres
    for i in range(depth - 1, -1, -1):
        d = model.blocks[i].backward(saved[i], d, 1.0 / 64.0, grads, f"blocks.{i}")
        saved[i] = None
    if arm == 2:
        lora.LoRA.detach(model)
    return d


def timed(f, reps=20):
    for _ in range(3):
        f()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        f()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


with torch.no_grad():
    for _ in range(2):
        for a in range(3):
            one_pass(a)
    torch.cuda.synchronize()
    times = [[] for _ in ARMS]
    for _ in range(args.rounds):
        for a in range(3):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            one_pass(a)
            e.record()
            torch.cuda.synchronize()
            times[a].append(s.elapsed_time(e) / depth)
    med = [statistics.median(t) for t in times]
    print(f"{arch} segs {segs} (R = {R}) fwd + bwd, {args.rounds} interleaved rounds, ms per block")
    for a, name in enumerate(ARMS):
        t = sorted(times[a])
        print(f"  ({'i' * (a + 1):>3}) {name:20s}: median {med[a]:7.3f}  min {t[0]:7.3f}  max {t[-1]:7.3f}", flush=True)
    print(f"  (iii)/(i) = {med[2] / med[0]:.3f}   (iii)/(ii) = {med[2] / med[1]:.3f}   (ii)/(i) = {med[1] / med[0]:.3f}", flush=True)

    # ---- the two kernels alone ------------------------------------------------------------------------------------------------
    dt = config.operand_dtype
    P = ops.LORA_PAD
    abuf = (torch.randn((R, D + P), device=dev) * 0.5).to(dt)
    dbuf = (torch.randn((R, 3 * D + P), device=dev) * 0.5).to(dt)
    xn_c, dqv_c = abuf[:, :D].contiguous(), torch.cat([dbuf[:, :D], dbuf[:, 2 * D:3 * D]], 1).contiguous()
    wd_f = (torch.randn((P, D), device=dev) * 0.05).to(dt)
    wd_b = (torch.randn((P, 2 * D), device=dev) * 0.05).to(dt)
    two = [(0, D), (2 * D, D)]
    u_c, du_c = abuf[:, D:].contiguous(), dbuf[:, 3 * D:].contiguous()
    print("kernels alone (us; HBM bytes = one read of the operands + one write of the result; TB/s; the guide's float4-copy rate is 6.29 TB/s)")

    def line(what, f, nbytes):
        us = timed(f)
        print(f"  {what:58s}: {us:8.1f} us  {nbytes / 1e6:7.1f} MB  {nbytes / us / 1e6:5.2f} TB/s", flush=True)
        return us
    b_dn = 2.0 * (R * D + P * D + R * P)
    line("lora_down fwd  u = xn A^T            [R,1024] -> [R,64]", lambda: ops.lora_down(abuf, [(0, D)], wd_f, out=abuf[:, D:]), b_dn)
    line("  torch.matmul(xn, Wd^T) (contiguous xn)", lambda: torch.matmul(xn_c, wd_f.t()), b_dn)
    b_dn2 = 2.0 * (R * 2 * D + P * 2 * D + R * P)
    line("lora_down bwd  du = [dQ|dV] Wd^T     [R,2x1024] -> [R,64]", lambda: ops.lora_down(dbuf, two, wd_b, out=dbuf[:, 3 * D:]), b_dn2)
    line("  torch.matmul([dQ|dV], Wd^T) on a contiguous copy", lambda: torch.matmul(dqv_c, wd_b.t()), b_dn2)
    line("  the copy [dQ|dV] -> contiguous", lambda: torch.cat([dbuf[:, :D], dbuf[:, 2 * D:3 * D]], 1), 8.0 * R * D)
    b_wa = 2.0 * R * (D + P) + 4.0 * P * D
    line("lora_wgrad dA = du^T xn              -> [64,1024]", lambda: ops.lora_wgrad(dbuf[:, 3 * D:], abuf, [(0, D)], 1.0), b_wa)
    line("  ops.wgrad on contiguous copies", lambda: ops.wgrad(du_c.view(1, R, 1, P), xn_c.view(1, R, 1, D), P, 1, 1, 1, 0, 1.0), b_wa)
    line("  the copies (xn, du) -> contiguous", lambda: (abuf[:, :D].contiguous(), dbuf[:, 3 * D:].contiguous()), 4.0 * R * (D + P))
    line("  torch.matmul(du^T, xn) (contiguous)", lambda: torch.matmul(du_c.t(), xn_c), b_wa)
    b_wg = 2.0 * R * (2 * D + P) + 4.0 * P * 2 * D
    line("lora_wgrad G  = u^T [dQ|dV]          -> [64,2048]", lambda: ops.lora_wgrad(abuf[:, D:], dbuf, two, 1.0), b_wg)
    line("  ops.wgrad on contiguous copies", lambda: ops.wgrad(u_c.view(1, R, 1, P), dqv_c.view(1, R, 1, 2 * D), P, 1, 1, 1, 0, 1.0), b_wg)
    line("  torch.matmul(u^T, [dQ|dV]) (contiguous)", lambda: torch.matmul(u_c.t(), dqv_c), b_wg)

    # ---- what the 64 extra K columns cost the GEMMs that run anyway ---------------------------------------------------------------
    wq = (torch.randn((3 * D, D + P), device=dev) * 0.02).to(dt)
    wq_c = wq[:, :D].contiguous()
    wb = (torch.randn((D, 3 * D + P), device=dev) * 0.02).to(dt)
    wb_c = wb[:, :3 * D].contiguous()
    dq_c = dbuf[:, :3 * D].contiguous()
    print("GEMMs at K and K + 64 (us), forms:", ops._shape_plan(R, 3 * D, D), ops._shape_plan(R, 3 * D, D + P),
          ops._shape_plan(R, D, 3 * D, out_f32=True), ops._shape_plan(R, D, 3 * D + P, out_f32=True))
    pairs = (("qkv GEMM            K 1024", lambda: ops.gemm(xn_c, wq_c), "K 1088", lambda: ops.gemm(abuf, wq)),
             ("input-gradient GEMM K 3072", lambda: ops.gemm(dq_c, wb_c, out_f32=True), "K 3136", lambda: ops.gemm(dbuf, wb, out_f32=True)))
    for n0, f0, n1, f1 in pairs:
        t0, t1 = [], []
        for _ in range(5):                       # alternating
            t0.append(timed(f0, 10)); t1.append(timed(f1, 10))
        m0, m1 = statistics.median(t0), statistics.median(t1)
        print(f"  {n0}: {m0:8.1f} us   {n1}: {m1:8.1f} us   +{m1 - m0:6.1f} us ({(m1 / m0 - 1) * 100:+.1f} %)", flush=True)
