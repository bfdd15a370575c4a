// Knowledge distillation: the KL divergence of the student's class distribution from the mean distribution of 1..8 teacher
// views, fused with the bilinear resize of every map like the losses of loss.hip, lovasz.hip and hardpixel.hip.  Built into
// libasis_distill.so (build.py SIDE_LIBS; ABI in include/asis_distill.h), beside libasis_hip.so, whose error plumbing it uses.
//
//     i = (b*H + y)*W + x the flat native pixel, N = B*H*W, T the temperature, V the number of teacher maps
//     z   = resize(student logits) at H x W              (tap_ac_false and blend_taps of bilinear_tap.h: the arithmetic of
//                                                         sample_logits_at.  Not its bits everywhere: the compiler fuses the
//                                                         blend into multiply-adds per call site, and against
//                                                         asis_resize_bilinear_fwd 9 % of the samples differ in the last bit)
//     t_k = resize(teacher map k) at H x W               (a mirrored map, flip[k], keeps taps and weights and mirrors the two column
//                                                         indices: the bits of the un-mirrored map.flip(2), as in predict.hip)
//     p = softmax(z * (1/T)),  q = (1/V) sum_k softmax(t_k * (1/T))        (views in list order; 1/T rounded to fp32 once)
//     kd_i = sum_c q_c (log q_c - log p_c)               (a term with q_c = 0 is 0)
//     loss = T^2 (sum_i kd_i) / N
//     dz[i][c] (=, or += with `accumulate`: one fp32 add) grad_scale (T / N) (p_c - q_c)
//
// A term is evaluated as q_c logf(q_c / p_c), one logarithm of a ratio: where the two distributions are close (a high temperature,
// a trained student) log q_c and log p_c agree in their leading digits, and the difference of two logarithms keeps their absolute
// rounding errors (measured: 40 ulp of the loss at T = 4 with three teacher maps), the logarithm of the ratio does not.  p_c = q_c
// gives exactly 0, so a student that equals its one teacher costs 0 and gets a gradient of exactly 0.  Where p_c underflows
// (below ST_TINY: a saturated student) under q_c > 0, log p_c comes from the log-sum-exp of the student's row and the term is
// q_c (logf(q_c) - log p_c): finite.
//
// One pass: nothing of size [B,H,W,C] exists but dz.  The maps are read through the caches (they are small), dz is written once (and
// read once when it is added into) with 16-byte accesses where C*4 is a multiple of 16 and dz is 16-byte aligned.  The kernel, its
// tiles and the fixed order of its sums are soft_target.h's, shared with consist.hip; this is its ungated instantiation.
#include "../../include/asis_distill.h"
#include "soft_target.h"

extern "C" int asis_distill_tile(void) { return ST_TILE; }

extern "C" int asis_distill_nblk(int64_t N) { return st_nblk("asis_distill_nblk", N); }

extern "C" int asis_distill_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers, const int* hs,
                                 const int* ws, const int* flips, int V, int H, int W, int C, float temperature, float grad_scale,
                                 int accumulate, double* partial, float* loss, float* dz) {
  return st_loss("asis_distill_loss", NoGate{}, stream, logits, B, h, w, teachers, hs, ws, flips, V, H, W, C, temperature, grad_scale,
                 accumulate, partial, loss, nullptr, dz);
}
