/* C ABI of libasis_consist.so (adaptersis_amd/csrc/consist.hip), a library beside libasis_hip.so and libasis_distill.so: return
 * codes, error text (asis_last_error) and conventions are those of asis_hip.h; gfx950 only.
 *
 * The consistency term of teacher-student (mean-teacher) training: the distillation loss of asis_distill.h with a per-pixel
 * confidence gate, a per-sample weight and the count of the pixels the gate let through.  logits, teachers, hs, ws, flips, V, H, W,
 * C, temperature as there; N = B*H*W, per native pixel i = (b*H + y)*W + x of sample b:
 *   z, t_k, p, q, kd_i exactly as asis_distill.h defines them (align_corners=False samples, student and teachers through one code
 *     path, a mirrored map read through mirrored columns, q a true division by V, q_c log(q_c / p_c) as one logarithm of a ratio,
 *     the log-sum-exp of z / T where p_c underflows).  Against asis_distill_loss at threshold <= 0 the last bits may differ (the
 *     compiler contracts the bilinear blend per call site); the bound of both is the float64 value.
 *   conf_i = max_c q_c: the teacher's confidence AT THE SAME temperature T as the loss.  A gate on the T = 1 distribution is what a
 *     run at T = 1, the default, has; at T > 1 the mean distribution is flatter and a given threshold keeps fewer pixels.
 *   m_i = [conf_i >= threshold].  threshold <= 0 keeps every pixel; threshold > 1 or NaN is an argument error.
 *   w_b = sample_weight[b] (fp32 [B] on the device; NULL = every weight is 1).  The weights must be finite and >= 0: this is the
 *     caller's duty and is not checked on the device (a negative or NaN weight gives a loss and a dz of no meaning, no fault).
 *   loss (1 float) = T^2 (sum_i w_b m_i kd_i) / N: normalised by N, not by the kept count (the FixMatch convention; it is what
 *     keeps this one pass).  Summed in double in a fixed order (one partial per workgroup, then one workgroup).
 *   kept (1 int) = sum_i m_i [w_b > 0], summed the same way (integers in double: exact).
 *   dz fp32 [B,H,W,C] = grad_scale (T / N) w_b m_i (p_c - q_c), each step rounded once: ((p - q) * (T / N)) * grad_scale, then
 *     * w_b only where sample_weight is given.  p == q gives exactly 0, a power-of-two grad_scale scales the bits, a weight of 1.0
 *     gives the bits of sample_weight == NULL.
 *     accumulate == 0: dz is written everywhere; a dropped pixel (m_i = 0 or w_b = 0) gets zeros.
 *     accumulate != 0: dz += the term on the kept pixels (one fp32 add); a dropped pixel's dz is neither read nor written.
 *   A sample with w_b = 0 reads none of its maps.
 *   partial: 2 * asis_consist_nblk(N) doubles owned by the caller, 8-byte aligned (asis_consist_nblk is callable without a GPU;
 *     -1 for N < 1 or N >= 2^31).  asis_consist_tile(): pixels one workgroup handles per pass.
 *   No host sync, no float atomics; the result is bit-identical from call to call.  C <= 16, V <= 8, N < 2^31, temperature > 0. */
#ifndef ASIS_CONSIST_H
#define ASIS_CONSIST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int asis_consist_tile(void);
int asis_consist_nblk(int64_t N);
int asis_consist_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers, const int* hs,
                      const int* ws, const int* flips, int V, int H, int W, int C, float temperature, float threshold,
                      const float* sample_weight, float grad_scale, int accumulate, double* partial, float* loss, int* kept,
                      float* dz);
#ifdef __cplusplus
}
#endif
#endif
