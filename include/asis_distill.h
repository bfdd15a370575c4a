/* C ABI of libasis_distill.so (adaptersis_amd/csrc/distill.hip), a library beside libasis_hip.so: return codes, error text
 * (asis_last_error) and conventions are those of asis_hip.h; gfx950 only.
 *
 * Knowledge distillation, fused with the resize like the losses of asis_hip.h: the KL divergence of the student from the mean
 * distribution of V teacher maps, 1 <= V <= 8.  logits fp32 NHWC [B,h,w,C] (the student); teachers[k] fp32 NHWC
 * [B,hs[k],ws[k],C], flips[k] != 0: map k was predicted from the mirrored frame and is read through mirrored columns (bit for bit
 * the sample of the un-mirrored map, the contract of asis_predict_mask_views).  N = B*H*W, per native pixel i = (b*H + y)*W + x:
 *   z, t_k = the align_corners=False bilinear samples of the student and of teacher map k (the arithmetic of
 *     asis_resize_bilinear_fwd, student and teachers through one code path: a teacher map holding the student's values gives the
 *     student's bits; against asis_resize_bilinear_fwd itself the last bit may differ);
 *   p = softmax(z / T), q = (1/V) sum_k softmax(t_k / T) in list order (fp32; z / T as z * (1/T) with 1/T rounded once);
 *   kd_i = sum_c q_c log(q_c / p_c), a term with q_c = 0 is 0; where p_c underflows log p_c comes from the log-sum-exp of z / T
 *     (finite).  A student equal to its one teacher costs exactly 0 and gets dz = 0 exactly.
 *   loss (1 float) = T^2 (sum_i kd_i) / N, summed in double in a fixed order (one partial per workgroup, then one workgroup).
 *   dz fp32 [B,H,W,C] = grad_scale (T / N) (p_c - q_c) = grad_scale * d loss / d z; accumulate != 0 adds it into dz (one fp32 add).
 *   partial: asis_distill_nblk(N) doubles owned by the caller, 8-byte aligned (callable without a GPU; -1 for N < 1 or
 *     N >= 2^31).  asis_distill_tile(): pixels one workgroup handles per pass.
 *   No host sync, no float atomics; the result is bit-identical from call to call.  C <= 16, N < 2^31, temperature > 0. */
#ifndef ASIS_DISTILL_H
#define ASIS_DISTILL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int asis_distill_tile(void);
int asis_distill_nblk(int64_t N);
int asis_distill_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers, const int* hs,
                      const int* ws, const int* flips, int V, int H, int W, int C, float temperature, float grad_scale,
                      int accumulate, double* partial, float* loss, float* dz);
#ifdef __cplusplus
}
#endif
#endif
