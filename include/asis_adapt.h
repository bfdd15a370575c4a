/* C ABI of libasis_adapt.so (adaptersis_amd/csrc/adapt.hip), a library beside libasis_hip.so, libasis_consist.so and
 * libasis_mix.so: return codes, error text (asis_last_error) and conventions are those of asis_hip.h; gfx950 only.
 *
 * Class-adaptive confidence thresholds for the consistency term (self-adaptive thresholding, FreeMatch, Wang et al. 2023): the
 * gate of asis_consist.h with one threshold per class, the statistics of the teacher's maps the thresholds follow, and their update.
 *
 * asis_adapt_consist_loss / asis_adapt_mix_consist_loss: asis_consist_loss / asis_mix_consist_loss (asis_consist.h, asis_mix.h) with
 *   `const float* class_threshold` (fp32 [C] on the device) in place of `float threshold`.  With q the teacher's mean distribution
 *   at pixel i (with mixing: the mixed q):
 *     a_i = argmax_c q_c, the lowest index among equal values;  conf_i = q_{a_i};  m_i = [conf_i >= class_threshold[a_i]].
 *   A class_threshold[c] <= 0 keeps every pixel of class c, a value above 1 (or NaN) drops them all; neither is an error.
 *   Everything else (weights, kept, the normalisation by N, dz and `accumulate`, the scratch of 2 * asis_adapt_nblk(N) doubles,
 *   asis_adapt_tile) is as there.  class_threshold filled with t gives the bits of threshold = t.
 *
 * asis_adapt_stats: over the pixels i of the samples with w_b > 0 (sample_weight[b], fp32 [B] on the device; NULL = every sample),
 *   each with weight 1 whatever the size of w_b, from the teacher's maps as asis_consist_loss reads them (resampling, flips,
 *   temperature, q a true division by V):
 *     sums[c] = S_c = sum_i q_i[c] (c < C),  sums[C] = S_conf = sum_i max_c q_i[c],  sums[C + 1] = cnt = the number of such pixels.
 *   sums: float64 [C + 2] on the device, 8-byte aligned.  partial: (C + 2) * asis_adapt_stats_nblk(N) doubles owned by the caller,
 *   8-byte aligned (asis_adapt_stats_nblk is callable without a GPU; -1 for N < 1 or N >= 2^31).  A sample with w_b <= 0 reads none
 *   of its maps.  Summed in double in a fixed order (per thread, per workgroup, then the partials in index order): no atomics, the
 *   result is bit-identical from call to call.  No host sync.
 *
 * asis_adapt_update: state float64 [C + 2] = tau, n_updates, ptilde[C] (the caller starts it at tau = 1/C, n_updates = 0,
 *   ptilde_c = 1/C); with cnt = sums[C + 1] > 0, in double, every step rounded once:
 *     tau <- momentum tau + (1 - momentum) S_conf / cnt,   ptilde_c <- momentum ptilde_c + (1 - momentum) S_c / cnt,  n_updates += 1,
 *     thr[c] = fp32(tau * ptilde_c / max_c ptilde_c)        (fp32 [C] on the device)
 *   With cnt == 0 neither state nor thr is written.  0 <= momentum < 1.  One workgroup, no host sync.
 *
 * C <= 16, V <= 8, N = B*H*W < 2^31, temperature > 0. */
#ifndef ASIS_ADAPT_H
#define ASIS_ADAPT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int asis_adapt_tile(void);
int asis_adapt_nblk(int64_t N);
int asis_adapt_stats_nblk(int64_t N);
int asis_adapt_consist_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers, const int* hs,
                            const int* ws, const int* flips, int V, int H, int W, int C, float temperature,
                            const float* class_threshold, const float* sample_weight, float grad_scale, int accumulate,
                            double* partial, float* loss, int* kept, float* dz);
int asis_adapt_mix_consist_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers, const int* hs,
                                const int* ws, const int* flips, int V, int H, int W, int C, float temperature,
                                const float* class_threshold, const float* sample_weight, const uint8_t* sel, const int* donor,
                                float grad_scale, int accumulate, double* partial, float* loss, int* kept, float* dz);
int asis_adapt_stats(void* stream, int B, const float* const* teachers, const int* hs, const int* ws, const int* flips, int V, int H,
                     int W, int C, float temperature, const float* sample_weight, double* partial, double* sums);
int asis_adapt_update(void* stream, const double* sums, double* state, float* thr, int C, double momentum);
#ifdef __cplusplus
}
#endif
#endif
