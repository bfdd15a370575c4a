// The consistency term of teacher-student (mean-teacher) training: the distillation loss of distill.hip with a per-pixel
// confidence gate, a per-sample weight and the count of the pixels the gate let through.  Built into libasis_consist.so (build.py
// SIDE_LIBS; ABI in include/asis_consist.h), beside libasis_hip.so, whose error plumbing it uses.  The kernel is soft_target.h's,
// the one distill.hip launches, instantiated with its gate; z, t_k, p, q, kd_i, the tiles and the order of the sums are documented
// there and in distill.hip.  What the gate adds:
//
//     conf_i = max_c q_c,  m_i = [conf_i >= threshold],  w_b = sample_weight[b] (1 without weights)
//     loss = T^2 (sum_i w_b m_i kd_i) / N,   kept = sum_i m_i [w_b > 0]       (one partial pair per workgroup; the count is exact)
//     dz[i][c] (=, or += with `accumulate`: one fp32 add) ((p_c - q_c) (T / N)) grad_scale [w_b], every step rounded once
//     kd_i: where p_c < ST_TINY a class with p_c == q_c adds exactly 0 (distill.hip takes the log-sum-exp form there too)
//
// What the gate and the weight change is which bytes are touched.  A sample of weight 0 reads none of its maps; with `accumulate`
// (the training step: the hard loss has written dz) a dropped pixel's dz is neither read nor written, without it the pixel gets
// zeros.  The maps of a dropped pixel of a sample with w_b > 0 are read: its confidence is what drops it.
#include "../../include/asis_consist.h"
#include "soft_target.h"

extern "C" int asis_consist_tile(void) { return ST_TILE; }

extern "C" int asis_consist_nblk(int64_t N) { return st_nblk("asis_consist_nblk", N); }

extern "C" int asis_consist_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers, const int* hs,
                                 const int* ws, const int* flips, int V, int H, int W, int C, float temperature, float threshold,
                                 const float* sample_weight, float grad_scale, int accumulate, double* partial, float* loss,
                                 int* kept, float* dz) {
  return st_loss("asis_consist_loss", Gate{threshold, sample_weight}, stream, logits, B, h, w, teachers, hs, ws, flips, V, H, W, C,
                 temperature, grad_scale, accumulate, partial, loss, kept, dz);
}
