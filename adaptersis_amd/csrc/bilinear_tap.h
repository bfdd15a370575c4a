// Bilinear sampling of the NHWC fp32 logits, shared by loss.hip (losses, metrics, asis_resize_bilinear_fwd) and predict.hip
// (asis_predict_mask): one definition of the tap and of the four-term blend, so every kernel that resizes the logits
// computes the same bits (= F.interpolate(mode="bilinear", align_corners=False), train.py:422).  It also holds what every
// per-pixel loss kernel (loss.hip, lovasz.hip, hardpixel.hip) computes identically on the sampled row of at most MAXC classes:
// the softmax and its transpose.  The losses recompute a softmax instead of storing it and compare each other's results bit
// for bit, so there is one copy of that arithmetic.
#pragma once
#include "asis_common.h"

namespace {

constexpr int MAXC = 16;

struct Tap {
  int i0, i1;
  float l0, l1;
};
// area_pixel_compute_source_index(align_corners=False): src = scale*(dst+0.5)-0.5, clamped at 0
__device__ __forceinline__ Tap tap_ac_false(int dst, float scale, int in) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  if (s < 0.f) s = 0.f;
  Tap t;
  t.i0 = (int)s;
  if (t.i0 > in - 1) t.i0 = in - 1;
  t.i1 = t.i0 + ((t.i0 < in - 1) ? 1 : 0);
  t.l1 = s - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// one channel of the interpolated pixel from its four neighbours (row i0: v00, v01; row i1: v10, v11)
__device__ __forceinline__ float blend_taps(const Tap& ty, const Tap& tx, float v00, float v01, float v10, float v11) {
  return ty.l0 * (tx.l0 * v00 + tx.l1 * v01) + ty.l1 * (tx.l0 * v10 + tx.l1 * v11);
}

// interpolated logits of output pixel (y, x) -> z[C]
__device__ __forceinline__ void sample_logits(const float* __restrict__ lg, int h, int w, int C, int y, int x, float sh,
                                              float sw, float* z) {
  const Tap ty = tap_ac_false(y, sh, h), tx = tap_ac_false(x, sw, w);
  const float* p00 = lg + ((int64_t)ty.i0 * w + tx.i0) * C;
  const float* p01 = lg + ((int64_t)ty.i0 * w + tx.i1) * C;
  const float* p10 = lg + ((int64_t)ty.i1 * w + tx.i0) * C;
  const float* p11 = lg + ((int64_t)ty.i1 * w + tx.i1) * C;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) z[c] = blend_taps(ty, tx, p00[c], p01[c], p10[c], p11[c]);
}
// the same for the flat pixel index i = (b * H + y) * W + x of a batch resized from h x w to H x W
__device__ __forceinline__ void sample_logits_at(const float* __restrict__ logits, int h, int w, int H, int W, int C, int64_t i,
                                                 float* z) {
  const int64_t hw = (int64_t)H * W;
  const int b = (int)(i / hw);
  const int p = (int)(i - (int64_t)b * hw);
  const int y = p / W, x = p - y * W;
  sample_logits(logits + (int64_t)b * h * w * C, h, w, C, y, x, (float)h / (float)H, (float)w / (float)W, z);
}

// z <- softmax(z) over the C classes, in registers
__device__ __forceinline__ void softmax_c(float* z, int C) {
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) m = fmaxf(m, z[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) {
      z[c] = __expf(z[c] - m);
      s += z[c];
    }
  const float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) z[c] *= inv;
}
__device__ __forceinline__ void softmax_bwd_c(float* g, const float* p, int C) {  // g <- p * (g - <g, p>)
  float dot = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) dot += g[c] * p[c];
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) g[c] = p[c] * (g[c] - dot);
}

}  // namespace
