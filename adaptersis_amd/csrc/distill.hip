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
// (below DS_TINY: a saturated student) under q_c > 0, log p_c comes from the log-sum-exp of the student's row and the term is
// q_c (logf(q_c) - log p_c): finite.
//
// One pass: nothing of size [B,H,W,C] exists but dz.  The maps are read through the caches (they are small), dz is written once (and
// read once when it is added into) with 16-byte accesses where C*4 is a multiple of 16 and dz is 16-byte aligned.  A tile is 256
// threads x 4 pixels, pixel = tile*1024 + item*256 + thread (consecutive threads hold consecutive pixels: coalesced); a workgroup
// walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ...  The loss has a fixed order: per thread the pixels in that order in
// double, block_sum over the workgroup, one partial per workgroup, distill_finalize_kernel over the partials.  No float atomics.
#include <type_traits>

#include "../../include/asis_distill.h"
#include "asis_common.h"
#include "bilinear_tap.h"    // MAXC, Tap, tap_ac_false, blend_taps, softmax_c
#include "radix_routines.h"  // RX_THREADS, block_sum, tree_sum256

namespace {

constexpr int DS_ITEMS = 4, DS_TILE = RX_THREADS * DS_ITEMS;
constexpr int DS_MAX_BLOCKS = 2048;  // cap of the grid (8 workgroups a CU); it sets the order of the partial sums
constexpr int DS_MAXVIEWS = 8;
constexpr float DS_TINY = 1e-30f;  // below it a probability counts as underflowed: its logarithm comes from the log-sum-exp

struct DistillViews {
  const float* p[DS_MAXVIEWS];
  int h[DS_MAXVIEWS], w[DS_MAXVIEWS], flip[DS_MAXVIEWS];
  int V;
};

// sample_logits of bilinear_tap.h for a map whose columns may be mirrored
template <int CB>
__device__ __forceinline__ void sample_view(const float* __restrict__ lg, int h, int w, int C, int y, int x, int H, int W, bool flip,
                                            float* z) {
  const Tap ty = tap_ac_false(y, (float)h / (float)H, h), tx = tap_ac_false(x, (float)w / (float)W, w);
  const int j0 = flip ? w - 1 - tx.i0 : tx.i0, j1 = flip ? w - 1 - tx.i1 : tx.i1;
  const float* p00 = lg + ((int64_t)ty.i0 * w + j0) * C;
  const float* p01 = lg + ((int64_t)ty.i0 * w + j1) * C;
  const float* p10 = lg + ((int64_t)ty.i1 * w + j0) * C;
  const float* p11 = lg + ((int64_t)ty.i1 * w + j1) * C;
#pragma unroll
  for (int c = 0; c < CB; ++c)
    if (c < C) z[c] = blend_taps(ty, tx, p00[c], p01[c], p10[c], p11[c]);
}

// log sum_c exp(zs_c) of a scaled row: log softmax_c = zs[c] - this, for the classes whose probability underflows
template <int CB>
__device__ __forceinline__ float row_lse(const float* zs, int C) {
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < CB; ++c)
    if (c < C) m = fmaxf(m, zs[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < CB; ++c)
    if (c < C) s += expf(zs[c] - m);
  return m + logf(s);
}

// CB >= C the unrolled class count; EXACT: C == CB (no per-class branch).  `vec`: 16-byte accesses to dz (C % 4 == 0, dz aligned).
template <int CB, bool EXACT>
__global__ __launch_bounds__(RX_THREADS) void distill_kernel(const float* __restrict__ logits, int h, int w, const DistillViews vs,
                                                             int H, int W, int C, int64_t N, int ntile, float inv_t,
                                                             float t_over_n, float grad_scale, int accumulate, int vec,
                                                             double* __restrict__ part, float* __restrict__ dz) {
  __shared__ double wd[RX_WAVES];
  if constexpr (EXACT) __builtin_assume(C == CB);
  else __builtin_assume(C >= 1 && C <= CB);
  const int tid = threadIdx.x;
  const int64_t hw = (int64_t)H * W;
  double acc = 0.0;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
#pragma unroll 1
    for (int j = 0; j < DS_ITEMS; ++j) {
      const int64_t i = (int64_t)tile * DS_TILE + j * RX_THREADS + tid;
      if (i >= N) continue;
      const int b = (int)(i / hw);
      const int r = (int)(i - (int64_t)b * hw);
      const int y = r / W, x = r - y * W;
      float p[CB], zs[CB], q[CB];
#pragma unroll
      for (int c = 0; c < CB; ++c) p[c] = zs[c] = q[c] = 0.f;
      // Map -1 is the student.  ONE body for the student and every teacher map, not unrolled: the compiler contracts the blend
      // into fused multiply-adds per call site, and two call sites of the same source have been seen to round differently.
      // Through one, a teacher map that holds the student's values gives the student's bits (p == q), and a mirrored map the bits
      // of its un-mirrored twin.
#pragma unroll 1
      for (int k = -1; k < vs.V; ++k) {
        const bool student = k < 0;
        const int hk = student ? h : vs.h[k], wk = student ? w : vs.w[k];
        const float* lg = student ? logits : vs.p[k];
        float t[MAXC];  // MAXC: the row softmax_c of bilinear_tap.h takes; entries >= CB are never touched
        sample_view<CB>(lg + (int64_t)b * hk * wk * C, hk, wk, C, y, x, H, W, !student && vs.flip[k] != 0, t);
#pragma unroll
        for (int c = 0; c < CB; ++c)
          if (c < C) t[c] = __fmul_rn(t[c], inv_t);
        if (student) {
#pragma unroll
          for (int c = 0; c < CB; ++c)
            if (c < C) zs[c] = t[c];
        }
        softmax_c(t, C);
#pragma unroll
        for (int c = 0; c < CB; ++c)
          if (c < C) {
            if (student) p[c] = t[c];
            else q[c] = __fadd_rn(q[c], t[c]);  // in list order: bit-identical from call to call
          }
      }
      bool tiny = false;
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (c < C) {
          // a true division: times a rounded 1/V every q_c is off by the same factor, and the loss by T^2 times that
          if (vs.V > 1) q[c] = __fdiv_rn(q[c], (float)vs.V);
          tiny |= q[c] > 0.f && p[c] < DS_TINY;
        }
      const float lse_p = tiny ? row_lse<CB>(zs, C) : 0.f;
      float kd = 0.f;
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (c < C && q[c] > 0.f) {
          const float lr = p[c] >= DS_TINY ? logf(__fdiv_rn(q[c], p[c])) : logf(q[c]) - (zs[c] - lse_p);
          kd += q[c] * lr;
        }
      acc += (double)kd;

      float g[CB];
#pragma unroll
      for (int c = 0; c < CB; ++c)  // no contraction: p == q gives 0, and a grad_scale 2^n scales the bits
        g[c] = c < C ? __fmul_rn(__fmul_rn(__fsub_rn(p[c], q[c]), t_over_n), grad_scale) : 0.f;
      float* out = dz + i * C;
      if (vec) {
#pragma unroll
        for (int c0 = 0; c0 + 3 < CB; c0 += 4)
          if (c0 < C) {
            f32x4 v = {g[c0], g[c0 + 1], g[c0 + 2], g[c0 + 3]};
            f32x4* o4 = reinterpret_cast<f32x4*>(out + c0);
            if (accumulate) {
              const f32x4 old = *o4;
#pragma unroll
              for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(old[e], v[e]);
            }
            *o4 = v;
          }
      } else {
#pragma unroll
        for (int c = 0; c < CB; ++c)
          if (c < C) out[c] = accumulate ? __fadd_rn(out[c], g[c]) : g[c];
      }
    }
  }
  const double sum = block_sum(acc, wd);
  if (tid == 0) part[blockIdx.x] = sum;
}

// loss = sum of the workgroup partials (double, fixed order) * scale
__global__ __launch_bounds__(RX_THREADS) void distill_finalize_kernel(const double* __restrict__ part, int nblk, double scale,
                                                                      float* __restrict__ loss) {
  __shared__ double red[RX_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < nblk; i += RX_THREADS) s += part[i];
  const double sum = tree_sum256(s, red);
  if (tid == 0) *loss = (float)(sum * scale);
}

inline int ds_ntile(int64_t N) { return (int)((N + DS_TILE - 1) / DS_TILE); }

template <int CB, bool EXACT, typename... Args>
void ds_launch(dim3 grid, hipStream_t s, Args... args) {
  hipLaunchKernelGGL((distill_kernel<CB, EXACT>), grid, dim3(RX_THREADS), 0, s, args...);
}

}  // namespace

extern "C" int asis_distill_tile(void) { return DS_TILE; }

extern "C" int asis_distill_nblk(int64_t N) {
  if (N < 1 || N >= ((int64_t)1 << 31)) {
    asis_set_error_("asis_distill_nblk: need 1 <= N < 2^31");
    return ASIS_EINVAL;
  }
  return asis_grid(ds_ntile(N), 1, DS_MAX_BLOCKS);
}

extern "C" int asis_distill_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers, const int* hs,
                                 const int* ws, const int* flips, int V, int H, int W, int C, float temperature, float grad_scale,
                                 int accumulate, double* partial, float* loss, float* dz) {
  ASIS_REQUIRE(V >= 1 && V <= DS_MAXVIEWS, "asis_distill_loss: V=%d teacher maps, supported 1..%d", V, DS_MAXVIEWS);
  ASIS_REQUIRE(logits && teachers && hs && ws && flips && partial && loss && dz, "asis_distill_loss: null pointer");
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "asis_distill_loss: C=%d must be in 1..%d", C, MAXC);
  ASIS_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "asis_distill_loss: non-positive size B=%d h=%d w=%d H=%d W=%d", B, h,
               w, H, W);
  ASIS_REQUIRE(temperature > 0.f, "asis_distill_loss: temperature=%g must be > 0", (double)temperature);
  const int64_t N = (int64_t)B * H * W;
  ASIS_REQUIRE(N < ((int64_t)1 << 31), "asis_distill_loss: B*H*W=%lld must be < 2^31", (long long)N);
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(partial) & 7) == 0, "asis_distill_loss: partial must be 8-byte aligned");
  DistillViews vs = {};
  vs.V = V;
  for (int k = 0; k < V; ++k) {
    ASIS_REQUIRE(teachers[k], "asis_distill_loss: teachers[%d] is a null pointer", k);
    ASIS_REQUIRE(hs[k] >= 1 && ws[k] >= 1, "asis_distill_loss: non-positive size of teacher map %d: hs=%d ws=%d", k, hs[k], ws[k]);
    vs.p[k] = teachers[k];
    vs.h[k] = hs[k];
    vs.w[k] = ws[k];
    vs.flip[k] = flips[k] != 0;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ntile = ds_ntile(N);
  const dim3 grid(asis_grid(ntile, 1, DS_MAX_BLOCKS));
  const float inv_t = 1.f / temperature;
  const float t_over_n = (float)((double)temperature / (double)N);
  const int vec = (C % 4 == 0 && asis_aligned16(dz)) ? 1 : 0;
  auto go = [&](auto cb, auto exact) {
    ds_launch<decltype(cb)::value, decltype(exact)::value>(grid, s, logits, h, w, vs, H, W, C, N, ntile, inv_t, t_over_n,
                                                           grad_scale, accumulate, vec, partial, dz);
  };
  using std::integral_constant;
  if (C == 2) go(integral_constant<int, 2>{}, std::true_type{});
  else if (C == 4) go(integral_constant<int, 4>{}, std::true_type{});
  else if (C == 8) go(integral_constant<int, 8>{}, std::true_type{});
  else if (C == 16) go(integral_constant<int, 16>{}, std::true_type{});
  else if (C < 4) go(integral_constant<int, 4>{}, std::false_type{});
  else if (C < 8) go(integral_constant<int, 8>{}, std::false_type{});
  else go(integral_constant<int, 16>{}, std::false_type{});
  hipLaunchKernelGGL(distill_finalize_kernel, dim3(1), dim3(RX_THREADS), 0, s, partial, (int)grid.x,
                     (double)temperature * (double)temperature / (double)N, loss);
  ASIS_CHECK_LAUNCH("asis_distill_loss");
  return ASIS_OK;
}
