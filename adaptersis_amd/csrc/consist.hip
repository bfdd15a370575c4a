// The consistency term of teacher-student (mean-teacher) training: the distillation loss of distill.hip with a per-pixel
// confidence gate, a per-sample weight and the count of the pixels the gate let through.  Built into libasis_consist.so (build.py
// SIDE_LIBS; ABI in include/asis_consist.h), beside libasis_hip.so, whose error plumbing it uses.  distill.hip stays what it is
// (its library's symbol list is pinned), so the arithmetic it documents is restated here, not shared:
//
//     i = (b*H + y)*W + x the flat native pixel, N = B*H*W, T the temperature, V the number of teacher maps
//     z, t_k = resize(student), resize(teacher map k) at H x W; a mirrored map mirrors the two column indices
//     p = softmax(z * (1/T)),  q = (sum_k softmax(t_k * (1/T))) / V           (views in list order; 1/T rounded to fp32 once)
//     kd_i = sum_c q_c logf(q_c / p_c)  (0 where q_c = 0; the log-sum-exp of the student's row where p_c < CS_TINY and p_c != q_c)
//     conf_i = max_c q_c,  m_i = [conf_i >= threshold],  w_b = sample_weight[b] (1 without weights)
//     loss = T^2 (sum_i w_b m_i kd_i) / N,   kept = sum_i m_i [w_b > 0]
//     dz[i][c] (=, or += with `accumulate`: one fp32 add) ((p_c - q_c) (T / N)) grad_scale [w_b], every step rounded once
//
// What the gate and the weight change is which bytes are touched.  A sample of weight 0 reads none of its maps; with `accumulate`
// (the training step: the hard loss has written dz) a dropped pixel's dz is neither read nor written, without it the pixel gets
// zeros.  The maps of a dropped pixel of a sample with w_b > 0 are read: its confidence is what drops it.
//
// Tiles, grid, the walk and the order of the sums are those of distill.hip: 256 threads x 4 pixels a tile, pixel = tile*1024 +
// item*256 + thread, a workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ...; per thread the pixels in that order in
// double, block_sum over the workgroup, one partial pair (loss, kept) per workgroup, consist_finalize_kernel over the partials.
// The kept count is a sum of integers below 2^31 in double: exact.  No float atomics.
#include <type_traits>

#include "../../include/asis_consist.h"
#include "asis_common.h"
#include "bilinear_tap.h"    // MAXC, Tap, tap_ac_false, blend_taps, softmax_c
#include "radix_routines.h"  // RX_THREADS, block_sum, tree_sum256

namespace {

constexpr int CS_ITEMS = 4, CS_TILE = RX_THREADS * CS_ITEMS;
constexpr int CS_MAX_BLOCKS = 2048;  // cap of the grid (8 workgroups a CU); it sets the order of the partial sums
constexpr int CS_MAXVIEWS = 8;
constexpr float CS_TINY = 1e-30f;  // below it a probability counts as underflowed: its logarithm comes from the log-sum-exp

struct ConsistViews {
  const float* p[CS_MAXVIEWS];
  int h[CS_MAXVIEWS], w[CS_MAXVIEWS], flip[CS_MAXVIEWS];
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

// dz of one pixel: g, or zeros.  `vec`: 16-byte accesses (C % 4 == 0, dz aligned)
template <int CB>
__device__ __forceinline__ void store_row(float* __restrict__ out, const float* g, int C, int vec, bool add) {
  if (vec) {
#pragma unroll
    for (int c0 = 0; c0 + 3 < CB; c0 += 4)
      if (c0 < C) {
        f32x4 v = {g[c0], g[c0 + 1], g[c0 + 2], g[c0 + 3]};
        f32x4* o4 = reinterpret_cast<f32x4*>(out + c0);
        if (add) {
          const f32x4 old = *o4;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = __fadd_rn(old[e], v[e]);
        }
        *o4 = v;
      }
  } else {
#pragma unroll
    for (int c = 0; c < CB; ++c)
      if (c < C) out[c] = add ? __fadd_rn(out[c], g[c]) : g[c];
  }
}

// CB >= C the unrolled class count; EXACT: C == CB (no per-class branch)
template <int CB, bool EXACT>
__global__ __launch_bounds__(RX_THREADS) void consist_kernel(const float* __restrict__ logits, int h, int w, const ConsistViews vs,
                                                             int H, int W, int C, int64_t N, int ntile, float inv_t,
                                                             float t_over_n, float threshold,
                                                             const float* __restrict__ sample_weight, float grad_scale,
                                                             int accumulate, int vec, double* __restrict__ part,
                                                             float* __restrict__ dz) {
  __shared__ double wd[RX_WAVES], wk[RX_WAVES];
  if constexpr (EXACT) __builtin_assume(C == CB);
  else __builtin_assume(C >= 1 && C <= CB);
  const int tid = threadIdx.x;
  const int64_t hw = (int64_t)H * W;
  double acc = 0.0;
  int nkept = 0;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
#pragma unroll 1
    for (int j = 0; j < CS_ITEMS; ++j) {
      const int64_t i = (int64_t)tile * CS_TILE + j * RX_THREADS + tid;
      if (i >= N) continue;
      const int b = (int)(i / hw);
      const int r = (int)(i - (int64_t)b * hw);
      const int y = r / W, x = r - y * W;
      float* out = dz + i * C;
      float g[CB];
#pragma unroll
      for (int c = 0; c < CB; ++c) g[c] = 0.f;
      const float wb = sample_weight ? sample_weight[b] : 1.f;
      if (!(wb > 0.f)) {  // the sample takes no soft term: none of its maps is read
        if (!accumulate) store_row<CB>(out, g, C, vec, false);
        continue;
      }
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
        const int hk = student ? h : vs.h[k], wk_ = student ? w : vs.w[k];
        const float* lg = student ? logits : vs.p[k];
        float t[MAXC];  // MAXC: the row softmax_c of bilinear_tap.h takes; entries >= CB are never touched
        sample_view<CB>(lg + (int64_t)b * hk * wk_ * C, hk, wk_, C, y, x, H, W, !student && vs.flip[k] != 0, t);
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
      float conf = 0.f;
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (c < C) {
          // a true division: times a rounded 1/V every q_c is off by the same factor, and the loss by T^2 times that
          if (vs.V > 1) q[c] = __fdiv_rn(q[c], (float)vs.V);
          conf = fmaxf(conf, q[c]);
        }
      if (!(conf >= threshold)) {  // the teacher is unsure here
        if (!accumulate) store_row<CB>(out, g, C, vec, false);
        continue;
      }
      ++nkept;
      bool tiny = false;
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (c < C) tiny |= q[c] > 0.f && p[c] < CS_TINY;
      const float lse_p = tiny ? row_lse<CB>(zs, C) : 0.f;
      float kd = 0.f;
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (c < C && q[c] > 0.f) {
          // equal values have the ratio 1 whatever their size: a student that is its own teacher costs exactly 0 also where it
          // is saturated (the log-sum-exp form would leave the rounding of two logarithms)
          const float lr = p[c] >= CS_TINY ? logf(__fdiv_rn(q[c], p[c])) : p[c] == q[c] ? 0.f : logf(q[c]) - (zs[c] - lse_p);
          kd += q[c] * lr;
        }
      acc += (double)wb * (double)kd;
#pragma unroll
      for (int c = 0; c < CB; ++c)  // no contraction: p == q gives 0, a grad_scale 2^n scales the bits, a weight of 1 changes none
        if (c < C) {
          const float gc = __fmul_rn(__fmul_rn(__fsub_rn(p[c], q[c]), t_over_n), grad_scale);
          g[c] = sample_weight ? __fmul_rn(gc, wb) : gc;
        }
      store_row<CB>(out, g, C, vec, accumulate != 0);
    }
  }
  const double sum = block_sum(acc, wd);
  const double cnt = block_sum((double)nkept, wk);
  if (tid == 0) {
    part[2 * blockIdx.x] = sum;
    part[2 * blockIdx.x + 1] = cnt;
  }
}

// loss = sum of the workgroup partials (double, fixed order) * scale; kept = the sum of the counts
__global__ __launch_bounds__(RX_THREADS) void consist_finalize_kernel(const double* __restrict__ part, int nblk, double scale,
                                                                      float* __restrict__ loss, int* __restrict__ kept) {
  __shared__ double red[RX_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0, k = 0.0;
  for (int i = tid; i < nblk; i += RX_THREADS) {
    s += part[2 * i];
    k += part[2 * i + 1];
  }
  const double sum = tree_sum256(s, red);
  __syncthreads();
  const double cnt = tree_sum256(k, red);
  if (tid == 0) {
    *loss = (float)(sum * scale);
    *kept = (int)cnt;
  }
}

inline int cs_ntile(int64_t N) { return (int)((N + CS_TILE - 1) / CS_TILE); }

template <int CB, bool EXACT, typename... Args>
void cs_launch(dim3 grid, hipStream_t s, Args... args) {
  hipLaunchKernelGGL((consist_kernel<CB, EXACT>), grid, dim3(RX_THREADS), 0, s, args...);
}

}  // namespace

extern "C" int asis_consist_tile(void) { return CS_TILE; }

extern "C" int asis_consist_nblk(int64_t N) {
  if (N < 1 || N >= ((int64_t)1 << 31)) {
    asis_set_error_("asis_consist_nblk: need 1 <= N < 2^31");
    return ASIS_EINVAL;
  }
  return asis_grid(cs_ntile(N), 1, CS_MAX_BLOCKS);
}

extern "C" int asis_consist_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers, const int* hs,
                                 const int* ws, const int* flips, int V, int H, int W, int C, float temperature, float threshold,
                                 const float* sample_weight, float grad_scale, int accumulate, double* partial, float* loss,
                                 int* kept, float* dz) {
  ASIS_REQUIRE(V >= 1 && V <= CS_MAXVIEWS, "asis_consist_loss: V=%d teacher maps, supported 1..%d", V, CS_MAXVIEWS);
  ASIS_REQUIRE(logits && teachers && hs && ws && flips && partial && loss && kept && dz, "asis_consist_loss: null pointer");
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "asis_consist_loss: C=%d must be in 1..%d", C, MAXC);
  ASIS_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "asis_consist_loss: non-positive size B=%d h=%d w=%d H=%d W=%d", B, h,
               w, H, W);
  ASIS_REQUIRE(temperature > 0.f, "asis_consist_loss: temperature=%g must be > 0", (double)temperature);
  ASIS_REQUIRE(threshold <= 1.f, "asis_consist_loss: threshold=%g must be <= 1 (<= 0 keeps every pixel)", (double)threshold);
  const int64_t N = (int64_t)B * H * W;
  ASIS_REQUIRE(N < ((int64_t)1 << 31), "asis_consist_loss: B*H*W=%lld must be < 2^31", (long long)N);
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(partial) & 7) == 0, "asis_consist_loss: partial must be 8-byte aligned");
  ConsistViews vs = {};
  vs.V = V;
  for (int k = 0; k < V; ++k) {
    ASIS_REQUIRE(teachers[k], "asis_consist_loss: teachers[%d] is a null pointer", k);
    ASIS_REQUIRE(hs[k] >= 1 && ws[k] >= 1, "asis_consist_loss: non-positive size of teacher map %d: hs=%d ws=%d", k, hs[k], ws[k]);
    vs.p[k] = teachers[k];
    vs.h[k] = hs[k];
    vs.w[k] = ws[k];
    vs.flip[k] = flips[k] != 0;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ntile = cs_ntile(N);
  const dim3 grid(asis_grid(ntile, 1, CS_MAX_BLOCKS));
  const float inv_t = 1.f / temperature;
  const float t_over_n = (float)((double)temperature / (double)N);
  const int vec = (C % 4 == 0 && asis_aligned16(dz)) ? 1 : 0;
  auto go = [&](auto cb, auto exact) {
    cs_launch<decltype(cb)::value, decltype(exact)::value>(grid, s, logits, h, w, vs, H, W, C, N, ntile, inv_t, t_over_n, threshold,
                                                           sample_weight, grad_scale, accumulate, vec, partial, dz);
  };
  using std::integral_constant;
  if (C == 2) go(integral_constant<int, 2>{}, std::true_type{});
  else if (C == 4) go(integral_constant<int, 4>{}, std::true_type{});
  else if (C == 8) go(integral_constant<int, 8>{}, std::true_type{});
  else if (C == 16) go(integral_constant<int, 16>{}, std::true_type{});
  else if (C < 4) go(integral_constant<int, 4>{}, std::false_type{});
  else if (C < 8) go(integral_constant<int, 8>{}, std::false_type{});
  else go(integral_constant<int, 16>{}, std::false_type{});
  hipLaunchKernelGGL(consist_finalize_kernel, dim3(1), dim3(RX_THREADS), 0, s, partial, (int)grid.x,
                     (double)temperature * (double)temperature / (double)N, loss, kept);
  ASIS_CHECK_LAUNCH("asis_consist_loss");
  return ASIS_OK;
}
