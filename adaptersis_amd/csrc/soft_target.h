// The soft-target loss that distill.hip and consist.hip export: one kernel body, its finalize kernel and the host code in front of
// them, included by those two sources and by mix.hip, and by nothing in libasis_hip.so.  distill.hip documents the arithmetic,
// consist.hip what the gate and the weight add, mix.hip what the mixing adds; the gate is a type (NoGate / Gate / MixGate), so the
// ungated kernel carries nothing of the gate and neither of the first two anything of the mixing.
//
// A tile is 256 threads x 4 pixels, pixel = tile*1024 + item*256 + thread (consecutive threads hold consecutive pixels:
// coalesced); a workgroup walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ...  The sums have a fixed order: per thread the
// pixels in that order in double, block_sum over the workgroup, one partial (with a gate a pair: loss, kept) per workgroup,
// st_finalize_kernel over the partials.  No float atomics.
#pragma once
#include <type_traits>

#include "asis_common.h"
#include "bilinear_tap.h"    // MAXC, Tap, tap_ac_false, blend_taps, softmax_c
#include "radix_routines.h"  // RX_THREADS, block_sum, tree_sum256

namespace {

constexpr int ST_ITEMS = 4, ST_TILE = RX_THREADS * ST_ITEMS;
constexpr int ST_MAX_BLOCKS = 2048;  // cap of the grid (8 workgroups a CU); it sets the order of the partial sums
constexpr int ST_MAXVIEWS = 8;
constexpr float ST_TINY = 1e-30f;  // below it a probability counts as underflowed: its logarithm comes from the log-sum-exp

struct StViews {
  const float* p[ST_MAXVIEWS];
  int h[ST_MAXVIEWS], w[ST_MAXVIEWS], flip[ST_MAXVIEWS];
  int V;
};

// every pixel of every sample takes part with weight 1: one partial per workgroup
struct NoGate {
  static constexpr bool on = false, mix = false, cls = false;
};
// a pixel takes part where max_c q_c >= threshold, times sample_weight[b] (NULL: 1): two partials per workgroup, loss and kept
struct Gate {
  static constexpr bool on = true, mix = false, cls = false;
  float threshold;
  const float* sample_weight;
};
// Gate over a mixed batch (mix.hip): where sel[i] != 0 every teacher map of pixel i is read from sample donor[b], at the same
// (y, x); the student, the weight and dz are sample b's.  A donor outside 0..B-1 is read as b: it is never an address.
struct MixGate {
  static constexpr bool on = true, mix = true, cls = false;
  float threshold;
  const float* sample_weight;
  const uint8_t* sel;
  const int* donor;
  int B;
};
// Gate and MixGate with a threshold per class (adapt.hip): a pixel takes part where conf >= class_threshold[a], a the lowest
// index of the largest q_c; class_threshold is fp32 [C] on the device.  The table is read inside the unrolled max loop, at
// compile-time indices (uniform addresses), never at the per-lane arg-max.
struct ClassGate {
  static constexpr bool on = true, mix = false, cls = true;
  const float* class_threshold;
  const float* sample_weight;
};
struct MixClassGate {
  static constexpr bool on = true, mix = true, cls = true;
  const float* class_threshold;
  const float* sample_weight;
  const uint8_t* sel;
  const int* donor;
  int B;
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

// dz of a pixel the gate dropped, in a fresh dz.  `vec`: 16-byte accesses (C % 4 == 0, dz aligned)
template <int CB>
__device__ __forceinline__ void zero_row(float* __restrict__ out, int C, int vec) {
  if (vec) {
#pragma unroll
    for (int c0 = 0; c0 + 3 < CB; c0 += 4)
      if (c0 < C) *reinterpret_cast<f32x4*>(out + c0) = f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int c = 0; c < CB; ++c)
      if (c < C) out[c] = 0.f;
  }
}

// CB >= C the unrolled class count; EXACT: C == CB (no per-class branch); G: a gate type above.  The order of the statements is part
// of the kernel: with `tiny` in a loop of its own after the gate, or the store of a kept row behind a function, the ungated
// 9..16-class kernels spill scalar registers or take more vector registers than distill.hip's always did.
template <int CB, bool EXACT, typename G>
__global__ __launch_bounds__(RX_THREADS) void st_kernel(const float* __restrict__ logits, int h, int w, const StViews vs, int H, int W,
                                                        int C, int64_t N, int ntile, float inv_t, float t_over_n, float grad_scale,
                                                        int accumulate, int vec, double* __restrict__ part,
                                                        float* __restrict__ dz, const G gate) {
  __shared__ double wd[(G::on ? 2 : 1) * RX_WAVES];
  if constexpr (EXACT) __builtin_assume(C == CB);
  else __builtin_assume(C >= 1 && C <= CB);
  const int tid = threadIdx.x;
  const int64_t hw = (int64_t)H * W;
  double acc = 0.0;
  int nkept = 0;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
#pragma unroll 1
    for (int j = 0; j < ST_ITEMS; ++j) {
      const int64_t i = (int64_t)tile * ST_TILE + j * RX_THREADS + tid;
      if (i >= N) continue;
      const int b = (int)(i / hw);
      const int r = (int)(i - (int64_t)b * hw);
      const int y = r / W, x = r - y * W;
      // A dropped pixel (here and at the threshold below) gets zeros in a fresh dz; in a dz that is added into it is neither read
      // nor written.
      float wb = 1.f;
      if constexpr (G::on) {
        if (gate.sample_weight) wb = gate.sample_weight[b];
        if (!(wb > 0.f)) {  // the sample takes no soft term: none of its maps is read
          if (!accumulate) zero_row<CB>(dz + i * C, C, vec);
          continue;
        }
      }
      int bt = b;  // the sample the teacher's maps are read from
      if constexpr (G::mix) {
        if (gate.sel[i]) {
          const int d = gate.donor[b];
          if ((unsigned)d < (unsigned)gate.B) bt = d;
        }
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
        const int hk = student ? h : vs.h[k], wk = student ? w : vs.w[k];
        const float* lg = student ? logits : vs.p[k];
        float t[MAXC];  // MAXC: the row softmax_c of bilinear_tap.h takes; entries >= CB are never touched
        int bk = b;
        if constexpr (G::mix) bk = student ? b : bt;
        sample_view<CB>(lg + (int64_t)bk * hk * wk * C, hk, wk, C, y, x, H, W, !student && vs.flip[k] != 0, t);
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
      float conf = 0.f;
      [[maybe_unused]] float thr = 0.f;
      if constexpr (G::cls) thr = gate.class_threshold[0];  // no q_c above 0 (a row of NaNs): class 0's, as the scalar gate's 0
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (c < C) {
          // a true division: times a rounded 1/V every q_c is off by the same factor, and the loss by T^2 times that
          if (vs.V > 1) q[c] = __fdiv_rn(q[c], (float)vs.V);
          tiny |= q[c] > 0.f && p[c] < ST_TINY;
          if constexpr (G::cls) {
            if (q[c] > conf) {  // strictly: the lowest index wins a tie
              conf = q[c];
              thr = gate.class_threshold[c];
            }
          } else if constexpr (G::on) conf = fmaxf(conf, q[c]);
        }
      if constexpr (G::on) {
        if constexpr (!G::cls) thr = gate.threshold;
        if (!(conf >= thr)) {  // the teacher is unsure here
          if (!accumulate) zero_row<CB>(dz + i * C, C, vec);
          continue;
        }
        ++nkept;
      }
      const float lse_p = tiny ? row_lse<CB>(zs, C) : 0.f;
      float kd = 0.f;
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (c < C && q[c] > 0.f) {
          // The two ops differ here.  With a gate, equal values have the ratio 1 whatever their size: a student that is its own
          // teacher costs exactly 0 also where it is saturated.  Without one the log-sum-exp form leaves the rounding of two
          // logarithms there (about -6e-41): the bits libasis_distill.so has always given.
          const float lr = p[c] >= ST_TINY         ? logf(__fdiv_rn(q[c], p[c]))
                           : G::on && p[c] == q[c] ? 0.f
                                                   : logf(q[c]) - (zs[c] - lse_p);
          kd += q[c] * lr;
        }
      acc += G::on ? (double)wb * (double)kd : (double)kd;

      float g[CB];
#pragma unroll
      for (int c = 0; c < CB; ++c) {  // no contraction: p == q gives 0, a grad_scale 2^n scales the bits, a weight of 1 changes none
        g[c] = c < C ? __fmul_rn(__fmul_rn(__fsub_rn(p[c], q[c]), t_over_n), grad_scale) : 0.f;
        if constexpr (G::on)
          if (gate.sample_weight) g[c] = __fmul_rn(g[c], wb);
      }
      float* out = dz + i * C;
      if (vec) {  // 16-byte accesses (C % 4 == 0, dz aligned)
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
  constexpr int NS = G::on ? 2 : 1;
  const double sum = block_sum(acc, wd);
  if (tid == 0) part[NS * blockIdx.x] = sum;
  if constexpr (G::on) {  // the kept count is a sum of integers below 2^31 in double: exact
    const double cnt = block_sum((double)nkept, wd + RX_WAVES);
    if (tid == 0) part[NS * blockIdx.x + 1] = cnt;
  }
}

// loss = sum of the workgroup partials (double, fixed order) * scale; with NS = 2 also kept = the sum of the counts
template <int NS>
__global__ __launch_bounds__(RX_THREADS) void st_finalize_kernel(const double* __restrict__ part, int nblk, double scale,
                                                                 float* __restrict__ loss, int* __restrict__ kept) {
  __shared__ double red[RX_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0, k = 0.0;
  for (int i = tid; i < nblk; i += RX_THREADS) {
    s += part[NS * i];
    if constexpr (NS == 2) k += part[NS * i + 1];
  }
  const double sum = tree_sum256(s, red);
  if (tid == 0) *loss = (float)(sum * scale);
  if constexpr (NS == 2) {
    __syncthreads();
    const double cnt = tree_sum256(k, red);
    if (tid == 0) *kept = (int)cnt;
  }
}

inline int st_ntile(int64_t N) { return (int)((N + ST_TILE - 1) / ST_TILE); }

// asis_*_nblk: the workgroups, and so the partials (pairs with a gate), of N pixels
inline int st_nblk(const char* op, int64_t N) {
  if (N < 1 || N >= ((int64_t)1 << 31)) {
    asis_set_error_("%s: need 1 <= N < 2^31", op);
    return ASIS_EINVAL;
  }
  return asis_grid(st_ntile(N), 1, ST_MAX_BLOCKS);
}

// asis_distill_loss (NoGate; kept unused), asis_consist_loss (Gate) and asis_mix_consist_loss (MixGate): the argument checks under
// the name `op`, the launch by class count and the finalize
template <typename G>
int st_loss(const char* op, G gate, void* stream, const float* logits, int B, int h, int w, const float* const* teachers,
            const int* hs, const int* ws, const int* flips, int V, int H, int W, int C, float temperature, float grad_scale,
            int accumulate, double* partial, float* loss, int* kept, float* dz) {
  ASIS_REQUIRE(V >= 1 && V <= ST_MAXVIEWS, "%s: V=%d teacher maps, supported 1..%d", op, V, ST_MAXVIEWS);
  ASIS_REQUIRE(logits && teachers && hs && ws && flips && partial && loss && (kept || !G::on) && dz, "%s: null pointer", op);
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "%s: C=%d must be in 1..%d", op, C, MAXC);
  ASIS_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "%s: non-positive size B=%d h=%d w=%d H=%d W=%d", op, B, h, w, H, W);
  ASIS_REQUIRE(temperature > 0.f, "%s: temperature=%g must be > 0", op, (double)temperature);
  if constexpr (G::cls) ASIS_REQUIRE(gate.class_threshold, "%s: null pointer (class_threshold)", op);
  else if constexpr (G::on)
    ASIS_REQUIRE(gate.threshold <= 1.f, "%s: threshold=%g must be <= 1 (<= 0 keeps every pixel)", op, (double)gate.threshold);
  if constexpr (G::mix) ASIS_REQUIRE(gate.sel && gate.donor, "%s: null pointer (sel, donor)", op);
  const int64_t N = (int64_t)B * H * W;
  ASIS_REQUIRE(N < ((int64_t)1 << 31), "%s: B*H*W=%lld must be < 2^31", op, (long long)N);
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(partial) & 7) == 0, "%s: partial must be 8-byte aligned", op);
  StViews vs = {};
  vs.V = V;
  for (int k = 0; k < V; ++k) {
    ASIS_REQUIRE(teachers[k], "%s: teachers[%d] is a null pointer", op, k);
    ASIS_REQUIRE(hs[k] >= 1 && ws[k] >= 1, "%s: non-positive size of teacher map %d: hs=%d ws=%d", op, k, hs[k], ws[k]);
    vs.p[k] = teachers[k];
    vs.h[k] = hs[k];
    vs.w[k] = ws[k];
    vs.flip[k] = flips[k] != 0;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ntile = st_ntile(N);
  const dim3 grid(asis_grid(ntile, 1, ST_MAX_BLOCKS));
  const float inv_t = 1.f / temperature;
  const float t_over_n = (float)((double)temperature / (double)N);
  const int vec = (C % 4 == 0 && asis_aligned16(dz)) ? 1 : 0;
  auto go = [&](auto cb, auto exact) {
    hipLaunchKernelGGL((st_kernel<decltype(cb)::value, decltype(exact)::value, G>), grid, dim3(RX_THREADS), 0, s, logits, h, w, vs, H,
                       W, C, N, ntile, inv_t, t_over_n, grad_scale, accumulate, vec, partial, dz, gate);
  };
  using std::integral_constant;
  if (C == 2) go(integral_constant<int, 2>{}, std::true_type{});
  else if (C == 4) go(integral_constant<int, 4>{}, std::true_type{});
  else if (C == 8) go(integral_constant<int, 8>{}, std::true_type{});
  else if (C == 16) go(integral_constant<int, 16>{}, std::true_type{});
  else if (C < 4) go(integral_constant<int, 4>{}, std::false_type{});
  else if (C < 8) go(integral_constant<int, 8>{}, std::false_type{});
  else go(integral_constant<int, 16>{}, std::false_type{});
  hipLaunchKernelGGL(st_finalize_kernel<(G::on ? 2 : 1)>, dim3(1), dim3(RX_THREADS), 0, s, partial, (int)grid.x,
                     (double)temperature * (double)temperature / (double)N, loss, kept);
  ASIS_CHECK_LAUNCH(op);
  return ASIS_OK;
}

}  // namespace
