// Class-adaptive confidence thresholds for the consistency term (self-adaptive thresholding, FreeMatch): the gate of consist.hip
// and mix.hip with a threshold per class, the statistics of the teacher's maps, and the update of the thresholds from them.  Built
// into libasis_adapt.so (build.py SIDE_LIBS; ABI and semantics in include/asis_adapt.h), beside libasis_hip.so, whose error
// plumbing it uses.
//
//   st_kernel<.., ClassGate / MixClassGate>  soft_target.h's kernel; the gate compares the confidence with the threshold of the
//                        class that holds it.  The table is read inside the unrolled max loop at compile-time indices: uniform
//                        addresses, one select per class and pixel, no per-lane lookup.
//   adapt_stats_kernel   the teacher loop of st_kernel alone, over its tiles, grid and pixel order: per thread C + 1 doubles
//                        (S_c, S_conf) and a count, block_sum per quantity, C + 2 doubles per workgroup.  A sample with w_b <= 0
//                        reads none of its maps and counts no pixel.
//   adapt_stats_finalize_kernel  one workgroup, thread k sums quantity k over the partials in index order.
//   adapt_update_kernel  one workgroup: the two moving averages in double and the fp32 thresholds.
// No atomics anywhere: two calls give the same bits.
#include "../../include/asis_adapt.h"
#include "soft_target.h"

namespace {

constexpr int AD_MAXQ = MAXC + 2;  // S_0..S_{C-1}, S_conf, cnt

template <int CB, bool EXACT>
__global__ __launch_bounds__(RX_THREADS) void adapt_stats_kernel(const StViews vs, int H, int W, int C, int64_t N, int ntile, float inv_t,
                                                                 const float* __restrict__ sample_weight,
                                                                 double* __restrict__ part) {
  __shared__ double wd[(CB + 2) * RX_WAVES];  // a region per quantity: block_sum's barrier orders each on its own
  if constexpr (EXACT) __builtin_assume(C == CB);
  else __builtin_assume(C >= 1 && C <= CB);
  const int tid = threadIdx.x;
  const int64_t hw = (int64_t)H * W;
  double acc[CB], aconf = 0.0;
#pragma unroll
  for (int c = 0; c < CB; ++c) acc[c] = 0.0;
  int cnt = 0;
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
#pragma unroll 1
    for (int j = 0; j < ST_ITEMS; ++j) {
      const int64_t i = (int64_t)tile * ST_TILE + j * RX_THREADS + tid;
      if (i >= N) continue;
      const int b = (int)(i / hw);
      const int r = (int)(i - (int64_t)b * hw);
      const int y = r / W, x = r - y * W;
      if (sample_weight && !(sample_weight[b] > 0.f)) continue;  // the sample takes no soft term: none of its maps is read
      float q[CB];
#pragma unroll
      for (int c = 0; c < CB; ++c) q[c] = 0.f;
      // ONE call site of sample_view and softmax_c for every map, not unrolled, as in st_kernel: the arithmetic of its teacher loop
#pragma unroll 1
      for (int k = 0; k < vs.V; ++k) {
        const int hk = vs.h[k], wk = vs.w[k];
        float t[MAXC];
        sample_view<CB>(vs.p[k] + (int64_t)b * hk * wk * C, hk, wk, C, y, x, H, W, vs.flip[k] != 0, t);
#pragma unroll
        for (int c = 0; c < CB; ++c)
          if (c < C) t[c] = __fmul_rn(t[c], inv_t);
        softmax_c(t, C);
#pragma unroll
        for (int c = 0; c < CB; ++c)
          if (c < C) q[c] = __fadd_rn(q[c], t[c]);  // in list order
      }
      float conf = 0.f;
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (c < C) {
          if (vs.V > 1) q[c] = __fdiv_rn(q[c], (float)vs.V);  // a true division, as in st_kernel
          conf = fmaxf(conf, q[c]);
          acc[c] += (double)q[c];
        }
      aconf += (double)conf;
      ++cnt;
    }
  }
  double* out = part + (int64_t)blockIdx.x * (C + 2);
#pragma unroll
  for (int c = 0; c < CB; ++c)
    if (c < C) {
      const double s = block_sum(acc[c], wd + c * RX_WAVES);
      if (tid == 0) out[c] = s;
    }
  const double sc = block_sum(aconf, wd + CB * RX_WAVES);
  const double n = block_sum((double)cnt, wd + (CB + 1) * RX_WAVES);  // integers below 2^31 in double: exact
  if (tid == 0) {
    out[C] = sc;
    out[C + 1] = n;
  }
}

// sums[k] = the partials of quantity k in index order (thread k; the count is a sum of integers: exact)
__global__ __launch_bounds__(64) void adapt_stats_finalize_kernel(const double* __restrict__ part, int nblk, int Q,
                                                                  double* __restrict__ sums) {
  const int k = threadIdx.x;
  if (k >= Q) return;
  double s = 0.0;
  for (int i = 0; i < nblk; ++i) s += part[(int64_t)i * Q + k];
  sums[k] = s;
}

// state = tau, n_updates, ptilde[C].  cnt == 0 (uniform over the workgroup): nothing is written.  No contraction: every step is
// rounded once, as the plain recursion in double is.
__global__ __launch_bounds__(64) void adapt_update_kernel(const double* __restrict__ sums, double* __restrict__ state,
                                                          float* __restrict__ thr, int C, double lam) {
  __shared__ double pt[MAXC];
  const int c = threadIdx.x;
  const double cnt = sums[C + 1];
  if (!(cnt > 0.0)) return;
  const double one_m = 1.0 - lam;
  const double tau = __dadd_rn(__dmul_rn(lam, state[0]), __dmul_rn(one_m, __ddiv_rn(sums[C], cnt)));
  const double nup = state[1] + 1.0;
  if (c < C) pt[c] = __dadd_rn(__dmul_rn(lam, state[2 + c]), __dmul_rn(one_m, __ddiv_rn(sums[c], cnt)));
  __syncthreads();  // every thread has read the old state and sees the new ptilde
  if (c == 0) {
    state[0] = tau;
    state[1] = nup;
  }
  if (c < C) {
    double mx = pt[0];
    for (int k = 1; k < C; ++k) mx = fmax(mx, pt[k]);
    state[2 + c] = pt[c];
    thr[c] = (float)__ddiv_rn(__dmul_rn(tau, pt[c]), mx);
  }
}

bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

}  // namespace

extern "C" int asis_adapt_tile(void) { return ST_TILE; }

extern "C" int asis_adapt_nblk(int64_t N) { return st_nblk("asis_adapt_nblk", N); }

extern "C" int asis_adapt_stats_nblk(int64_t N) { return st_nblk("asis_adapt_stats_nblk", N); }

extern "C" int asis_adapt_consist_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers,
                                       const int* hs, const int* ws, const int* flips, int V, int H, int W, int C, float temperature,
                                       const float* class_threshold, const float* sample_weight, float grad_scale, int accumulate,
                                       double* partial, float* loss, int* kept, float* dz) {
  return st_loss("asis_adapt_consist_loss", ClassGate{class_threshold, sample_weight}, stream, logits, B, h, w, teachers, hs, ws, flips,
                 V, H, W, C, temperature, grad_scale, accumulate, partial, loss, kept, dz);
}

extern "C" int asis_adapt_mix_consist_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers,
                                           const int* hs, const int* ws, const int* flips, int V, int H, int W, int C,
                                           float temperature, const float* class_threshold, const float* sample_weight,
                                           const uint8_t* sel, const int* donor, float grad_scale, int accumulate, double* partial,
                                           float* loss, int* kept, float* dz) {
  return st_loss("asis_adapt_mix_consist_loss", MixClassGate{class_threshold, sample_weight, sel, donor, B}, stream, logits, B, h, w,
                 teachers, hs, ws, flips, V, H, W, C, temperature, grad_scale, accumulate, partial, loss, kept, dz);
}

extern "C" int asis_adapt_stats(void* stream, int B, const float* const* teachers, const int* hs, const int* ws, const int* flips, int V,
                                int H, int W, int C, float temperature, const float* sample_weight, double* partial, double* sums) {
  const char* op = "asis_adapt_stats";
  ASIS_REQUIRE(V >= 1 && V <= ST_MAXVIEWS, "%s: V=%d teacher maps, supported 1..%d", op, V, ST_MAXVIEWS);
  ASIS_REQUIRE(teachers && hs && ws && flips && partial && sums, "%s: null pointer", op);
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "%s: C=%d must be in 1..%d", op, C, MAXC);
  ASIS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive size B=%d H=%d W=%d", op, B, H, W);
  ASIS_REQUIRE(temperature > 0.f, "%s: temperature=%g must be > 0", op, (double)temperature);
  const int64_t N = (int64_t)B * H * W;
  ASIS_REQUIRE(N < ((int64_t)1 << 31), "%s: B*H*W=%lld must be < 2^31", op, (long long)N);
  ASIS_REQUIRE(aligned8(partial) && aligned8(sums), "%s: partial and sums must be 8-byte aligned", op);
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
  auto go = [&](auto cb, auto exact) {
    hipLaunchKernelGGL((adapt_stats_kernel<decltype(cb)::value, decltype(exact)::value>), grid, dim3(RX_THREADS), 0, s, vs, H, W, C, N,
                       ntile, inv_t, sample_weight, partial);
  };
  using std::integral_constant;
  if (C == 2) go(integral_constant<int, 2>{}, std::true_type{});
  else if (C == 4) go(integral_constant<int, 4>{}, std::true_type{});
  else if (C == 8) go(integral_constant<int, 8>{}, std::true_type{});
  else if (C == 16) go(integral_constant<int, 16>{}, std::true_type{});
  else if (C < 4) go(integral_constant<int, 4>{}, std::false_type{});
  else if (C < 8) go(integral_constant<int, 8>{}, std::false_type{});
  else go(integral_constant<int, 16>{}, std::false_type{});
  static_assert(AD_MAXQ <= 64, "one thread per quantity");
  hipLaunchKernelGGL(adapt_stats_finalize_kernel, dim3(1), dim3(64), 0, s, partial, (int)grid.x, C + 2, sums);
  ASIS_CHECK_LAUNCH(op);
  return ASIS_OK;
}

extern "C" int asis_adapt_update(void* stream, const double* sums, double* state, float* thr, int C, double momentum) {
  const char* op = "asis_adapt_update";
  ASIS_REQUIRE(sums && state && thr, "%s: null pointer", op);
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "%s: C=%d must be in 1..%d", op, C, MAXC);
  ASIS_REQUIRE(momentum >= 0.0 && momentum < 1.0, "%s: momentum=%g must be in [0, 1)", op, momentum);
  ASIS_REQUIRE(aligned8(sums) && aligned8(state), "%s: sums and state must be 8-byte aligned", op);
  hipLaunchKernelGGL(adapt_update_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), sums, state, thr, C, momentum);
  ASIS_CHECK_LAUNCH(op);
  return ASIS_OK;
}
