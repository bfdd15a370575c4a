// Exponential moving average of the flat fp32 parameter buckets (adaptersis_amd/optim.py: EMA).
// Two kernels per update, no host synchronisation:
//   ema_prepare (once)         the optimizer's skip decision -> update count, this update's weight 1 - decay(t), apply flag
//   ema_update  (per bucket)   e = fma(w, p - e, e) over the bucket, or nothing when the step was skipped
// Only ema_prepare writes the count and the record; the update kernels read them, so nothing races inside a grid (the rule of
// adamw.hip).  The decay and the count live on the device: no scalar argument changes from step to step.
#include "asis_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int GRID_CAP = 2048;     // 8 workgroups per CU on 256 CUs; the rest is the grid-stride walk

// One thread.  rec = {1 - decay(t), apply flag}; state = {updates applied}.
__global__ void ema_prepare_kernel(const int* __restrict__ guard, int* __restrict__ state, float* __restrict__ rec, double decay,
                                   int warmup) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (guard != nullptr && guard[0] != 0) {   // the optimizer skipped this step: the weights did not move, neither does the average
    rec[1] = 0.f;
    return;
  }
  const int t = ++state[0];
  double d = decay;
  if (warmup) d = fmin(decay, (1.0 + (double)t) / (10.0 + (double)t));
  rec[0] = (float)(1.0 - d);
  rec[1] = 1.f;
}

// an explicit fma: the bits do not depend on what the compiler contracts
__device__ __forceinline__ float ema1(const float e, const float p, const float w) { return __builtin_fmaf(w, p - e, e); }

// the average is touched once per step and by nothing in between: its loads and stores carry the non-temporal hint; the weights are
// read again right away (the 16-bit packs of the next forward), so theirs do not
__device__ __forceinline__ f32x4 load_nt(const f32x4* q) { return __builtin_nontemporal_load(q); }
__device__ __forceinline__ void store_nt(f32x4* q, const f32x4 v) { __builtin_nontemporal_store(v, q); }

// Both bases 16-byte aligned.  A tile is QUADS_PER_TILE = 4 x 256 consecutive quads (16 KB of each array), four quads per lane in
// flight; the capped grid walks the tiles with a grid stride.  Measured on the ViT-L bucket (304 M elements, 12 B each): one
// contiguous range per workgroup with two quads in flight, the adamw_step_kernel walk, 718 us; this walk with plain accesses 690;
// with the hint on the average 635.  The n % 4 tail goes to the first lanes of workgroup 0, one element each.
constexpr int QUADS_PER_LANE = 4;
constexpr int QUADS_PER_TILE = QUADS_PER_LANE * BLOCK;
__global__ __launch_bounds__(BLOCK) void ema_update_vec_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n,
                                                               const float* __restrict__ rec) {
  if (rec[1] == 0.f) return;   // uniform over the grid: written by ema_prepare, a kernel before this one
  const float w = rec[0];
  f32x4* __restrict__ e4 = reinterpret_cast<f32x4*>(ema);
  const f32x4* __restrict__ p4 = reinterpret_cast<const f32x4*>(p);
  const int64_t n4 = n / 4;
  const int64_t stride = (int64_t)gridDim.x * QUADS_PER_TILE;
  for (int64_t i = (int64_t)blockIdx.x * QUADS_PER_TILE + threadIdx.x; i < n4; i += stride) {
    f32x4 e[QUADS_PER_LANE], q[QUADS_PER_LANE];
#pragma unroll
    for (int u = 0; u < QUADS_PER_LANE; ++u) {
      const int64_t j = i + u * BLOCK < n4 ? i + u * BLOCK : i;   // past the end in the last tile: read quad i again, store nothing
      e[u] = load_nt(e4 + j);
      q[u] = p4[j];
    }
#pragma unroll
    for (int u = 0; u < QUADS_PER_LANE; ++u) {
      if (u == 0 || i + u * BLOCK < n4) {
        f32x4 r;
        r.x = ema1(e[u].x, q[u].x, w); r.y = ema1(e[u].y, q[u].y, w); r.z = ema1(e[u].z, q[u].z, w); r.w = ema1(e[u].w, q[u].w, w);
        store_nt(e4 + i + u * BLOCK, r);
      }
    }
  }
  const int64_t k = 4 * n4 + threadIdx.x;
  if (blockIdx.x == 0 && k < n) ema[k] = ema1(ema[k], p[k], w);
}

// A misaligned base (the ABI is public; a flat bucket never is): one element per lane, grid-stride.
__global__ __launch_bounds__(BLOCK) void ema_update_scalar_kernel(float* __restrict__ ema, const float* __restrict__ p, int64_t n,
                                                                  const float* __restrict__ rec) {
  if (rec[1] == 0.f) return;
  const float w = rec[0];
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) ema[i] = ema1(ema[i], p[i], w);
}

}  // namespace

extern "C" int asis_ema_prepare(void* stream, const int32_t* guard, int32_t* state, float* rec, double decay, int warmup) {
  ASIS_REQUIRE(state && rec, "asis_ema_prepare: null pointer");
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(guard) & 3) == 0 && (reinterpret_cast<uintptr_t>(state) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(rec) & 3) == 0, "asis_ema_prepare: misaligned pointer");
  ASIS_REQUIRE(decay > 0.0 && decay < 1.0, "asis_ema_prepare: decay=%g must lie in (0, 1)", decay);
  hipLaunchKernelGGL(ema_prepare_kernel, dim3(1), dim3(1), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const int*>(guard), reinterpret_cast<int*>(state), rec, decay, warmup);
  ASIS_CHECK_LAUNCH("asis_ema_prepare");
  return ASIS_OK;
}

extern "C" int asis_ema_update(void* stream, float* ema, const float* p, int64_t n, const float* rec) {
  ASIS_REQUIRE(ema && p && rec, "asis_ema_update: null pointer");
  ASIS_REQUIRE(n >= 0, "asis_ema_update: n=%lld must not be negative", (long long)n);
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(ema) & 3) == 0 && (reinterpret_cast<uintptr_t>(p) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(rec) & 3) == 0, "asis_ema_update: misaligned pointer");
  if (n == 0) return ASIS_OK;
  if (asis_aligned16(ema) && asis_aligned16(p)) {
    hipLaunchKernelGGL(ema_update_vec_kernel, dim3(asis_grid(n / 4, QUADS_PER_TILE, GRID_CAP)), dim3(BLOCK), 0,
                       reinterpret_cast<hipStream_t>(stream), ema, p, n, rec);
  } else {
    hipLaunchKernelGGL(ema_update_scalar_kernel, dim3(asis_grid(n, BLOCK, GRID_CAP)), dim3(BLOCK), 0,
                       reinterpret_cast<hipStream_t>(stream), ema, p, n, rec);
  }
  ASIS_CHECK_LAUNCH("asis_ema_update");
  return ASIS_OK;
}
