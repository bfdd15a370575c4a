// Fused AdamW with global-norm gradient clipping over the flat fp32 parameter buckets (adaptersis_amd/optim.py: AdamW).
// Three kernels per step, no host synchronisation:
//   grad_sumsq    (per bucket)   sum of squares of the gradient bucket -> one fp32 partial per workgroup
//   adamw_prepare (once)         all partials -> norm, overflow decision, step count, clip coefficient, bias corrections
//   adamw_step    (per bucket)   torch.optim.AdamW (decoupled decay, amsgrad=False) with per-quad (lr_scale, weight_decay) groups
// Only adamw_prepare writes the guard and the record; the step kernels read them, so nothing races inside a grid.
#include <float.h>

#include "asis_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int GRID_CAP = 2048;     // 8 workgroups per CU on 256 CUs; the rest is the grid-stride loop
constexpr int MAX_GROUPS = 256;    // the group code is one byte
constexpr int MAX_PARTIALS = 1 << 20;

__device__ __forceinline__ float sumsq4(const float4 a, float s) {
  s = __builtin_fmaf(a.x, a.x, s);
  s = __builtin_fmaf(a.y, a.y, s);
  s = __builtin_fmaf(a.z, a.z, s);
  return __builtin_fmaf(a.w, a.w, s);
}

// partial[blockIdx.x] = sum of g^2 over the quads this workgroup visits: per-thread fp32 sum in loop order, wave butterfly, then
// the four wave sums in wave order.  No atomics and a grid that depends on n alone: the same bits from call to call.  An inf or
// NaN element (or a square that overflows) makes the partial non-finite, which is the overflow signal adamw_prepare reads.
__global__ __launch_bounds__(BLOCK) void grad_sumsq_kernel(const float4* __restrict__ g4, int64_t n4, float* __restrict__ partial) {
  __shared__ float red[BLOCK / 64];
  const int64_t stride = (int64_t)gridDim.x * BLOCK;
  int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  float s = 0.f;
  for (; i + 3 * stride < n4; i += 4 * stride) {
    const float4 a = g4[i], b = g4[i + stride], c = g4[i + 2 * stride], d = g4[i + 3 * stride];
    s = sumsq4(a, s); s = sumsq4(b, s); s = sumsq4(c, s); s = sumsq4(d, s);
  }
  for (; i < n4; i += stride) s = sumsq4(g4[i], s);
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup.  rec = {clip_coef, 1 / (1 - beta1^t), 1 / sqrt(1 - beta2^t), norm}; guard = {skip flag, skipped steps, t}.
// The sum runs in double in a fixed order: thread k takes partials k, k + 256, ... in index order, then a halving tree.
__global__ __launch_bounds__(BLOCK) void adamw_prepare_kernel(const float* __restrict__ partials, int n_partials, int* __restrict__ guard,
                                                              float* __restrict__ rec, float inv_scale, float max_norm, double beta1,
                                                              double beta2) {
  __shared__ double red[BLOCK];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += BLOCK) s += (double)partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = BLOCK / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double sum = red[0];
  if (!(sum <= DBL_MAX)) {   // inf or NaN: skip the step, keep t, the record and everything the step kernels would touch
    guard[0] = 1;
    guard[1] += 1;
    return;
  }
  guard[0] = 0;
  const int t = ++guard[2];
  const double norm = (double)inv_scale * sqrt(sum);
  double clip = 1.0;
  if (max_norm > 0.f) clip = fmin(1.0, (double)max_norm / (norm + 1e-6));   // torch.nn.utils.clip_grad_norm_
  rec[0] = (float)clip;
  rec[1] = (float)(1.0 / (1.0 - pow(beta1, (double)t)));
  rec[2] = (float)(1.0 / sqrt(1.0 - pow(beta2, (double)t)));
  rec[3] = (float)norm;
}

struct AdamConst {
  float b1, omb1, b2, omb2, eps, gscale, bc1, bc2s;
};

// one quad: lr_e = lr * lr_scale[code] and decay = 1 - lr_e * wd[code] come from the table.  v_sqrt_f32 and v_rcp_f32 (1 ulp each)
// instead of the IEEE sequences: they only touch the update lr_e m / (sqrt(v) + eps), whose 1e-7 relative error is 1e-7 of
// lr_e-sized steps — far below the rounding of p itself; m and v do not see them
__device__ __forceinline__ void adamw4(float4& p, const float4 g, float4& m, float4& v, const float2 grp, const AdamConst& c) {
  float* pp = reinterpret_cast<float*>(&p);
  float* mm = reinterpret_cast<float*>(&m);
  float* vv = reinterpret_cast<float*>(&v);
  const float* gg = reinterpret_cast<const float*>(&g);
  const float step = grp.x * c.bc1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float gs = gg[k] * c.gscale;
    const float mk = __builtin_fmaf(c.b1, mm[k], c.omb1 * gs);
    const float vk = __builtin_fmaf(c.b2, vv[k], c.omb2 * gs * gs);
    const float den = __builtin_fmaf(__builtin_amdgcn_sqrtf(vk), c.bc2s, c.eps);
    mm[k] = mk;
    vv[k] = vk;
    pp[k] = pp[k] * grp.y - step * (mk * __builtin_amdgcn_rcpf(den));
  }
}

// Two float4 per array in flight per lane, like sgd_vec_kernel; n is a multiple of 4, so there is no scalar tail.  Every workgroup
// owns ONE contiguous range of quads (a multiple of the 512 it covers per pass) and walks it front to back: with seven streams
// (p, m, v in and out, g in) a grid-stride walk, whose two quads per lane lie a whole grid (8 MB per array) apart, ran the ViT-L
// bucket at 4.3 TB/s; contiguous ranges on the same 2048-workgroup grid run it at 5.9 (scripts/bench_adamw.py).
constexpr int QUADS_PER_PASS = 2 * BLOCK;
__global__ __launch_bounds__(BLOCK) void adamw_step_kernel(float4* __restrict__ p4, const float4* __restrict__ g4, float4* __restrict__ m4,
                                                           float4* __restrict__ v4, const uint8_t* __restrict__ codes, int64_t n4,
                                                           const float* __restrict__ lr_scale, const float* __restrict__ wd, int n_groups,
                                                           double lr, float b1, float omb1, float b2, float omb2, float eps,
                                                           float inv_scale, const int* __restrict__ guard, const float* __restrict__ rec) {
  if (guard[0] != 0) return;   // uniform over the grid: written by adamw_prepare, the kernel before this one
  __shared__ float2 tab[MAX_GROUPS];
  for (int k = threadIdx.x; k < n_groups; k += BLOCK) {
    const double lr_e = lr * (double)lr_scale[k];
    tab[k] = make_float2((float)lr_e, (float)(1.0 - lr_e * (double)wd[k]));
  }
  __syncthreads();
  AdamConst c;
  c.b1 = b1; c.omb1 = omb1; c.b2 = b2; c.omb2 = omb2; c.eps = eps;
  c.gscale = inv_scale * rec[0];
  c.bc1 = rec[1];
  c.bc2s = rec[2];
  const int last = n_groups - 1;
  const int64_t per = ((n4 + gridDim.x - 1) / gridDim.x + QUADS_PER_PASS - 1) / QUADS_PER_PASS * QUADS_PER_PASS;
  const int64_t lo = (int64_t)blockIdx.x * per;
  const int64_t hi = lo + per < n4 ? lo + per : n4;   // hi <= lo for the workgroups past the end: they do nothing
  for (int64_t i = lo + threadIdx.x; i < hi; i += QUADS_PER_PASS) {
    const bool two = i + BLOCK < hi;
    const int64_t j = two ? i + BLOCK : i;             // the range's last pass may hold one quad for this lane: read it twice, store once
    const int ca = codes[i], cb = codes[j];
    float4 pa = p4[i], pb = p4[j];
    const float4 ga = g4[i], gb = g4[j];
    float4 ma = m4[i], mb = m4[j];
    float4 va = v4[i], vb = v4[j];
    adamw4(pa, ga, ma, va, tab[ca < last ? ca : last], c);   // a code past the table cannot read outside it
    adamw4(pb, gb, mb, vb, tab[cb < last ? cb : last], c);
    m4[i] = ma; v4[i] = va; p4[i] = pa;
    if (two) { m4[j] = mb; v4[j] = vb; p4[j] = pb; }
  }
}

}  // namespace

// workgroups (= partials written) of asis_grad_sumsq for n elements: four quads per lane and pass, capped
extern "C" int asis_grad_sumsq_blocks(int64_t n) { return asis_grid((n / 4 + 3) / 4, BLOCK, GRID_CAP); }

extern "C" int asis_grad_sumsq(void* stream, const float* g, int64_t n, float* partials) {
  ASIS_REQUIRE(g && partials, "asis_grad_sumsq: null pointer");
  ASIS_REQUIRE(n > 0 && n % 4 == 0, "asis_grad_sumsq: n=%lld must be a positive multiple of 4 (flat buckets are)", (long long)n);
  ASIS_REQUIRE(asis_aligned16(g) && (reinterpret_cast<uintptr_t>(partials) & 3) == 0,
               "asis_grad_sumsq: g must be 16-byte aligned (partials 4-byte)");
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(asis_grad_sumsq_blocks(n)), dim3(BLOCK), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<const float4*>(g), n / 4, partials);
  ASIS_CHECK_LAUNCH("asis_grad_sumsq");
  return ASIS_OK;
}

extern "C" int asis_adamw_prepare(void* stream, const float* partials, int n_partials, int32_t* guard, float* rec, float inv_scale,
                                  float max_norm, double beta1, double beta2) {
  ASIS_REQUIRE(partials && guard && rec, "asis_adamw_prepare: null pointer");
  ASIS_REQUIRE(n_partials >= 1 && n_partials <= MAX_PARTIALS, "asis_adamw_prepare: n_partials=%d must be in 1..%d", n_partials,
               MAX_PARTIALS);
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 3) == 0 && (reinterpret_cast<uintptr_t>(guard) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(rec) & 3) == 0, "asis_adamw_prepare: misaligned pointer");
  ASIS_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "asis_adamw_prepare: beta1=%g beta2=%g must be in [0, 1)",
               beta1, beta2);
  ASIS_REQUIRE(inv_scale > 0.f && inv_scale <= FLT_MAX, "asis_adamw_prepare: inv_scale=%g must be positive and finite", (double)inv_scale);
  ASIS_REQUIRE(max_norm == max_norm, "asis_adamw_prepare: max_norm is NaN (<= 0 turns clipping off)");
  hipLaunchKernelGGL(adamw_prepare_kernel, dim3(1), dim3(BLOCK), 0, reinterpret_cast<hipStream_t>(stream), partials, n_partials,
                     reinterpret_cast<int*>(guard), rec, inv_scale, max_norm, beta1, beta2);
  ASIS_CHECK_LAUNCH("asis_adamw_prepare");
  return ASIS_OK;
}

extern "C" int asis_adamw_step(void* stream, float* p, const float* g, float* m, float* v, int64_t n, const uint8_t* codes,
                               const float* lr_scale, const float* weight_decay, int n_groups, double lr, double beta1, double beta2,
                               double eps, float inv_scale, const int32_t* guard, const float* rec) {
  ASIS_REQUIRE(p && g && m && v && codes && lr_scale && weight_decay && guard && rec, "asis_adamw_step: null pointer");
  ASIS_REQUIRE(n > 0 && n % 4 == 0, "asis_adamw_step: n=%lld must be a positive multiple of 4 (flat buckets are)", (long long)n);
  ASIS_REQUIRE(asis_aligned16(p) && asis_aligned16(g) && asis_aligned16(m) && asis_aligned16(v),
               "asis_adamw_step: p, g, m and v must be 16-byte aligned");
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(lr_scale) & 3) == 0 && (reinterpret_cast<uintptr_t>(weight_decay) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(guard) & 3) == 0 && (reinterpret_cast<uintptr_t>(rec) & 3) == 0,
               "asis_adamw_step: misaligned table, guard or record");
  ASIS_REQUIRE(n_groups >= 1 && n_groups <= MAX_GROUPS, "asis_adamw_step: n_groups=%d must be in 1..%d", n_groups, MAX_GROUPS);
  ASIS_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "asis_adamw_step: beta1=%g beta2=%g must be in [0, 1)", beta1,
               beta2);
  ASIS_REQUIRE(eps > 0.0, "asis_adamw_step: eps=%g must be positive", eps);
  ASIS_REQUIRE(lr == lr && inv_scale > 0.f && inv_scale <= FLT_MAX, "asis_adamw_step: lr is NaN or inv_scale is not positive and finite");
  const int64_t n4 = n / 4;
  hipLaunchKernelGGL(adamw_step_kernel, dim3(asis_grid((n4 + 1) / 2, BLOCK, GRID_CAP)), dim3(BLOCK), 0,
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<float4*>(p), reinterpret_cast<const float4*>(g),
                     reinterpret_cast<float4*>(m), reinterpret_cast<float4*>(v), codes, n4, lr_scale, weight_decay, n_groups, lr,
                     (float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, inv_scale,
                     reinterpret_cast<const int*>(guard), rec);
  ASIS_CHECK_LAUNCH("asis_adamw_step");
  return ASIS_OK;
}
