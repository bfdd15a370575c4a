// Row / elementwise backward kernels of the DINOv2 block (dinov2/layers/block.py:89-114), all HBM-bound streaming:
//   LayerNorm backward            nn.LayerNorm(eps=1e-6), block.py:63,75
//   GELU (erf) forward / backward on 16-bit operands (mlp.py:35) — the training forward keeps the pre-activation
//   column sums of a 16-bit matrix (bias gradients of qkv / fc1)
//   LayerScale + Linear finish    out = x + gamma * (A W^T + b): from G = dout^T A (unscaled wgrad GEMM) and
//                                 cs = colsum(dout):  dW = gamma G,  db = gamma cs,  dgamma = rowsum(W * G) + b cs
// One wave64 per row for the row kernels, 16-byte accesses, fp32 arithmetic.
#include "asis_common.h"
#include "row_routines.h"   // LN_MAXC, ln_bwd_block, cast_colsum_block

namespace {

// dx[row] = (res ? res[row] : 0) + rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * w
// partial[blk][0][c] = sum_rows dy * xhat (d weight),  partial[blk][1][c] = sum_rows dy (d bias)
// Each block owns ROWS_PER_BLOCK consecutive rows, 4 waves striding over them; statistics are recomputed from x (row_routines.h).
template <int MAXC>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, int64_t lddy,
                                                            const float* __restrict__ x, int64_t ldx,
                                                            const float* __restrict__ w, float eps,
                                                            const float* __restrict__ res, int64_t ldr,
                                                            float* __restrict__ dx, int64_t lddx,
                                                            float* __restrict__ partial, int64_t rows, int D,
                                                            int rows_per_block) {
  ln_bwd_block<MAXC>(dy, lddy, x, ldx, w, eps, res, ldr, dx, lddx, partial, rows, D, rows_per_block, RowIdentity());
}

// exact (libm erff) derivative is used in the backward: one pass, not in a GEMM epilogue
template <typename T, bool BWD>
__global__ __launch_bounds__(256) void gelu16_kernel(const T* __restrict__ pre, const T* __restrict__ dpost, T* __restrict__ out,
                                                     int64_t n8) {
  typedef typename T16<T>::v8 v8;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (int64_t)gridDim.x * blockDim.x) {
    const v8 p = reinterpret_cast<const v8*>(pre)[i];
    v8 o;
    if (BWD) {
      const v8 g = reinterpret_cast<const v8*>(dpost)[i];
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = (T)((float)g[k] * gelu_erf_grad((float)p[k]));
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) o[k] = (T)gelu_erf((float)p[k]);
    }
    reinterpret_cast<v8*>(out)[i] = o;
  }
}

// SwiGLU gate backward (swiglu_ffn.py:30-34): h = silu(x1) * x2 with x12 = [x1 | x2] fp32 [R, 2 Hd], dh 16-bit [R, Hd]
//   d x1 = dh * x2 * sig(x1) * (1 + x1 (1 - sig(x1))),  d x2 = dh * silu(x1)      -> 16-bit [R, 2 Hd]
template <typename T>
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const float* __restrict__ x12, const T* __restrict__ dh,
                                                         T* __restrict__ dx12, int64_t R, int Hd) {
  const int cpr = Hd >> 2;
  const int64_t total = R * cpr;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cpr;
    const int c = (int)(i - r * cpr);
    const float4 a = reinterpret_cast<const float4*>(x12 + r * 2 * Hd)[c];
    const float4 b = reinterpret_cast<const float4*>(x12 + r * 2 * Hd + Hd)[c];
    const uint2 gw = reinterpret_cast<const uint2*>(dh + r * Hd)[c];
    float g[4];
    unpack2<T>(gw.x, g[0], g[1]);
    unpack2<T>(gw.y, g[2], g[3]);
    const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
    float d1[4], d2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float sg = 1.f / (1.f + __expf(-av[k]));
      d1[k] = g[k] * bv[k] * sg * (1.f + av[k] * (1.f - sg));
      d2[k] = g[k] * av[k] * sg;
    }
    uint2 o;
    o.x = pack2<T>(d1[0], d1[1]);
    o.y = pack2<T>(d1[2], d1[3]);
    reinterpret_cast<uint2*>(dx12 + r * 2 * Hd)[c] = o;
    o.x = pack2<T>(d2[0], d2[1]);
    o.y = pack2<T>(d2[2], d2[3]);
    reinterpret_cast<uint2*>(dx12 + r * 2 * Hd + Hd)[c] = o;
  }
}

// partial[blk][c] = sum over the block's rows of x[r, c] (16-bit input, fp32 sums); threads run along columns (8 per thread)
template <typename T>
__global__ __launch_bounds__(256) void colsum16_kernel(const T* __restrict__ x, int64_t ld, float* __restrict__ partial,
                                                       int64_t rows, int C, int rows_per_block) {
  typedef typename T16<T>::v8 v8;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  for (int c8 = blockIdx.y * blockDim.x + threadIdx.x; c8 < (C >> 3); c8 += gridDim.y * blockDim.x) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int64_t r = r0;
    for (; r + 3 < r1; r += 4) {   // four independent 16-byte loads in flight per thread
      v8 v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const v8*>(x + (r + j) * ld + c8 * 8);
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) s[k] += (float)v[j][k];
    }
    for (; r < r1; ++r) {
      const v8 v = *reinterpret_cast<const v8*>(x + r * ld + c8 * 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) s[k] += (float)v[k];
    }
    float4* o = reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * C + c8 * 8);
    o[0] = make_float4(s[0], s[1], s[2], s[3]);
    o[1] = make_float4(s[4], s[5], s[6], s[7]);
  }
}

// fp32 variant (column sums of the residual-stream gradient)
__global__ __launch_bounds__(256) void colsum32_kernel(const float* __restrict__ x, int64_t ld, float* __restrict__ partial,
                                                       int64_t rows, int C, int rows_per_block) {
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  for (int c4 = blockIdx.y * blockDim.x + threadIdx.x; c4 < (C >> 2); c4 += gridDim.y * blockDim.x) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int64_t r = r0; r < r1; ++r) {
      const float4 v = *reinterpret_cast<const float4*>(x + r * ld + c4 * 4);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * C + c4 * 4) = s;
  }
}

// out16[r, :] = (T)(scale * x[r, :]) and partial[blk][c] = sum over the block's rows of x[r, c]: the 16-bit GEMM operand of
// a residual-stream gradient and its column sums (LayerScale / bias gradients) in one read of the fp32 rows
template <typename T, int MAXC>
__global__ __launch_bounds__(256) void cast_colsum_kernel(const float* __restrict__ x, int64_t ldx, T* __restrict__ out,
                                                          int64_t ldo, float scale, float* __restrict__ partial,
                                                          int64_t rows, int D, int rows_per_block) {
  cast_colsum_block<T, MAXC, false>(x, ldx, out, ldo, scale, partial, rows, D, rows_per_block, RowIdentity());
}

// one wave per output feature n: dW[n,:] = gs * gamma[n] * G[n,:];  dgamma[n] = gs * (sum_k W[n,k] G[n,k] + b[n] cs[n]);
// db[n] = gs * gamma[n] * cs[n]     (gs = 1 / loss scale; gamma NULL = plain Linear: dW = gs G, db = gs cs)
__global__ __launch_bounds__(256) void ls_linear_finish_kernel(const float* __restrict__ G, const float* __restrict__ Wt,
                                                               const float* __restrict__ bias, const float* __restrict__ gamma,
                                                               const float* __restrict__ cs, float gs, float* __restrict__ dW,
                                                               float* __restrict__ db, float* __restrict__ dgamma, int N,
                                                               int K) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const float ga = gamma ? gamma[n] : 1.f;
  const float4* g4 = reinterpret_cast<const float4*>(G + (int64_t)n * K);
  const float4* w4 = reinterpret_cast<const float4*>(Wt + (int64_t)n * K);
  float4* o4 = reinterpret_cast<float4*>(dW + (int64_t)n * K);
  float dot = 0.f;
  const float sc = gs * ga;
  for (int c = lane; c < (K >> 2); c += 64) {
    const float4 g = g4[c];
    if (gamma) {
      const float4 w = w4[c];
      dot += (g.x * w.x + g.y * w.y) + (g.z * w.z + g.w * w.w);
    }
    o4[c] = make_float4(g.x * sc, g.y * sc, g.z * sc, g.w * sc);
  }
  if (gamma) dot = wave_sum(dot);
  if (lane == 0) {
    const float c = cs ? cs[n] : 0.f;
    if (db) db[n] = sc * c;
    if (gamma && dgamma) dgamma[n] = gs * (dot + (bias ? bias[n] : 0.f) * c);
  }
}

}  // namespace

extern "C" int asis_rowblock_nblk(int64_t rows) {
  return asis_grid(rows, 32, 2048);
}

extern "C" int asis_layernorm_bwd(void* stream, const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* w,
                                  float eps, const float* res, int64_t ldr, float* dx, int64_t lddx, float* partial,
                                  int64_t rows, int D) {
  ASIS_REQUIRE(dy && x && w && dx && partial, "asis_layernorm_bwd: null pointer");
  ASIS_REQUIRE(D > 0 && D % 4 == 0 && D <= LN_MAXC * 256, "asis_layernorm_bwd: D=%d must be a multiple of 4, <= %d", D, LN_MAXC * 256);
  ASIS_REQUIRE(lddy % 4 == 0 && ldx % 4 == 0 && lddx % 4 == 0 && (!res || ldr % 4 == 0), "asis_layernorm_bwd: row strides must be multiples of 4");
  ASIS_REQUIRE(rows > 0, "asis_layernorm_bwd: no rows");
  const int nblk = asis_rowblock_nblk(rows);
  const int rpb = (int)((rows + nblk - 1) / nblk);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (D <= 1024)
    hipLaunchKernelGGL((layernorm_bwd_kernel<4>), dim3(nblk), dim3(256), 0, s, dy, lddy, x, ldx, w, eps, res, ldr, dx, lddx,
                       partial, rows, D, rpb);
  else if (D <= 1536)
    hipLaunchKernelGGL((layernorm_bwd_kernel<6>), dim3(nblk), dim3(256), 0, s, dy, lddy, x, ldx, w, eps, res, ldr, dx, lddx,
                       partial, rows, D, rpb);
  else
    hipLaunchKernelGGL((layernorm_bwd_kernel<LN_MAXC>), dim3(nblk), dim3(256), 0, s, dy, lddy, x, ldx, w, eps, res, ldr, dx,
                       lddx, partial, rows, D, rpb);
  ASIS_CHECK_LAUNCH("asis_layernorm_bwd");
  return ASIS_OK;
}

namespace {
// erf-GELU of an fp32 pre-activation into a split-precision 16-bit operand pair (hi, lo = rounding residual of hi)
template <typename T>
__global__ __launch_bounds__(256) void gelu_split_kernel(const float* __restrict__ x, T* __restrict__ hi, T* __restrict__ lo, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(x)[i];
    float g0 = v.x, g1 = v.y, g2 = v.z, g3 = v.w;
    gelu_erf4(g0, g1, g2, g3);
    uint2 h;
    h.x = pack2<T>(g0, g1); h.y = pack2<T>(g2, g3);
    reinterpret_cast<uint2*>(hi)[i] = h;
    if (lo) {
      uint2 l;
      l.x = pack2<T>(lo_part<T>(g0), lo_part<T>(g1)); l.y = pack2<T>(lo_part<T>(g2), lo_part<T>(g3));
      reinterpret_cast<uint2*>(lo)[i] = l;
    }
  }
}
}  // namespace

extern "C" int asis_gelu_split(void* stream, int dtype, const float* x, void* hi, void* lo, int64_t n) {
  ASIS_REQUIRE(x && hi && n > 0 && n % 4 == 0, "asis_gelu_split: bad arguments (n %% 4 == 0)");
  ASIS_DT_OK(dtype, "asis_gelu_split");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int g = asis_grid(n / 4, 256, 65535 * 4);
  if (int rc = asis_dispatch16(dtype, "asis_gelu_split", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((gelu_split_kernel<T>), dim3(g), dim3(256), 0, s, x, static_cast<T*>(hi), static_cast<T*>(lo), n / 4);
      })) return rc;
  ASIS_CHECK_LAUNCH("asis_gelu_split");
  return ASIS_OK;
}

extern "C" int asis_gelu16(void* stream, int dtype, const void* pre, const void* dpost, void* out, int64_t n) {
  ASIS_REQUIRE(pre && out && n > 0 && n % 8 == 0, "asis_gelu16: bad arguments (n %% 8 == 0)");
  ASIS_DT_OK(dtype, "asis_gelu16");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t n8 = n / 8;
  const int g = asis_grid(n8, 256, 65535 * 4);
  if (int rc = asis_dispatch16(dtype, "asis_gelu16", [&](auto t) {
        using T = decltype(t);
        if (dpost) hipLaunchKernelGGL((gelu16_kernel<T, true>), dim3(g), dim3(256), 0, s, static_cast<const T*>(pre), static_cast<const T*>(dpost), static_cast<T*>(out), n8);
        else hipLaunchKernelGGL((gelu16_kernel<T, false>), dim3(g), dim3(256), 0, s, static_cast<const T*>(pre), static_cast<const T*>(nullptr), static_cast<T*>(out), n8);
      })) return rc;
  ASIS_CHECK_LAUNCH("asis_gelu16");
  return ASIS_OK;
}

extern "C" int asis_swiglu_bwd(void* stream, int dtype, const float* x12, const void* dh, void* dx12, int64_t R, int Hd) {
  ASIS_REQUIRE(x12 && dh && dx12 && R > 0 && Hd > 0 && Hd % 4 == 0, "asis_swiglu_bwd: bad arguments (Hd %% 4 == 0)");
  ASIS_DT_OK(dtype, "asis_swiglu_bwd");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int g = asis_grid(R * (Hd / 4), 256, 65535 * 4);
  if (int rc = asis_dispatch16(dtype, "asis_swiglu_bwd", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((swiglu_bwd_kernel<T>), dim3(g), dim3(256), 0, s, x12, static_cast<const T*>(dh), static_cast<T*>(dx12), R, Hd);
      })) return rc;
  ASIS_CHECK_LAUNCH("asis_swiglu_bwd");
  return ASIS_OK;
}

extern "C" int asis_colsum(void* stream, int dtype, const void* x, int64_t ld, float* partial, int64_t rows, int C) {
  ASIS_REQUIRE(x && partial && rows > 0, "asis_colsum: bad arguments");
  if (dtype != ASIS_F32) ASIS_DT_OK(dtype, "asis_colsum");
  ASIS_REQUIRE(C > 0 && C % 8 == 0 && ld % 8 == 0 && ld >= C, "asis_colsum: C=%d and ld must be multiples of 8", C);
  const int nblk = asis_rowblock_nblk(rows);
  const int rpb = (int)((rows + nblk - 1) / nblk);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // gridDim.y walks the columns (256 threads x 8 / 4 columns each), so few-rows x very-wide inputs (the batch sum of a
  // [B, tokens*D] gradient) still fill the chip
  const int per = dtype == ASIS_F32 ? 4 : 8;
  const int gy = asis_grid(C / per, 256, 4096);
  if (dtype == ASIS_F32)  // the float branch stays explicit: the dispatcher knows the two 16-bit types only
    hipLaunchKernelGGL(colsum32_kernel, dim3(nblk, gy), dim3(256), 0, s, static_cast<const float*>(x), ld, partial, rows, C, rpb);
  else if (int rc = asis_dispatch16(dtype, "asis_colsum", [&](auto t) {
             using T = decltype(t);
             hipLaunchKernelGGL((colsum16_kernel<T>), dim3(nblk, gy), dim3(256), 0, s, static_cast<const T*>(x), ld, partial, rows, C, rpb);
           })) return rc;
  ASIS_CHECK_LAUNCH("asis_colsum");
  return ASIS_OK;
}

extern "C" int asis_cast_colsum(void* stream, int dtype, const float* x, int64_t ldx, void* out, int64_t ldo, float scale,
                                float* partial, int64_t rows, int D) {
  ASIS_REQUIRE(x && out && partial && rows > 0, "asis_cast_colsum: bad arguments");
  ASIS_DT_OK(dtype, "asis_cast_colsum");
  ASIS_REQUIRE(D > 0 && D % 4 == 0 && D <= LN_MAXC * 256 && ldx % 4 == 0 && ldo % 4 == 0 && ldo >= D,
               "asis_cast_colsum: D=%d must be a multiple of 4, <= %d; row strides multiples of 4", D, LN_MAXC * 256);
  const int nblk = asis_rowblock_nblk(rows);
  const int rpb = (int)((rows + nblk - 1) / nblk);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = asis_dispatch16(dtype, "asis_cast_colsum", [&](auto t) {
        using T = decltype(t);
        if (D <= 1024) hipLaunchKernelGGL((cast_colsum_kernel<T, 4>), dim3(nblk), dim3(256), 0, s, x, ldx, static_cast<T*>(out), ldo, scale, partial, rows, D, rpb);
        else hipLaunchKernelGGL((cast_colsum_kernel<T, LN_MAXC>), dim3(nblk), dim3(256), 0, s, x, ldx, static_cast<T*>(out), ldo, scale, partial, rows, D, rpb);
      })) return rc;
  ASIS_CHECK_LAUNCH("asis_cast_colsum");
  return ASIS_OK;
}

extern "C" int asis_ls_linear_finish(void* stream, const float* G, const float* W, const float* bias, const float* gamma,
                                     const float* cs, float grad_scale, float* dW, float* db, float* dgamma, int N, int K) {
  ASIS_REQUIRE(G && dW && N > 0 && K > 0 && K % 4 == 0, "asis_ls_linear_finish: bad arguments (K %% 4 == 0)");
  ASIS_REQUIRE(!gamma || W, "asis_ls_linear_finish: gamma needs the weight");
  hipLaunchKernelGGL(ls_linear_finish_kernel, dim3((N + 3) / 4), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), G, W, bias,
                     gamma, cs, grad_scale, dW, db, dgamma, N, K);
  ASIS_CHECK_LAUNCH("asis_ls_linear_finish");
  return ASIS_OK;
}
