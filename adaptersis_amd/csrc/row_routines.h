// Per-row device routines of the HBM-bound row kernels, shared by their plain entry points (norm.hip: asis_layernorm,
// vit_bwd.hip: asis_layernorm_bwd / asis_cast_colsum) and by the sample-indirected forms of stochastic depth (droppath.hip).
// One wave64 per row, 16-byte accesses, fp32 arithmetic.  A ``Map`` turns the row a wave works on into the row of the fp32
// residual stream it reads or writes (and may replace the row's scale): RowIdentity for the plain kernels — it compiles to
// nothing, so those entry points compute exactly what they did with the code inline —, RowGather for a compact matrix that
// holds the rows of the kept samples only.
#pragma once
#include "asis_common.h"

namespace {

constexpr int LN_MAXC = 8;  // float4 chunks per lane -> D <= 2048

struct RowIdentity {
  __device__ __forceinline__ int64_t operator()(int64_t r, float&) const { return r; }
};

// compact row r of a dropped branch -> its row of the full stream.  cpre[K + 1]: compact row prefix of the K kept samples
// (cpre[0] = 0, cpre[K] = R'), src[K]: first full-stream row of each, alpha[K]: its branch scale (b / kept, or 1 / (1 - p)).
struct RowGather {
  const int32_t* __restrict__ cpre;
  const int32_t* __restrict__ src;
  const float* __restrict__ alpha;
  int K;
  __device__ __forceinline__ int64_t operator()(int64_t r, float& scale) const {
    int lo = 0, hi = K - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (cpre[mid] <= r) lo = mid;
      else hi = mid - 1;
    }
    scale = alpha[lo];
    return (int64_t)src[lo] + (r - cpre[lo]);
  }
};

// LayerNorm of one row by one wave: xr -> yr (float when OUT_F32, else T)
template <typename T, bool OUT_F32>
__device__ __forceinline__ void ln_row(const float* __restrict__ xrow, const float* __restrict__ w, const float* __restrict__ b,
                                       float eps, void* __restrict__ yrow, int D, int lane) {
  const int nchunk = D >> 2;
  const float4* xr = reinterpret_cast<const float4*>(xrow);
  float4 v[LN_MAXC];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) {
      v[i] = xr[c];
      s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) {
      const float a0 = v[i].x - mean, a1 = v[i].y - mean, a2 = v[i].z - mean, a3 = v[i].w - mean;
      q += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  const float4* w4 = reinterpret_cast<const float4*>(w);
  const float4* b4 = reinterpret_cast<const float4*>(b);
#pragma unroll
  for (int i = 0; i < LN_MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < nchunk) {
      const float4 ww = w4[c], bb = b4[c];
      const float o0 = (v[i].x - mean) * rstd * ww.x + bb.x;
      const float o1 = (v[i].y - mean) * rstd * ww.y + bb.y;
      const float o2 = (v[i].z - mean) * rstd * ww.z + bb.z;
      const float o3 = (v[i].w - mean) * rstd * ww.w + bb.w;
      if (OUT_F32) {
        reinterpret_cast<float4*>(yrow)[c] = make_float4(o0, o1, o2, o3);
      } else {
        uint2 p;
        p.x = pack2<T>(o0, o1);
        p.y = pack2<T>(o2, o3);
        reinterpret_cast<uint2*>(yrow)[c] = p;
      }
    }
  }
}

// LayerNorm backward of the rows [blockIdx.x * rows_per_block, ...) of dy by one 256-thread block:
// dx[m(row)] = (res ? res[m(row)] : 0) + rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy[row] * w, statistics from x[m(row)]
// partial[blk][0][c] = sum_rows dy * xhat (d weight),  partial[blk][1][c] = sum_rows dy (d bias)
// 4 waves stride over the block's rows; x, res and dx are addressed through the map, dy by the row itself.
template <int MAXC, typename Map>
__device__ __forceinline__ void ln_bwd_block(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ x, int64_t ldx,
                                             const float* __restrict__ w, float eps, const float* __restrict__ res, int64_t ldr,
                                             float* __restrict__ dx, int64_t lddx, float* __restrict__ partial, int64_t rows, int D,
                                             int rows_per_block, const Map m) {
  __shared__ float red[3][2][MAXC * 64 * 4];  // waves 1..3 park their column sums here
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nchunk = D >> 2;
  const float4* w4 = reinterpret_cast<const float4*>(w);
  float4 gw[MAXC], gb[MAXC], ww[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) {
    gw[i] = gb[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int c = lane + 64 * i;
    ww[i] = c < nchunk ? w4[c] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  const float invD = 1.0f / (float)D;
  // the next row's loads (x, dy, residual) are issued before this row's three wave reductions: two rows in flight per wave
  constexpr bool PF = MAXC <= 6;   // 6 x MAXC float4 of row data + 3 x MAXC of sums / weight must fit 256 VGPRs
  float4 v[MAXC], g[MAXC], e[MAXC];
  int64_t mrow = 0;                // m(row) of the row held in v / g / e
  auto load_row = [&](int64_t row, float4* vv, float4* gg, float4* ee) -> int64_t {
    float unused = 1.f;
    const int64_t sr = m(row, unused);
    const float4* xr = reinterpret_cast<const float4*>(x + sr * ldx);
    const float4* gr = reinterpret_cast<const float4*>(dy + row * lddy);
    const float4* rr = res ? reinterpret_cast<const float4*>(res + sr * ldr) : nullptr;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunk) {
        vv[i] = xr[c];
        gg[i] = gr[c];
        if (rr) ee[i] = rr[c];
      }
    }
    return sr;
  };
  int64_t row = r0 + wid;
  if constexpr (PF) {
    if (row < r1) mrow = load_row(row, v, g, e);
  }
  for (; row < r1; row += 4) {
    float4 vn[PF ? MAXC : 1], gn[PF ? MAXC : 1], en[PF ? MAXC : 1];
    int64_t mnext = 0;
    if constexpr (PF) {
      if (row + 4 < r1) mnext = load_row(row + 4, vn, gn, en);
    } else {
      mrow = load_row(row, v, g, e);
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunk) s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_sum(s) * invD;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunk) {
        v[i].x -= mean; v[i].y -= mean; v[i].z -= mean; v[i].w -= mean;
        q += (v[i].x * v[i].x + v[i].y * v[i].y) + (v[i].z * v[i].z + v[i].w * v[i].w);
      }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) * invD + eps);
    float a = 0.f, bq = 0.f;  // sum g, sum g*xhat
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunk) {
        v[i].x *= rstd; v[i].y *= rstd; v[i].z *= rstd; v[i].w *= rstd;  // xhat
        gw[i].x += g[i].x * v[i].x; gw[i].y += g[i].y * v[i].y; gw[i].z += g[i].z * v[i].z; gw[i].w += g[i].w * v[i].w;
        gb[i].x += g[i].x; gb[i].y += g[i].y; gb[i].z += g[i].z; gb[i].w += g[i].w;
        g[i].x *= ww[i].x; g[i].y *= ww[i].y; g[i].z *= ww[i].z; g[i].w *= ww[i].w;
        a += (g[i].x + g[i].y) + (g[i].z + g[i].w);
        bq += (g[i].x * v[i].x + g[i].y * v[i].y) + (g[i].z * v[i].z + g[i].w * v[i].w);
      }
    }
    a = wave_sum(a) * invD;
    bq = wave_sum(bq) * invD;
    float4* o = reinterpret_cast<float4*>(dx + mrow * lddx);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunk) {
        float4 t;
        t.x = rstd * (g[i].x - a - v[i].x * bq);
        t.y = rstd * (g[i].y - a - v[i].y * bq);
        t.z = rstd * (g[i].z - a - v[i].z * bq);
        t.w = rstd * (g[i].w - a - v[i].w * bq);
        if (res) {
          t.x += e[i].x; t.y += e[i].y; t.z += e[i].z; t.w += e[i].w;
        }
        o[c] = t;
      }
    }
    if constexpr (PF) {
#pragma unroll
      for (int i = 0; i < MAXC; ++i) {
        v[i] = vn[i];
        g[i] = gn[i];
        e[i] = en[i];
      }
      mrow = mnext;
    }
  }
  // column sums over the block's rows: waves 1..3 -> LDS -> wave 0 adds and writes
  if (wid > 0) {
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      reinterpret_cast<float4*>(red[wid - 1][0])[i * 64 + lane] = gw[i];
      reinterpret_cast<float4*>(red[wid - 1][1])[i * 64 + lane] = gb[i];
    }
  }
  __syncthreads();
  if (wid == 0) {
    float4* pw = reinterpret_cast<float4*>(partial + ((int64_t)blockIdx.x * 2 + 0) * D);
    float4* pb = reinterpret_cast<float4*>(partial + ((int64_t)blockIdx.x * 2 + 1) * D);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunk) {
        float4 sw = gw[i], sb = gb[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float4 t = reinterpret_cast<const float4*>(red[k][0])[i * 64 + lane];
          const float4 u = reinterpret_cast<const float4*>(red[k][1])[i * 64 + lane];
          sw.x += t.x; sw.y += t.y; sw.z += t.z; sw.w += t.w;
          sb.x += u.x; sb.y += u.y; sb.z += u.z; sb.w += u.w;
        }
        pw[c] = sw;
        pb[c] = sb;
      }
    }
  }
}

// out16[row, :] = (T)(scale * x[m(row), :]) for the rows [blockIdx.x * rows_per_block, ...) and partial[blk][c] = the column
// sums over those rows: of x itself (SCALED_SUM false: asis_cast_colsum) or of scale * x with the row's own scale from the
// map (SCALED_SUM true: the branch gradient of stochastic depth).  partial NULL: the cast alone.
template <typename T, int MAXC, bool SCALED_SUM, typename Map>
__device__ __forceinline__ void cast_colsum_block(const float* __restrict__ x, int64_t ldx, T* __restrict__ out, int64_t ldo,
                                                  float scale, float* __restrict__ partial, int64_t rows, int D, int rows_per_block,
                                                  const Map m) {
  __shared__ float red[3][MAXC * 64 * 4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nchunk = D >> 2;
  float4 acc[MAXC];
#pragma unroll
  for (int i = 0; i < MAXC; ++i) acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  int64_t r1 = r0 + rows_per_block;
  if (r1 > rows) r1 = rows;
  for (int64_t row = r0 + wid; row < r1; row += 4) {
    const float4* xr = reinterpret_cast<const float4*>(x + m(row, scale) * ldx);
    uint2* o = reinterpret_cast<uint2*>(out + row * ldo);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunk) {
        const float4 v = xr[c];
        if (SCALED_SUM) {
          acc[i].x += v.x * scale; acc[i].y += v.y * scale; acc[i].z += v.z * scale; acc[i].w += v.w * scale;
        } else {
          acc[i].x += v.x; acc[i].y += v.y; acc[i].z += v.z; acc[i].w += v.w;
        }
        uint2 p;
        p.x = pack2<T>(v.x * scale, v.y * scale);
        p.y = pack2<T>(v.z * scale, v.w * scale);
        o[c] = p;
      }
    }
  }
  if (!partial) return;   // uniform over the block
  if (wid > 0) {
#pragma unroll
    for (int i = 0; i < MAXC; ++i) reinterpret_cast<float4*>(red[wid - 1])[i * 64 + lane] = acc[i];
  }
  __syncthreads();
  if (wid == 0) {
    float4* pw = reinterpret_cast<float4*>(partial + (int64_t)blockIdx.x * D);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
      const int c = lane + 64 * i;
      if (c < nchunk) {
        float4 s = acc[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float4 t = reinterpret_cast<const float4*>(red[k])[i * 64 + lane];
          s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        pw[c] = s;
      }
    }
  }
}

}  // namespace
