// Stochastic depth of the unfrozen ViT in DINOv2's subset form (dinov2/layers/block.py:117-138): a residual branch runs on the
// kept samples only, so its GEMMs and its attention see a COMPACT [R', D] matrix and are untouched; the four memory-bound row
// kernels around them gain a sample indirection.  The arithmetic per row is the existing one (row_routines.h):
//   asis_layernorm_gather       LayerNorm of the kept samples' rows of the fp32 stream -> compact 16-bit        (norm1 / norm2)
//   asis_scaled_index_add       out = x, + alpha * res[compact row] on kept rows, fp32, plain stores            (the residual add)
//   asis_gather_cast_colsum     alpha * dres on kept rows -> compact 16-bit (+ column-sum partials)             (branch gradient)
//   asis_layernorm_bwd_scatter  dx = dres + LN^T(dy) on kept rows, dres elsewhere (+ d weight / d bias partials)
// Index table of one branch (int32 words, built on the host: adaptersis_amd/droppath.py), K kept of S stacked samples:
//   cpre[K + 1] | src[K] | alpha[K] (float) | spre[S + 1] | cpos[S] | salpha[S] (float)
// cpre / src / alpha: RowGather (row_routines.h); spre: full-stream row prefix of the samples, cpos: first compact row of a
// sample or -1 when it is dropped, salpha: its alpha.  Kept samples are distinct, so no two waves write one row: no atomics.
#include "asis_common.h"
#include "row_routines.h"

namespace {

struct DropTab {
  const int32_t *cpre, *src, *spre, *cpos;
  const float *alpha, *salpha;
  int K, S;
  __host__ __device__ DropTab(const int32_t* t, int K_, int S_) : K(K_), S(S_) {
    cpre = t;
    src = t + K_ + 1;
    alpha = reinterpret_cast<const float*>(t + 2 * K_ + 1);
    spre = t + 3 * K_ + 1;
    cpos = spre + S_ + 1;
    salpha = reinterpret_cast<const float*>(cpos + S_);
  }
  __device__ __forceinline__ RowGather gather() const { return RowGather{cpre, src, alpha, K}; }
  // sample of full-stream row r
  __device__ __forceinline__ int sample_of(int64_t r) const {
    int lo = 0, hi = S - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (spre[mid] <= r) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  }
};

template <typename T>
__global__ __launch_bounds__(256) void layernorm_gather_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                               const float* __restrict__ b, float eps, T* __restrict__ y, int64_t ldy,
                                                               const int32_t* __restrict__ tab, int K, int S, int64_t rows_c, int D) {
  const DropTab t(tab, K, S);
  const RowGather m = t.gather();
  const int lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows_c; row += (int64_t)gridDim.x * 4) {
    float unused;
    ln_row<T, false>(x + m(row, unused) * ldx, w, b, eps, y + row * ldy, D, lane);
  }
}

// COPY_ONLY: the dropped rows alone are written (out = x there): the second half of asis_layernorm_bwd_scatter
template <bool COPY_ONLY>
__global__ __launch_bounds__(256) void scaled_index_add_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ res,
                                                               int64_t ldres, float* __restrict__ out, int64_t ldo,
                                                               const int32_t* __restrict__ tab, int K, int S, int64_t rows, int D) {
  const DropTab t(tab, K, S);
  const int lane = threadIdx.x & 63;
  const int nchunk = D >> 2;
  for (int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (int64_t)gridDim.x * 4) {
    const int s = t.sample_of(row);
    const int cp = t.cpos[s];
    const float4* xr = reinterpret_cast<const float4*>(x + row * ldx);
    float4* o = reinterpret_cast<float4*>(out + row * ldo);
    if (cp < 0) {
#pragma unroll 4
      for (int c = lane; c < nchunk; c += 64) o[c] = xr[c];
    } else if (!COPY_ONLY) {
      const float a = t.salpha[s];
      const float4* rr = reinterpret_cast<const float4*>(res + ((int64_t)cp + (row - t.spre[s])) * ldres);
#pragma unroll 4
      for (int c = lane; c < nchunk; c += 64) {
        const float4 v = xr[c], r = rr[c];
        o[c] = make_float4(v.x + a * r.x, v.y + a * r.y, v.z + a * r.z, v.w + a * r.w);
      }
    }
  }
}

template <typename T, int MAXC>
__global__ __launch_bounds__(256) void gather_cast_colsum_kernel(const float* __restrict__ x, int64_t ldx, T* __restrict__ out, int64_t ldo,
                                                                 float* __restrict__ partial, const int32_t* __restrict__ tab, int K, int S,
                                                                 int64_t rows_c, int D, int rows_per_block) {
  const DropTab t(tab, K, S);
  cast_colsum_block<T, MAXC, true>(x, ldx, out, ldo, 1.f, partial, rows_c, D, rows_per_block, t.gather());
}

template <int MAXC>
__global__ __launch_bounds__(256) void layernorm_bwd_scatter_kernel(const float* __restrict__ dy, int64_t lddy, const float* __restrict__ x,
                                                                    int64_t ldx, const float* __restrict__ w, float eps,
                                                                    const float* __restrict__ res, int64_t ldr, float* __restrict__ dx,
                                                                    int64_t lddx, float* __restrict__ partial, const int32_t* __restrict__ tab,
                                                                    int K, int S, int64_t rows_c, int D, int rows_per_block) {
  const DropTab t(tab, K, S);
  ln_bwd_block<MAXC>(dy, lddy, x, ldx, w, eps, res, ldr, dx, lddx, partial, rows_c, D, rows_per_block, t.gather());
}

bool tab_ok(const int32_t* tab, int K, int S) { return tab && K >= 0 && S >= 1 && K <= S && (((uintptr_t)tab) & 3) == 0; }
bool rows_ok(int64_t r) { return r >= 0 && r < ((int64_t)1 << 31); }   // the tables hold rows as int32

}  // namespace

extern "C" int asis_layernorm_gather(void* stream, int dtype, const float* x, int64_t ldx, const float* w, const float* b, float eps,
                                     void* y, int64_t ldy, const int32_t* tab, int K, int S, int64_t rows_c, int D) {
  ASIS_REQUIRE(x && w && b && tab_ok(tab, K, S) && rows_ok(rows_c), "asis_layernorm_gather: bad arguments");
  ASIS_REQUIRE(D > 0 && D % 4 == 0 && D <= 256 * LN_MAXC, "asis_layernorm_gather: D=%d must be a multiple of 4 and <= %d", D, 256 * LN_MAXC);
  ASIS_REQUIRE(ldx % 4 == 0 && ldx >= D && ldy % 4 == 0 && ldy >= D, "asis_layernorm_gather: row strides must be multiples of 4 and >= D");
  ASIS_REQUIRE(asis_aligned16(x) && asis_aligned16(w) && asis_aligned16(b) && (((uintptr_t)y) & 7) == 0,
               "asis_layernorm_gather: pointers must be 16-byte aligned");
  ASIS_DT_OK(dtype, "asis_layernorm_gather");
  if (rows_c == 0 || K == 0) return ASIS_OK;
  ASIS_REQUIRE(y, "asis_layernorm_gather: null output");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int grid = asis_grid(rows_c, 4, 4096);
  if (int rc = asis_dispatch16(dtype, "asis_layernorm_gather", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((layernorm_gather_kernel<T>), dim3(grid), dim3(256), 0, s, x, ldx, w, b, eps, static_cast<T*>(y), ldy, tab, K, S,
                           rows_c, D);
      })) return rc;
  ASIS_CHECK_LAUNCH("asis_layernorm_gather");
  return ASIS_OK;
}

extern "C" int asis_scaled_index_add(void* stream, const float* x, int64_t ldx, const float* res, int64_t ldres, float* out, int64_t ldo,
                                     const int32_t* tab, int K, int S, int64_t rows, int D) {
  ASIS_REQUIRE(x && out && x != out && tab_ok(tab, K, S) && rows_ok(rows) && (res || K == 0), "asis_scaled_index_add: bad arguments");
  ASIS_REQUIRE(D > 0 && D % 4 == 0 && ldx % 4 == 0 && ldx >= D && ldo % 4 == 0 && ldo >= D && (!res || (ldres % 4 == 0 && ldres >= D)),
               "asis_scaled_index_add: D=%d and the row strides must be multiples of 4, strides >= D", D);
  ASIS_REQUIRE(asis_aligned16(x) && asis_aligned16(out) && (!res || asis_aligned16(res)), "asis_scaled_index_add: pointers must be 16-byte aligned");
  if (rows == 0) return ASIS_OK;
  hipLaunchKernelGGL((scaled_index_add_kernel<false>), dim3(asis_grid(rows, 4, 4096)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x,
                     ldx, res, ldres, out, ldo, tab, K, S, rows, D);
  ASIS_CHECK_LAUNCH("asis_scaled_index_add");
  return ASIS_OK;
}

extern "C" int asis_gather_cast_colsum(void* stream, int dtype, const float* x, int64_t ldx, void* out, int64_t ldo, float* partial,
                                       const int32_t* tab, int K, int S, int64_t rows_c, int D) {
  ASIS_REQUIRE(x && tab_ok(tab, K, S) && rows_ok(rows_c), "asis_gather_cast_colsum: bad arguments");
  ASIS_DT_OK(dtype, "asis_gather_cast_colsum");
  ASIS_REQUIRE(D > 0 && D % 4 == 0 && D <= LN_MAXC * 256 && ldx % 4 == 0 && ldx >= D && ldo % 4 == 0 && ldo >= D,
               "asis_gather_cast_colsum: D=%d must be a multiple of 4, <= %d; row strides multiples of 4", D, LN_MAXC * 256);
  ASIS_REQUIRE(asis_aligned16(x) && (((uintptr_t)out) & 7) == 0 && (!partial || asis_aligned16(partial)),
               "asis_gather_cast_colsum: pointers must be 16-byte aligned");
  if (rows_c == 0 || K == 0) return ASIS_OK;
  ASIS_REQUIRE(out, "asis_gather_cast_colsum: null output");
  const int nblk = asis_rowblock_nblk(rows_c);
  const int rpb = (int)((rows_c + nblk - 1) / nblk);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = asis_dispatch16(dtype, "asis_gather_cast_colsum", [&](auto t) {
        using T = decltype(t);
        if (D <= 1024) hipLaunchKernelGGL((gather_cast_colsum_kernel<T, 4>), dim3(nblk), dim3(256), 0, s, x, ldx, static_cast<T*>(out), ldo, partial, tab, K, S, rows_c, D, rpb);
        else hipLaunchKernelGGL((gather_cast_colsum_kernel<T, LN_MAXC>), dim3(nblk), dim3(256), 0, s, x, ldx, static_cast<T*>(out), ldo, partial, tab, K, S, rows_c, D, rpb);
      })) return rc;
  ASIS_CHECK_LAUNCH("asis_gather_cast_colsum");
  return ASIS_OK;
}

extern "C" int asis_layernorm_bwd_scatter(void* stream, const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* w, float eps,
                                          const float* res, int64_t ldr, float* dx, int64_t lddx, float* partial, const int32_t* tab, int K,
                                          int S, int64_t rows, int64_t rows_c, int D) {
  ASIS_REQUIRE(x && w && res && dx && dx != res && tab_ok(tab, K, S) && rows_ok(rows) && rows_ok(rows_c) && rows_c <= rows,
               "asis_layernorm_bwd_scatter: bad arguments");
  ASIS_REQUIRE(D > 0 && D % 4 == 0 && D <= LN_MAXC * 256, "asis_layernorm_bwd_scatter: D=%d must be a multiple of 4, <= %d", D, LN_MAXC * 256);
  ASIS_REQUIRE(lddy % 4 == 0 && ldx % 4 == 0 && ldx >= D && lddx % 4 == 0 && lddx >= D && ldr % 4 == 0 && ldr >= D,
               "asis_layernorm_bwd_scatter: row strides must be multiples of 4 and >= D");
  ASIS_REQUIRE(asis_aligned16(x) && asis_aligned16(w) && asis_aligned16(res) && asis_aligned16(dx) && (!dy || asis_aligned16(dy)) &&
               (!partial || asis_aligned16(partial)), "asis_layernorm_bwd_scatter: pointers must be 16-byte aligned");
  if (rows == 0) return ASIS_OK;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the dropped rows: dx = dres (disjoint from the rows the second launch writes)
  hipLaunchKernelGGL((scaled_index_add_kernel<true>), dim3(asis_grid(rows, 4, 4096)), dim3(256), 0, s, res, ldr, static_cast<const float*>(nullptr),
                     (int64_t)0, dx, lddx, tab, K, S, rows, D);
  ASIS_CHECK_LAUNCH("asis_layernorm_bwd_scatter");
  if (rows_c == 0 || K == 0) return ASIS_OK;
  ASIS_REQUIRE(dy && partial && lddy >= D, "asis_layernorm_bwd_scatter: kept rows need dy and partial");
  const int nblk = asis_rowblock_nblk(rows_c);
  const int rpb = (int)((rows_c + nblk - 1) / nblk);
#define ASIS_LNBS(MAXC)                                                                                                                   \
  hipLaunchKernelGGL((layernorm_bwd_scatter_kernel<MAXC>), dim3(nblk), dim3(256), 0, s, dy, lddy, x, ldx, w, eps, res, ldr, dx, lddx, partial, \
                     tab, K, S, rows_c, D, rpb)
  if (D <= 1024) ASIS_LNBS(4);
  else if (D <= 1536) ASIS_LNBS(6);
  else ASIS_LNBS(LN_MAXC);
#undef ASIS_LNBS
  ASIS_CHECK_LAUNCH("asis_layernorm_bwd_scatter");
  return ASIS_OK;
}
