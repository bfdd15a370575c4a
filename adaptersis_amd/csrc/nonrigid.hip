// Non-rigid stage of the training-time augmentation (`train.py:155-159`: OneOf([ElasticTransform(alpha=120, sigma=120 * 0.05,
// alpha_affine=120 * 0.03), GridDistortion, OpticalDistortion(distort_limit=2, shift_limit=0.5)]), which the reference carries at
// p = 0 behind `#p=0.8 if self.use_vis_aug_non_rigid else 0`).  Every member is a resample of the frame through a coordinate map,
// so the stage is two entries:
//   asis_nonrigid_map    the map of every sample as Q5 fixed point (1/32 pixel: OpenCV remap's INTER_BITS), by kind
//   asis_nonrigid_remap  bilinear image / nearest mask through that map, integer arithmetic, reflect-101 border
// Elastic: the displacement field is alpha * (Gaussian blur of uniform noise).  The noise is a pure function of (seed, field,
// pixel) — Philox4x32-10, philox.h — and is regenerated where it is needed, halo included; no noise plane exists.  The blur is
// separable: a row pass (noise -> LDS -> fp32 plane `tmp`) and a column pass fused into the map kernel.  Both borders are scipy's
// `reflect` (half-sample, period 2 S), and the row pass of a reflected row IS the reflected row of the row pass, so `tmp` holds
// rows 0 .. S - 1 only.  Workgroups of the row pass whose sample is not elastic return at once; no workgroup waits on another.
#include "asis_common.h"
#include "philox.h"

namespace {

constexpr int NR_RMAX = 64;     // largest Gauss radius (sigma = 6 -> r = 24)
constexpr int NR_SEG = 256;     // output columns of one row-pass workgroup
constexpr int NR_ROWS = 4;      // output rows of one thread of the map kernel

// scipy.ndimage mode='reflect' (d c b a | a b c d | d c b a), any distance
__device__ __forceinline__ int reflect_half(int i, int S) {
  const int P = 2 * S;
  int m = i % P;
  if (m < 0) m += P;
  return m < S ? m : P - 1 - m;
}
// cv2.BORDER_REFLECT_101 (d c b | a b c d | c b a), any distance; S >= 2
__device__ __forceinline__ int reflect_101(int i, int S) {
  const int P = 2 * S - 2;
  int m = i % P;
  if (m < 0) m += P;
  return m < S ? m : P - m;
}

// n(f, e) = 2 U - 1, U = (w >> 8) 2^-24, w = word e & 3 of philox(counter (e >> 2, f, 0), key seed): exact in fp32
__device__ __forceinline__ float noise_at(uint64_t seed, uint32_t f, uint64_t e) {
  const uint64_t blk = e >> 2;
  const philox4 p = philox4x32_10((uint32_t)blk, (uint32_t)(blk >> 32), f, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t sel = (uint32_t)e & 3u;
  const uint32_t w = sel == 0 ? p.x : (sel == 1 ? p.y : (sel == 2 ? p.z : p.w));
  return 2.0f * ((float)(w >> 8) * 5.9604644775390625e-08f) - 1.0f;
}

// row pass: tmp[b][f][y][x] = sum_i gauss[i] n(f, y, reflect(x - r + i)); grid (segments, S, B)
__global__ __launch_bounds__(256) void nonrigid_rowblur_kernel(const int* __restrict__ kind, const int64_t* __restrict__ seed,
                                                               const float* __restrict__ gauss, int r, float* __restrict__ tmp, int S) {
  const int b = blockIdx.z;
  if (kind[b] != 1) return;                            // whole workgroup: only elastic samples pay for the blur
  __shared__ float s_n[2][NR_SEG + 2 * NR_RMAX];
  __shared__ float s_w[2 * NR_RMAX + 1];
  const int y = blockIdx.y, x0 = blockIdx.x * NR_SEG, tid = threadIdx.x;
  const uint64_t sd = (uint64_t)seed[b];
  for (int j = tid; j < NR_SEG + 2 * r; j += 256) {
    const uint64_t e = (uint64_t)y * S + reflect_half(x0 - r + j, S);
    s_n[0][j] = noise_at(sd, 0u, e);
    s_n[1][j] = noise_at(sd, 1u, e);
  }
  for (int j = tid; j <= 2 * r; j += 256) s_w[j] = gauss[j];
  __syncthreads();
  const int x = x0 + tid;
  if (x >= S) return;
  float a0 = 0.f, a1 = 0.f;
  for (int i = 0; i <= 2 * r; ++i) {
    const float w = s_w[i];
    a0 = __builtin_fmaf(w, s_n[0][tid + i], a0);
    a1 = __builtin_fmaf(w, s_n[1][tid + i], a1);
  }
  const int64_t plane = (int64_t)S * S;
  float* o = tmp + (int64_t)b * 2 * plane + (int64_t)y * S + x;
  o[0] = a0;
  o[plane] = a1;
}

// column pass (elastic) + the map of every kind; block (64, 4), a thread owns NR_ROWS consecutive rows of one column
__global__ __launch_bounds__(256) void nonrigid_map_kernel(const int* __restrict__ kind, const float4* __restrict__ params,
                                                           const float* __restrict__ gx, const float* __restrict__ gy,
                                                           const float* __restrict__ gauss, int r, const float* __restrict__ tmp,
                                                           int2* __restrict__ map, float* __restrict__ field, int S) {
  __shared__ float s_w[2 * NR_RMAX + 1];
  const int b = blockIdx.z;
  const int k = kind[b];
  if (k == 1) {                                        // uniform over the workgroup
    for (int j = threadIdx.y * 64 + threadIdx.x; j <= 2 * r; j += 256) s_w[j] = gauss[j];
    __syncthreads();
  }
  const int x = blockIdx.x * 64 + threadIdx.x;
  const int y0 = (blockIdx.y * 4 + threadIdx.y) * NR_ROWS;
  if (x >= S || y0 >= S) return;
  const int64_t plane = (int64_t)S * S;
  const float4 p0 = params[2 * b], p1 = params[2 * b + 1];
  float d0[NR_ROWS], d1[NR_ROWS];
#pragma unroll
  for (int q = 0; q < NR_ROWS; ++q) d0[q] = d1[q] = 0.f;
  if (k == 1) {
    const float* t0 = tmp + (int64_t)b * 2 * plane + x;
    const float* t1 = t0 + plane;
    for (int j = 0; j < 2 * r + NR_ROWS; ++j) {        // every output adds its taps in the order i = -r .. r
      const int64_t row = (int64_t)reflect_half(y0 - r + j, S) * S;
      const float v0 = t0[row], v1 = t1[row];
#pragma unroll
      for (int q = 0; q < NR_ROWS; ++q) {
        const int t = j - q;
        if (t >= 0 && t <= 2 * r) {
          const float w = s_w[t];
          d0[q] = __builtin_fmaf(w, v0, d0[q]);
          d1[q] = __builtin_fmaf(w, v1, d1[q]);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < NR_ROWS; ++q) {
    const int y = y0 + q;
    if (y >= S) break;
    const int64_t pix = (int64_t)y * S + x;
    int2 o;
    if (k == 1) {                                      // (alpha, A00, A01, A02 | A10, A11, A12, -)
      const float ex = p0.x * d0[q], ey = p0.x * d1[q];
      if (field) {
        field[(int64_t)b * 2 * plane + pix] = ex;
        field[(int64_t)b * 2 * plane + plane + pix] = ey;
      }
      const float X = (float)x + ex, Y = (float)y + ey;
      const float u = __builtin_fmaf(p0.y, X, __builtin_fmaf(p0.z, Y, p0.w));
      const float v = __builtin_fmaf(p1.x, X, __builtin_fmaf(p1.y, Y, p1.z));
      o = make_int2(__float2int_rn(32.0f * u), __float2int_rn(32.0f * v));
    } else if (k == 2) {
      o = make_int2(__float2int_rn(32.0f * gx[(int64_t)b * S + x]), __float2int_rn(32.0f * gy[(int64_t)b * S + y]));
    } else if (k == 3) {                               // (k, dx, dy): initUndistortRectifyMap, fx = fy = S, (k1, k2) = (k, k)
      const float fS = (float)S, c = 0.5f * (float)(S - 1);
      const float xh = ((float)x - c) / fS, yh = ((float)y - c) / fS;
      const float r2 = xh * xh + yh * yh;
      const float kr = 1.0f + p0.x * r2 + p0.x * r2 * r2;
      o = make_int2(__float2int_rn(32.0f * (fS * xh * kr + 0.5f * fS + p0.y)), __float2int_rn(32.0f * (fS * yh * kr + 0.5f * fS + p0.z)));
    } else {
      o = make_int2(32 * x, 32 * y);
    }
    map[(int64_t)b * plane + pix] = o;
  }
}

// OpenCV remap, INTER_LINEAR on 8-bit data through a Q5 map (BilinearTab_i without its common factor 32), BORDER_REFLECT_101
__global__ __launch_bounds__(256) void nonrigid_remap_kernel(const uint8_t* __restrict__ img, const int64_t* __restrict__ msk,
                                                             const int2* __restrict__ map, uint8_t* __restrict__ out,
                                                             int64_t* __restrict__ mout, int S) {
  const int b = blockIdx.y;
  const int64_t plane = (int64_t)S * S;
  const uint8_t* im = img + (int64_t)b * plane * 3;
  const int64_t* mk = msk + (int64_t)b * plane;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < plane; p += (int64_t)gridDim.x * blockDim.x) {
    const int2 q = map[(int64_t)b * plane + p];
    const int ix = q.x >> 5, iy = q.y >> 5, fx = q.x & 31, fy = q.y & 31;
    const int x0 = reflect_101(ix, S), y0 = reflect_101(iy, S);
    const int x1 = reflect_101(ix + 1, S), y1 = reflect_101(iy + 1, S);       // ix <= 2^26: no overflow
    const uint8_t* r0 = im + (int64_t)y0 * S * 3;
    const uint8_t* r1 = im + (int64_t)y1 * S * 3;
    const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
    uint8_t* o = out + ((int64_t)b * plane + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      o[c] = (uint8_t)((w00 * r0[x0 * 3 + c] + w01 * r0[x1 * 3 + c] + w10 * r1[x0 * 3 + c] + w11 * r1[x1 * 3 + c] + 512) >> 10);
    const int nx = reflect_101((int)(((int64_t)q.x + 16) >> 5), S), ny = reflect_101((int)(((int64_t)q.y + 16) >> 5), S);
    mout[(int64_t)b * plane + p] = mk[(int64_t)ny * S + nx];
  }
}

}  // namespace

extern "C" int asis_nonrigid_map(void* stream, const int32_t* kind, const float* params, const int64_t* seed, const float* gx,
                                 const float* gy, const float* gauss, int r, float* tmp, int32_t* map, float* field, int B, int S) {
  ASIS_REQUIRE(kind && params && seed && gx && gy && gauss && tmp && map, "asis_nonrigid_map: null pointer");
  ASIS_REQUIRE(B >= 1 && B <= 65535 && S >= 2 && S <= 8192, "asis_nonrigid_map: bad batch / size");
  ASIS_REQUIRE(r >= 0 && r <= NR_RMAX, "asis_nonrigid_map: Gauss radius must be in [0, %d]", NR_RMAX);
  ASIS_REQUIRE(asis_aligned16(params) && (reinterpret_cast<uintptr_t>(map) & 7) == 0 && (reinterpret_cast<uintptr_t>(seed) & 7) == 0,
               "asis_nonrigid_map: table alignment");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(nonrigid_rowblur_kernel, dim3((S + NR_SEG - 1) / NR_SEG, S, B), dim3(256), 0, s, kind, seed, gauss, r, tmp, S);
  hipLaunchKernelGGL(nonrigid_map_kernel, dim3((S + 63) / 64, (S + 4 * NR_ROWS - 1) / (4 * NR_ROWS), B), dim3(64, 4), 0, s, kind,
                     reinterpret_cast<const float4*>(params), gx, gy, gauss, r, tmp, reinterpret_cast<int2*>(map), field, S);
  ASIS_CHECK_LAUNCH("asis_nonrigid_map");
  return ASIS_OK;
}

extern "C" int asis_nonrigid_remap(void* stream, const uint8_t* img, const int64_t* mask, const int32_t* map, uint8_t* out,
                                   int64_t* mask_out, int B, int S) {
  ASIS_REQUIRE(img && mask && map && out && mask_out, "asis_nonrigid_remap: null pointer");
  ASIS_REQUIRE(B >= 1 && B <= 65535 && S >= 2 && S <= 8192, "asis_nonrigid_remap: bad batch / size");
  ASIS_REQUIRE(img != out && mask != mask_out, "asis_nonrigid_remap: the outputs must not alias the inputs");
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(map) & 7) == 0 && (reinterpret_cast<uintptr_t>(mask) & 7) == 0 &&
               (reinterpret_cast<uintptr_t>(mask_out) & 7) == 0, "asis_nonrigid_remap: map / mask alignment");
  const int64_t plane = (int64_t)S * S;
  hipLaunchKernelGGL(nonrigid_remap_kernel, dim3(asis_grid(plane, 256, 4096), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     img, mask, reinterpret_cast<const int2*>(map), out, reinterpret_cast<int64_t*>(mask_out), S);
  ASIS_CHECK_LAUNCH("asis_nonrigid_remap");
  return ASIS_OK;
}
