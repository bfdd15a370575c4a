// The strong student view of semi-supervised training: colour jitter (brightness, contrast, saturation, hue in a per-sample
// order), greyscale, Gaussian blur, on the fp32 [B,3,H,W] output of asis_augment.  Built into libasis_strong.so (build.py
// SIDE_LIBS; ABI and semantics in include/asis_strong.h), beside libasis_hip.so, whose error plumbing it uses.
//
// Two kernels:
//   strong_mean_kernel  only for batches with a contrast operation: the grey sum of a sample under the operations in front of
//                       contrast.  Workgroup j of a sample sums SM_CHUNK pixels in double: a thread's items, an xor tree over the
//                       wave, the 4 waves in index order -> partial[b][j].  No atomics: the same bits from call to call.
//   strong_view_kernel  one read and one write of the image.  A workgroup owns a SV_TILE x SV_TILE output tile of ONE sample, so
//                       the operation codes, factors, flags and taps are uniform (scalar loads, scalar branches).  Radius 0: the
//                       pointwise chain on registers (16-byte accesses when VEC; a sample without any operation is copied bit
//                       by bit).  Radius R: the tile plus a halo of R through the reflect map, the chain applied once per loaded
//                       pixel into LDS [3][TW][TW], TW = SV_TILE + 2 R; horizontal taps into [3][TW][SV_TILE]; vertical taps,
//                       clamp, store.  R is a template argument (the taps live in registers, the loops unroll), chosen by a
//                       uniform switch.  LDS of the launch: that of the batch's largest radius (40128 bytes at 6: 4 workgroups
//                       = 16 waves a CU; none for a batch without blur).
// Every global read goes through reflect() + a clamp to the image, every store is guarded by y < H && x < W.
#include "../../include/asis_strong.h"
#include "asis_common.h"

namespace {

constexpr int SV_THREADS = 256, SV_TILE = 32, SV_RMAX = 6;
constexpr int SM_ITEMS = 16, SM_CHUNK = SV_THREADS * SM_ITEMS;
constexpr int OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3;

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ float grey_of(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

// RGB -> HSV (max / min form with its guards: a grey pixel has s = 0 and stays itself), h <- (h + f) mod 1, HSV -> RGB
__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float f) {
  const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
  const bool eq = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eq ? 1.f : maxc);
  const float inv = 1.f / (eq ? 1.f : cr);
  const float rc = (maxc - r) * inv, gc = (maxc - g) * inv, bc = (maxc - b) * inv;
  float h = maxc == r ? bc - gc : (maxc == g ? 2.f + rc - bc : 4.f + gc - rc);
  h = h / 6.f + 1.f;
  h -= floorf(h);
  h += f;
  h -= floorf(h);
  const float h6 = h * 6.f, fi = floorf(h6), ff = h6 - fi;
  int i = (int)fi;
  i = i >= 6 ? i - 6 : i;  // h can round to 1
  const float v = maxc;
  const float p = clamp01(v * (1.f - s)), q = clamp01(v * (1.f - s * ff)), t = clamp01(v * (1.f - s * (1.f - ff)));
  r = (i == 0 || i == 5) ? v : (i == 1 ? q : (i == 4 ? t : p));
  g = (i == 1 || i == 2) ? v : (i == 0 ? t : (i == 3 ? q : p));
  b = (i == 3 || i == 4) ? v : (i == 2 ? t : (i == 5 ? q : p));
}

// what a workgroup does to every pixel of its sample: uniform over the workgroup
struct Chain {
  int op[4];
  float f[4];
  bool grey, contrast;
  float mean;
};

__device__ __forceinline__ Chain load_chain(const int* __restrict__ ops, const float* __restrict__ fac, const int* __restrict__ apply, int b) {
  Chain c;
  const bool on = !apply || apply[b] != 0;
  c.contrast = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    c.op[k] = on ? ops[4 * b + k] : -1;
    c.f[k] = fac[4 * b + k];
    c.contrast |= c.op[k] == OP_CONTRAST;
  }
  c.grey = false;
  c.mean = 0.f;
  return c;
}

// N pixels through the operations, in order.  PREFIX: stop in front of contrast (the image whose grey mean contrast uses).
template <int N, bool PREFIX> __device__ __forceinline__ void run_chain(float (&r)[N], float (&g)[N], float (&b)[N], const Chain& c) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int op = c.op[k];
    const float f = c.f[k];
    if (op == OP_CONTRAST) {
      if (PREFIX) return;
      const float add = (1.f - f) * c.mean;
#pragma unroll
      for (int e = 0; e < N; ++e) {
        r[e] = clamp01(f * r[e] + add);
        g[e] = clamp01(f * g[e] + add);
        b[e] = clamp01(f * b[e] + add);
      }
    } else if (op == OP_BRIGHTNESS) {
#pragma unroll
      for (int e = 0; e < N; ++e) {
        r[e] = clamp01(r[e] * f);
        g[e] = clamp01(g[e] * f);
        b[e] = clamp01(b[e] * f);
      }
    } else if (op == OP_SATURATION) {
#pragma unroll
      for (int e = 0; e < N; ++e) {
        const float add = (1.f - f) * grey_of(r[e], g[e], b[e]);
        r[e] = clamp01(f * r[e] + add);
        g[e] = clamp01(f * g[e] + add);
        b[e] = clamp01(f * b[e] + add);
      }
    } else if (op == OP_HUE) {
#pragma unroll
      for (int e = 0; e < N; ++e) hue_shift(r[e], g[e], b[e], f);
    }
  }
  if (!PREFIX && c.grey) {
#pragma unroll
    for (int e = 0; e < N; ++e) r[e] = g[e] = b[e] = grey_of(r[e], g[e], b[e]);
  }
}

// x fp32 [B,3,HW]; grid (nblk, B)
template <bool VEC>
__global__ __launch_bounds__(SV_THREADS) void strong_mean_kernel(const float* __restrict__ x, const int* __restrict__ ops,
                                                                 const float* __restrict__ fac, const int* __restrict__ apply, int HW,
                                                                 int nblk, double* __restrict__ partial) {
  __shared__ double ws[SV_THREADS / 64];
  const int b = blockIdx.y, tid = threadIdx.x;
  const Chain c = load_chain(ops, fac, apply, b);
  if (!c.contrast) return;  // uniform: nobody reads this sample's row
  const float* xb = x + (int64_t)b * 3 * HW;
  const int base = blockIdx.x * SM_CHUNK;  // < HW
  double acc = 0.0;
  if constexpr (VEC) {  // HW % 4 == 0: i < HW means i + 3 < HW
#pragma unroll
    for (int j = 0; j < SM_ITEMS / 4; ++j) {
      const int i = base + (j * SV_THREADS + tid) * 4;
      if (i < HW) {
        const f32x4 vr = *reinterpret_cast<const f32x4*>(xb + i), vg = *reinterpret_cast<const f32x4*>(xb + HW + i),
                    vb = *reinterpret_cast<const f32x4*>(xb + 2 * (int64_t)HW + i);
        float r[4] = {vr[0], vr[1], vr[2], vr[3]}, g[4] = {vg[0], vg[1], vg[2], vg[3]}, bl[4] = {vb[0], vb[1], vb[2], vb[3]};
        run_chain<4, true>(r, g, bl, c);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc += (double)grey_of(r[e], g[e], bl[e]);
      }
    }
  } else {
#pragma unroll 4
    for (int j = 0; j < SM_ITEMS; ++j) {
      const int i = base + j * SV_THREADS + tid;
      if (i < HW) {
        float r[1] = {xb[i]}, g[1] = {xb[HW + i]}, bl[1] = {xb[2 * (int64_t)HW + i]};
        run_chain<1, true>(r, g, bl, c);
        acc += (double)grey_of(r[0], g[0], bl[0]);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) ws[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[(int64_t)b * nblk + blockIdx.x] = ((ws[0] + ws[1]) + ws[2]) + ws[3];
}

// reflect border without edge repeat; one reflection is exact for -n < i < 2 n - 1, the clamp keeps any other index (the rows and
// columns of an edge tile that no output of the image uses) inside the image
__device__ __forceinline__ int reflect(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * (n - 1) - i : i;
  return min(max(i, 0), n - 1);
}

template <int R>
__device__ __forceinline__ void blur_tile(const float* __restrict__ xb, float* __restrict__ ob, int H, int W, int x0, int y0,
                                          const Chain& c, const float* __restrict__ taps, float* lds) {
  constexpr int TW = SV_TILE + 2 * R, NT = 2 * R + 1, PLANE = TW * TW, HPLANE = TW * SV_TILE;
  float* stage = lds;           // [3][TW][TW]
  float* hb = lds + 3 * PLANE;  // [3][TW][SV_TILE]
  const int tid = threadIdx.x;
  const int HW = H * W;
  float w[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) w[k] = taps[SV_RMAX - R + k];
  for (int idx = tid; idx < PLANE; idx += SV_THREADS) {
    const int ly = idx / TW, lx = idx - ly * TW;
    const int off = reflect(y0 - R + ly, H) * W + reflect(x0 - R + lx, W);
    float r[1] = {xb[off]}, g[1] = {xb[HW + off]}, b[1] = {xb[2 * (int64_t)HW + off]};
    run_chain<1, false>(r, g, b, c);
    stage[idx] = r[0];
    stage[PLANE + idx] = g[0];
    stage[2 * PLANE + idx] = b[0];
  }
  __syncthreads();
  for (int idx = tid; idx < HPLANE; idx += SV_THREADS) {
    const int ly = idx / SV_TILE, tx = idx - ly * SV_TILE;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float* s = stage + ch * PLANE + ly * TW + tx;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < NT; ++k) acc = __builtin_fmaf(w[k], s[k], acc);
      hb[ch * HPLANE + idx] = acc;
    }
  }
  __syncthreads();
  const int tx = tid & (SV_TILE - 1), x = x0 + tx;
#pragma unroll
  for (int j = 0; j < SV_TILE * SV_TILE / SV_THREADS; ++j) {
    const int ty = (tid / SV_TILE) + j * (SV_THREADS / SV_TILE), y = y0 + ty;
    if (y < H && x < W) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float* s = hb + ch * HPLANE + ty * SV_TILE + tx;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < NT; ++k) acc = __builtin_fmaf(w[k], s[k * SV_TILE], acc);
        ob[(int64_t)ch * HW + y * W + x] = clamp01(acc);
      }
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void point_tile(const float* __restrict__ xb, float* __restrict__ ob, int H, int W, int x0, int y0,
                                           const Chain& c) {
  const int tid = threadIdx.x;
  const int HW = H * W;
  if constexpr (VEC) {  // W % 4 == 0: the 4 pixels lie in one row, x < W means x + 3 < W
    const int y = y0 + (tid >> 3), x = x0 + (tid & 7) * 4;
    if (y >= H || x >= W) return;
    const int off = y * W + x;
    const f32x4 vr = *reinterpret_cast<const f32x4*>(xb + off), vg = *reinterpret_cast<const f32x4*>(xb + HW + off),
                vb = *reinterpret_cast<const f32x4*>(xb + 2 * (int64_t)HW + off);
    float r[4] = {vr[0], vr[1], vr[2], vr[3]}, g[4] = {vg[0], vg[1], vg[2], vg[3]}, b[4] = {vb[0], vb[1], vb[2], vb[3]};
    run_chain<4, false>(r, g, b, c);
    *reinterpret_cast<f32x4*>(ob + off) = f32x4{r[0], r[1], r[2], r[3]};
    *reinterpret_cast<f32x4*>(ob + HW + off) = f32x4{g[0], g[1], g[2], g[3]};
    *reinterpret_cast<f32x4*>(ob + 2 * (int64_t)HW + off) = f32x4{b[0], b[1], b[2], b[3]};
  } else {
    const int x = x0 + (tid & (SV_TILE - 1));
#pragma unroll
    for (int j = 0; j < SV_TILE * SV_TILE / SV_THREADS; ++j) {
      const int y = y0 + (tid / SV_TILE) + j * (SV_THREADS / SV_TILE);
      if (y < H && x < W) {
        const int off = y * W + x;
        float r[1] = {xb[off]}, g[1] = {xb[HW + off]}, b[1] = {xb[2 * (int64_t)HW + off]};
        run_chain<1, false>(r, g, b, c);
        ob[off] = r[0];
        ob[HW + off] = g[0];
        ob[2 * (int64_t)HW + off] = b[0];
      }
    }
  }
}

// grid (cdiv(W, SV_TILE), cdiv(H, SV_TILE), B); dynamic LDS: view_lds_bytes(max_radius)
template <bool VEC>
__global__ __launch_bounds__(SV_THREADS) void strong_view_kernel(const float* __restrict__ x, const int* __restrict__ ops,
                                                                 const float* __restrict__ fac, const int* __restrict__ flags,
                                                                 const float* __restrict__ gauss, const int* __restrict__ apply,
                                                                 const double* __restrict__ partial, int nblk, int max_radius, int H,
                                                                 int W, float* __restrict__ out) {
  extern __shared__ float lds[];
  const int b = blockIdx.z, x0 = blockIdx.x * SV_TILE, y0 = blockIdx.y * SV_TILE;
  const int HW = H * W;
  Chain c = load_chain(ops, fac, apply, b);
  const bool on = !apply || apply[b] != 0;
  c.grey = on && flags[2 * b] != 0;
  int radius = on ? flags[2 * b + 1] : 0;
  if (radius < 0 || radius > max_radius || radius >= min(H, W)) radius = 0;  // never a halo the LDS or the reflect map cannot hold
  if (c.contrast && partial) {
    double s = 0.0;
    for (int j = 0; j < nblk; ++j) s += partial[(int64_t)b * nblk + j];
    c.mean = (float)(s / (double)HW);
  }
  const float* xb = x + (int64_t)b * 3 * HW;
  float* ob = out + (int64_t)b * 3 * HW;
  const float* taps = gauss + b * (2 * SV_RMAX + 1);
  switch (radius) {
    case 0: point_tile<VEC>(xb, ob, H, W, x0, y0, c); break;
    case 1: blur_tile<1>(xb, ob, H, W, x0, y0, c, taps, lds); break;
    case 2: blur_tile<2>(xb, ob, H, W, x0, y0, c, taps, lds); break;
    case 3: blur_tile<3>(xb, ob, H, W, x0, y0, c, taps, lds); break;
    case 4: blur_tile<4>(xb, ob, H, W, x0, y0, c, taps, lds); break;
    case 5: blur_tile<5>(xb, ob, H, W, x0, y0, c, taps, lds); break;
    default: blur_tile<6>(xb, ob, H, W, x0, y0, c, taps, lds); break;
  }
}

size_t view_lds_bytes(int max_radius) {
  if (max_radius <= 0) return 0;
  const int tw = SV_TILE + 2 * max_radius;
  return sizeof(float) * 3 * (size_t)(tw * tw + tw * SV_TILE);
}

// the sizes both entries share
int strong_sizes(const char* op, int B, int H, int W) {
  ASIS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive size B=%d H=%d W=%d", op, B, H, W);
  ASIS_REQUIRE((int64_t)B * 3 * H * W < ((int64_t)1 << 31), "%s: B*3*H*W must be < 2^31 (B=%d H=%d W=%d)", op, B, H, W);
  ASIS_REQUIRE(B <= 65535 && asis_cdiv(H, SV_TILE) <= 65535, "%s: B=%d and H/%d=%ld must be <= 65535", op, B, SV_TILE,
               asis_cdiv(H, SV_TILE));
  return ASIS_OK;
}

}  // namespace

extern "C" int asis_strong_chunk(void) { return SM_CHUNK; }

extern "C" int asis_strong_nblk(int64_t HW) {
  if (HW < 1 || HW >= ((int64_t)1 << 31)) {
    asis_set_error_("asis_strong_nblk: need 1 <= H*W < 2^31 (H*W=%lld)", (long long)HW);
    return ASIS_EINVAL;
  }
  return (int)asis_cdiv(HW, SM_CHUNK);
}

extern "C" int asis_strong_mean(void* stream, const float* x, const int* ops, const float* fac, const int* apply, int B, int H, int W,
                                double* partial) {
  const char* op = "asis_strong_mean";
  ASIS_REQUIRE(x && ops && fac && partial, "%s: null pointer", op);
  if (strong_sizes(op, B, H, W) != ASIS_OK) return ASIS_EINVAL;
  const int HW = H * W, nblk = (int)asis_cdiv(HW, SM_CHUNK);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)nblk, (unsigned)B);
  if (HW % 4 == 0 && asis_aligned16(x))
    hipLaunchKernelGGL(strong_mean_kernel<true>, grid, dim3(SV_THREADS), 0, s, x, ops, fac, apply, HW, nblk, partial);
  else
    hipLaunchKernelGGL(strong_mean_kernel<false>, grid, dim3(SV_THREADS), 0, s, x, ops, fac, apply, HW, nblk, partial);
  ASIS_CHECK_LAUNCH(op);
  return ASIS_OK;
}

extern "C" int asis_strong_view(void* stream, const float* x, const int* ops, const float* fac, const int* flags, const float* gauss,
                                const int* apply, const double* partial, int max_radius, int B, int H, int W, float* out) {
  const char* op = "asis_strong_view";
  ASIS_REQUIRE(x && ops && fac && flags && gauss && out, "%s: null pointer", op);
  if (strong_sizes(op, B, H, W) != ASIS_OK) return ASIS_EINVAL;
  ASIS_REQUIRE(max_radius >= 0 && max_radius <= SV_RMAX, "%s: max_radius=%d must be in 0..%d", op, max_radius, SV_RMAX);
  const int64_t n = (int64_t)B * 3 * H * W;
  ASIS_REQUIRE(out + n <= x || x + n <= out, "%s: out overlaps x", op);
  const int nblk = (int)asis_cdiv((int64_t)H * W, SM_CHUNK);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)asis_cdiv(W, SV_TILE), (unsigned)asis_cdiv(H, SV_TILE), (unsigned)B);
  const size_t lds = view_lds_bytes(max_radius);
  if (W % 4 == 0 && asis_aligned16(x) && asis_aligned16(out))
    hipLaunchKernelGGL(strong_view_kernel<true>, grid, dim3(SV_THREADS), lds, s, x, ops, fac, flags, gauss, apply, partial, nblk,
                       max_radius, H, W, out);
  else
    hipLaunchKernelGGL(strong_view_kernel<false>, grid, dim3(SV_THREADS), lds, s, x, ops, fac, flags, gauss, apply, partial, nblk,
                       max_radius, H, W, out);
  ASIS_CHECK_LAUNCH(op);
  return ASIS_OK;
}
