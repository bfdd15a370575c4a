// On-device frame resize of the datasets' host path (`tools/dataset.py:51-53`: PIL img.resize((S, S), BILINEAR),
// mask.resize((S, S), NEAREST)), bit-identical to Pillow's 8-bit resample.  The coefficient tables come from the host
// (adaptersis_amd/tools/frame_resize.py, float64 restatement of Pillow's precompute_coeffs); here only integer arithmetic:
//   acc = 2^21 + sum_j k_j * px (int32, 22 fractional bits) ; out = 255 if acc >= 2^30, 0 if acc <= 0, else acc >> 22
// Pillow's order: horizontal pass rounded to uint8 first, vertical pass on its result; an unchanged axis is skipped.
//   resize_h_kernel      one workgroup per input row: the row is staged in LDS with 16-byte loads, every thread makes four
//                        output pixels (12 bytes, three dword stores)
//   resize_v_kernel      per output row the taps are rows: every thread makes 4 consecutive bytes of the row from dword loads
//   mask_nearest_kernel  out = lut[mask[iy[y], ix[x]]] (NEAREST commutes with the pointwise label table)
#include "asis_common.h"

namespace {

__device__ __forceinline__ uint32_t clip8(int acc) {
  return acc >= (1 << 30) ? 255u : (acc <= 0 ? 0u : (uint32_t)(acc >> 22));
}

// src [rows, Wi, 3] -> dst [rows, Wo, 3]; span [Wo] = (xmin, n), coef [Wo, K]
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const int2* __restrict__ span, const int* __restrict__ coef, int Wi,
                                                       int Wo, int K, int vec_in, int vec_out) {
  extern __shared__ uint4 s_row4[];
  uint8_t* s_row = reinterpret_cast<uint8_t*>(s_row4);
  const int64_t row = blockIdx.x;
  const int in_bytes = Wi * 3;
  const uint8_t* s = src + row * in_bytes;
  if (vec_in) {
    const uint4* s4 = reinterpret_cast<const uint4*>(s);
    for (int i = threadIdx.x; i < in_bytes / 16; i += blockDim.x) s_row4[i] = s4[i];
  } else {
    for (int i = threadIdx.x; i < in_bytes; i += blockDim.x) s_row[i] = s[i];
  }
  __syncthreads();
  uint8_t* d = dst + row * (int64_t)Wo * 3;
  for (int p0 = threadIdx.x * 4; p0 < Wo; p0 += blockDim.x * 4) {
    uint32_t res[12];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = p0 + u < Wo ? p0 + u : Wo - 1;
      const int2 sp = span[p];
      const int* kp = coef + (int64_t)p * K;
      const int nt = min(sp.y, K);
      int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
      for (int j = 0; j < nt; ++j) {
        const int k = kp[j];
        const int xx = min(sp.x + j, Wi - 1) * 3;
        a0 += k * s_row[xx];
        a1 += k * s_row[xx + 1];
        a2 += k * s_row[xx + 2];
      }
      res[u * 3] = clip8(a0); res[u * 3 + 1] = clip8(a1); res[u * 3 + 2] = clip8(a2);
    }
    if (vec_out && p0 + 4 <= Wo) {
      uint32_t* d4 = reinterpret_cast<uint32_t*>(d + p0 * 3);
#pragma unroll
      for (int w = 0; w < 3; ++w)
        d4[w] = res[w * 4] | (res[w * 4 + 1] << 8) | (res[w * 4 + 2] << 16) | (res[w * 4 + 3] << 24);
    } else {
      const int np = min(4, Wo - p0);
      for (int i = 0; i < np * 3; ++i) d[p0 * 3 + i] = (uint8_t)res[i];
    }
  }
}

// src [B, Hi, row_bytes] -> dst [B, Ho, row_bytes]; span [Ho] = (ymin, n), coef [Ho, K]; one thread per 4 bytes of an output row
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                       const int2* __restrict__ span, const int* __restrict__ coef, int Hi,
                                                       int Ho, int row_bytes, int K, int vec) {
  const int b = blockIdx.y;
  const int quads = (row_bytes + 3) / 4;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)Ho * quads) return;
  const int y = (int)(t / quads), q = (int)(t - (int64_t)y * quads) * 4;
  const int2 sp = span[y];
  const int* kp = coef + (int64_t)y * K;
  const int nt = min(sp.y, K);
  const uint8_t* s = src + (int64_t)b * Hi * row_bytes + q;
  uint8_t* d = dst + ((int64_t)b * Ho + y) * row_bytes + q;
  int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21, a3 = 1 << 21;
  if (vec) {
    for (int j = 0; j < nt; ++j) {
      const int k = kp[j];
      const uint32_t v = *reinterpret_cast<const uint32_t*>(s + (int64_t)min(sp.x + j, Hi - 1) * row_bytes);
      a0 += k * (int)(v & 255u);
      a1 += k * (int)((v >> 8) & 255u);
      a2 += k * (int)((v >> 16) & 255u);
      a3 += k * (int)(v >> 24);
    }
    *reinterpret_cast<uint32_t*>(d) = clip8(a0) | (clip8(a1) << 8) | (clip8(a2) << 16) | (clip8(a3) << 24);
  } else {
    const int nb = min(4, row_bytes - q);
    int acc[4] = {a0, a1, a2, a3};
    for (int j = 0; j < nt; ++j) {
      const int k = kp[j];
      const uint8_t* r = s + (int64_t)min(sp.x + j, Hi - 1) * row_bytes;
      for (int i = 0; i < nb; ++i) acc[i] += k * r[i];
    }
    for (int i = 0; i < nb; ++i) d[i] = (uint8_t)clip8(acc[i]);
  }
}

// mask [B, Hi, Wi] -> out [B, Ho, Wo] = lut[mask[b, iy[y], ix[x]]]; one thread per 4 output bytes of a row
__global__ __launch_bounds__(256) void mask_nearest_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ iy,
                                                           const int* __restrict__ ix, const uint8_t* __restrict__ lut,
                                                           uint8_t* __restrict__ out, int Hi, int Wi, int Ho, int Wo, int vec) {
  __shared__ uint8_t s_lut[256];
  s_lut[threadIdx.x] = lut[threadIdx.x];
  __syncthreads();
  const int b = blockIdx.y;
  const int quads = (Wo + 3) / 4;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (int64_t)Ho * quads) return;
  const int y = (int)(t / quads), x0 = (int)(t - (int64_t)y * quads) * 4;
  const uint8_t* r = mask + ((int64_t)b * Hi + iy[y]) * Wi;
  uint8_t* d = out + ((int64_t)b * Ho + y) * Wo + x0;
  if (vec) {
    const int4 xs = *reinterpret_cast<const int4*>(ix + x0);
    *reinterpret_cast<uint32_t*>(d) = (uint32_t)s_lut[r[xs.x]] | ((uint32_t)s_lut[r[xs.y]] << 8) |
                                      ((uint32_t)s_lut[r[xs.z]] << 16) | ((uint32_t)s_lut[r[xs.w]] << 24);
  } else {
    const int nb = min(4, Wo - x0);
    for (int i = 0; i < nb; ++i) d[i] = s_lut[r[ix[x0 + i]]];
  }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

}  // namespace

extern "C" int asis_frame_resize(void* stream, const uint8_t* img, const uint8_t* mask, const int32_t* xspan, const int32_t* xcoef,
                                 int kx, const int32_t* yspan, const int32_t* ycoef, int ky, const int32_t* ix, const int32_t* iy,
                                 const uint8_t* lut, uint8_t* tmp, uint8_t* out_img, uint8_t* out_mask, int B, int Hi, int Wi,
                                 int Ho, int Wo) {
  ASIS_REQUIRE(B >= 1 && Hi >= 1 && Wi >= 1 && Ho >= 1 && Wo >= 1, "asis_frame_resize: bad batch / sizes");
  ASIS_REQUIRE(Wi <= 16384 && Hi <= 16384 && Wo <= 16384 && Ho <= 16384, "asis_frame_resize: sizes above 16384");
  ASIS_REQUIRE((img == nullptr) == (out_img == nullptr) && (mask == nullptr) == (out_mask == nullptr),
               "asis_frame_resize: input and output must both be given or both be null");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (img) {
    const bool need_h = Wi != Wo, need_v = Hi != Ho;
    ASIS_REQUIRE(!need_h || (xspan && xcoef && kx >= 1 && kx <= 1024), "asis_frame_resize: horizontal tables");
    ASIS_REQUIRE(!need_v || (yspan && ycoef && ky >= 1 && ky <= 1024), "asis_frame_resize: vertical tables");
    ASIS_REQUIRE(!(need_h && need_v) || tmp, "asis_frame_resize: both axes change and tmp [B, Hi, Wo, 3] is null");
    ASIS_REQUIRE(((reinterpret_cast<uintptr_t>(xspan) | reinterpret_cast<uintptr_t>(yspan)) & 7) == 0,
                 "asis_frame_resize: span table alignment");
    if (!need_h && !need_v) {
      if (hipMemcpyAsync(out_img, img, (size_t)B * Hi * Wi * 3, hipMemcpyDeviceToDevice, s) != hipSuccess)
        ASIS_FAIL(ASIS_ELAUNCH, "asis_frame_resize: copy failed");
    }
    const uint8_t* vsrc = img;
    if (need_h) {
      uint8_t* hdst = need_v ? tmp : out_img;
      const int in_bytes = Wi * 3;
      const size_t lds = (size_t)((in_bytes + 15) / 16) * 16;
      const int vec_in = (in_bytes % 16 == 0) && asis_aligned16(img);
      const int vec_out = (Wo % 4 == 0) && aligned4(hdst);
      hipLaunchKernelGGL(resize_h_kernel, dim3((unsigned)((int64_t)B * Hi)), dim3(256), lds, s, img, hdst,
                         reinterpret_cast<const int2*>(xspan), xcoef, Wi, Wo, kx, vec_in, vec_out);
      ASIS_CHECK_LAUNCH("asis_frame_resize (horizontal)");
      vsrc = hdst;
    }
    if (need_v) {
      const int row_bytes = Wo * 3;
      const int quads = (row_bytes + 3) / 4;
      const int vec = (row_bytes % 4 == 0) && aligned4(vsrc) && aligned4(out_img);
      const int64_t n = (int64_t)Ho * quads;
      hipLaunchKernelGGL(resize_v_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, s, vsrc, out_img,
                         reinterpret_cast<const int2*>(yspan), ycoef, Hi, Ho, row_bytes, ky, vec);
      ASIS_CHECK_LAUNCH("asis_frame_resize (vertical)");
    }
  }
  if (mask) {
    ASIS_REQUIRE(ix && iy && lut, "asis_frame_resize: mask tables");
    const int quads = (Wo + 3) / 4;
    const int vec = (Wo % 4 == 0) && aligned4(out_mask) && asis_aligned16(ix);
    const int64_t n = (int64_t)Ho * quads;
    hipLaunchKernelGGL(mask_nearest_kernel, dim3((unsigned)((n + 255) / 256), B), dim3(256), 0, s, mask, iy, ix, lut, out_mask,
                       Hi, Wi, Ho, Wo, vec);
    ASIS_CHECK_LAUNCH("asis_frame_resize (mask)");
  }
  return ASIS_OK;
}
