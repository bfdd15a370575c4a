// Prediction: native-size label masks straight from the decoder's low-resolution logits.
//
//     out  = F.interpolate(logits, size=(H, W), mode="bilinear")      (align_corners=False, train.py:422)
//     pred = out.argmax(1)                                            (train.py:616; ties -> lowest class)
//     mask = encode[pred]                                             (class index -> pixel value of the dataset's mask files)
//
// fused: the fp32 [B, H, W, C] map and the int64 indices are never written.  The logit map (a few MB) is read through the
// caches; the kernel's stream is its 1 B/px store.  Sampling is bilinear_tap.h, shared with loss.hip, so the mask equals the
// argmax over asis_resize_bilinear_fwd bit for bit.
//   predict_mask_kernel   every thread makes 4 horizontally adjacent pixels of one row and stores them as one dword (a wave
//                         writes 256 contiguous bytes); the vertical tap and the two row pointers are computed once per thread,
//                         the horizontal tap per pixel; a tap's C contiguous channels are read with 16-byte loads when C is a
//                         multiple of 4, 8-byte loads when it is even, dword loads otherwise (template V).  A quad whose address
//                         is not 4-byte aligned (row width not a multiple of 4, odd base) or that crosses the end of the row is
//                         stored byte by byte.
//   optional, same pass:  overlay = (frame * (255 - a) + palette * a + 127) / 255 with a = alpha[pred]  (12 bytes per thread,
//                         three dword loads / stores when aligned), and per-class pixel counts against lut[raw mask]
//                         (LDS atomics per wave, then one 64-bit atomic add per non-zero entry per block: integer, so the
//                         result does not depend on the order).
//   predict_views_kernel  test-time augmentation: K <= 8 logit maps of their own sizes, some of them mirrored, of one batch.  Per
//                         native pixel and view (in view order): the same taps and blend, a softmax over the C samples
//                         (exp(z - max) / sum, fp32), acc[c] += p[c]; the mask is encode[argmax acc] (strict >, lowest class on a
//                         tie), the optional confidence (uint8)(255 * acc[pred] / K + 0.5).  A mirrored view keeps the taps and
//                         weights of pixel x and mirrors the two column indices (i -> w - 1 - i): index for index the resize of
//                         the column-reversed map.  The views come in the kernel arguments (ViewSet, by value); the loop over
//                         them is a runtime loop around the four pixels of the thread, so the vertical tap of a view is computed
//                         once per thread and only acc[4][CB] and one pixel's samples are live (CB = C rounded up to 4 / 8 / 16:
//                         no scratch).  Same quad store, overlay and counts as predict_mask_kernel (PredictTables).
#include "asis_common.h"
#include "bilinear_tap.h"

namespace {

constexpr int PX = 4;  // pixels per thread = bytes of the vector store

__device__ __forceinline__ bool aligned4_dev(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// V consecutive channels of one tap (C % V == 0 and a V * 4-byte aligned map: one V-dword load)
template <int V>
__device__ __forceinline__ void load_channels(const float* __restrict__ p, float* o) {
  if constexpr (V == 4) {
    const float4 v = *reinterpret_cast<const float4*>(p);
    o[0] = v.x; o[1] = v.y; o[2] = v.z; o[3] = v.w;
  } else if constexpr (V == 2) {
    const float2 v = *reinterpret_cast<const float2*>(p);
    o[0] = v.x; o[1] = v.y;
  } else {
    o[0] = *p;
  }
}

// The tables of a block and the tail shared by both kernels: quad store of the mask, overlay blend, per-class counts.
struct PredictTables {
  uint8_t enc[MAXC], alpha[MAXC], pal[MAXC * 3], lut[256];
  int cnt[4][MAXC * 3];
};

__device__ __forceinline__ void load_tables(PredictTables& s, int tid, int C, const uint8_t* __restrict__ encode,
                                            const uint8_t* __restrict__ palette, const uint8_t* __restrict__ alpha, bool overlay,
                                            const uint8_t* __restrict__ lut, bool counts) {
  if (tid < MAXC) s.enc[tid] = tid < C ? encode[tid] : 0;
  if (overlay) {
    if (tid < MAXC) s.alpha[tid] = tid < C ? alpha[tid] : 0;
    if (tid < MAXC * 3) s.pal[tid] = tid < C * 3 ? palette[tid] : 0;
  }
  if (counts) {
    s.lut[tid] = lut[tid];
    if (tid < 4 * MAXC * 3) (&s.cnt[0][0])[tid] = 0;
  }
  __syncthreads();
}

// np <= 4 bytes v[0..np) at d: one dword when the quad is whole and d is 4-byte aligned, byte by byte otherwise
__device__ __forceinline__ void store_quad(uint8_t* d, int np, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
  if (np == PX && aligned4_dev(d)) {
    *reinterpret_cast<uint32_t*>(d) = v0 | (v1 << 8) | (v2 << 16) | (v3 << 24);
  } else {
    const uint32_t v[PX] = {v0, v1, v2, v3};
    for (int u = 0; u < np; ++u) d[u] = (uint8_t)v[u];
  }
}

// the classes cls[0..np) of the pixels pix .. pix + np - 1 (pix = (b * H + y) * W + x0) -> mask, overlay, LDS counts of the wave
__device__ __forceinline__ void emit_quad(PredictTables& s, int tid, int C, const int (&cls)[PX], int np, int64_t pix,
                                          uint8_t* __restrict__ mask, const uint8_t* __restrict__ frames,
                                          uint8_t* __restrict__ overlay, const uint8_t* __restrict__ target, bool counts) {
  store_quad(mask + pix, np, s.enc[cls[0]], s.enc[cls[1]], s.enc[cls[2]], s.enc[cls[3]]);
  if (overlay) {
    const uint8_t* f = frames + pix * 3;
    uint8_t* o = overlay + pix * 3;
    const bool vec = np == PX && aligned4_dev(f) && aligned4_dev(o);
    uint32_t px[PX * 3];
    if (vec) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const uint32_t v = reinterpret_cast<const uint32_t*>(f)[k];
        px[k * 4] = v & 255u; px[k * 4 + 1] = (v >> 8) & 255u; px[k * 4 + 2] = (v >> 16) & 255u; px[k * 4 + 3] = v >> 24;
      }
    } else {
      for (int i = 0; i < PX * 3; ++i) px[i] = i < np * 3 ? f[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < PX; ++u) {
      const uint32_t a = s.alpha[cls[u]];
#pragma unroll
      for (int k = 0; k < 3; ++k)
        px[u * 3 + k] = (px[u * 3 + k] * (255u - a) + (uint32_t)s.pal[cls[u] * 3 + k] * a + 127u) / 255u;
    }
    if (vec) {
#pragma unroll
      for (int k = 0; k < 3; ++k)
        reinterpret_cast<uint32_t*>(o)[k] = px[k * 4] | (px[k * 4 + 1] << 8) | (px[k * 4 + 2] << 16) | (px[k * 4 + 3] << 24);
    } else {
      for (int i = 0; i < np * 3; ++i) o[i] = (uint8_t)px[i];
    }
  }
  if (counts) {
    int* cnt = s.cnt[tid >> 6];
    const uint8_t* tg = target + pix;
    for (int u = 0; u < np; ++u) {
      const int lab = s.lut[tg[u]];
      atomicAdd(&cnt[cls[u] * 3 + 1], 1);
      if (lab < C) atomicAdd(&cnt[lab * 3 + 2], 1);   // labels >= C belong to no class
      if (lab == cls[u]) atomicAdd(&cnt[lab * 3 + 0], 1);
    }
  }
}

// after the last emit_quad of the block: one 64-bit atomic add per non-zero entry
__device__ __forceinline__ void flush_counts(PredictTables& s, int tid, int C, unsigned long long* __restrict__ counts) {
  __syncthreads();
  if (tid < C * 3) {
    const int n = (s.cnt[0][tid] + s.cnt[1][tid]) + (s.cnt[2][tid] + s.cnt[3][tid]);
    if (n) atomicAdd(&counts[tid], (unsigned long long)n);
  }
}

// logits [B, h, w, C] -> mask [B, H, W]; grid (ceil(H * ceil(W / 4) / 256), B); V = channels per load (C % V == 0)
template <int V>
__global__ __launch_bounds__(256) void predict_mask_kernel(const float* __restrict__ logits, int h, int w, int C, int H, int W,
                                                           const uint8_t* __restrict__ encode, uint8_t* __restrict__ mask,
                                                           const uint8_t* __restrict__ frames, const uint8_t* __restrict__ palette,
                                                           const uint8_t* __restrict__ alpha, uint8_t* __restrict__ overlay,
                                                           const uint8_t* __restrict__ target, const uint8_t* __restrict__ lut,
                                                           unsigned long long* __restrict__ counts) {
  __shared__ PredictTables s;
  const int tid = threadIdx.x;
  load_tables(s, tid, C, encode, palette, alpha, overlay != nullptr, lut, counts != nullptr);

  const int b = blockIdx.y;
  const int quads = (W + PX - 1) / PX;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + tid;
  if (t < (int64_t)H * quads) {
    const int y = (int)(t / quads), x0 = (int)(t - (int64_t)y * quads) * PX;
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    const Tap ty = tap_ac_false(y, sh, h);
    const float* lg = logits + (int64_t)b * h * w * C;
    const float* r0 = lg + (int64_t)ty.i0 * w * C;
    const float* r1 = lg + (int64_t)ty.i1 * w * C;
    const int np = min(PX, W - x0);
    int cls[PX];
#pragma unroll
    for (int u = 0; u < PX; ++u) {
      const Tap tx = tap_ac_false(min(x0 + u, W - 1), sw, w);
      const float* p00 = r0 + (int64_t)tx.i0 * C;
      const float* p01 = r0 + (int64_t)tx.i1 * C;
      const float* p10 = r1 + (int64_t)tx.i0 * C;
      const float* p11 = r1 + (int64_t)tx.i1 * C;
      float m = -INFINITY;
      int am = 0;
#pragma unroll
      for (int c0 = 0; c0 < MAXC; c0 += V)
        if (c0 < C) {
          float v00[V], v01[V], v10[V], v11[V];
          load_channels<V>(p00 + c0, v00);
          load_channels<V>(p01 + c0, v01);
          load_channels<V>(p10 + c0, v10);
          load_channels<V>(p11 + c0, v11);
#pragma unroll
          for (int k = 0; k < V; ++k) {
            const float z = blend_taps(ty, tx, v00[k], v01[k], v10[k], v11[k]);
            if (z > m) { m = z; am = c0 + k; }   // strict, in class order: the lowest class wins a tie (ce_acc_kernel, torch.max)
          }
        }
      cls[u] = am;
    }
    emit_quad(s, tid, C, cls, np, ((int64_t)b * H + y) * W + x0, mask, frames, overlay, target, counts != nullptr);
  }
  if (counts) flush_counts(s, tid, C, counts);
}

// K views of one batch in the kernel arguments: map k is fp32 NHWC [B, h[k], w[k], C], flip[k] != 0 mirrors its columns
constexpr int MAXVIEWS = 8;
struct ViewSet {
  const float* p[MAXVIEWS];
  int h[MAXVIEWS], w[MAXVIEWS], flip[MAXVIEWS];
  int K;
};

// views -> mask [B, H, W] (+ confidence [B, H, W]); grid as predict_mask_kernel; V = channels per load (C % V == 0, every map
// V * 4-byte aligned), CB >= C = the unrolled class count (4, 8 or 16)
template <int V, int CB>
__global__ __launch_bounds__(256) void predict_views_kernel(const ViewSet vs, int C, int H, int W, const uint8_t* __restrict__ encode,
                                                            uint8_t* __restrict__ mask, uint8_t* __restrict__ confidence,
                                                            const uint8_t* __restrict__ frames, const uint8_t* __restrict__ palette,
                                                            const uint8_t* __restrict__ alpha, uint8_t* __restrict__ overlay,
                                                            const uint8_t* __restrict__ target, const uint8_t* __restrict__ lut,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ PredictTables s;
  const int tid = threadIdx.x;
  load_tables(s, tid, C, encode, palette, alpha, overlay != nullptr, lut, counts != nullptr);

  const int b = blockIdx.y;
  const int quads = (W + PX - 1) / PX;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + tid;
  if (t < (int64_t)H * quads) {
    const int y = (int)(t / quads), x0 = (int)(t - (int64_t)y * quads) * PX;
    const int np = min(PX, W - x0);
    float acc[PX][CB];
#pragma unroll
    for (int u = 0; u < PX; ++u)
#pragma unroll
      for (int c = 0; c < CB; ++c) acc[u][c] = 0.f;
    for (int k = 0; k < vs.K; ++k) {
      const int h = vs.h[k], w = vs.w[k];
      const bool flip = vs.flip[k] != 0;
      const float sh = (float)h / (float)H, sw = (float)w / (float)W;
      const Tap ty = tap_ac_false(y, sh, h);
      const float* lg = vs.p[k] + (int64_t)b * h * w * C;
      const float* r0 = lg + (int64_t)ty.i0 * w * C;
      const float* r1 = lg + (int64_t)ty.i1 * w * C;
#pragma unroll
      for (int u = 0; u < PX; ++u) {
        const Tap tx = tap_ac_false(min(x0 + u, W - 1), sw, w);   // taps and weights of pixel x; a mirrored view mirrors the columns
        const int j0 = flip ? w - 1 - tx.i0 : tx.i0, j1 = flip ? w - 1 - tx.i1 : tx.i1;
        const float* p00 = r0 + (int64_t)j0 * C;
        const float* p01 = r0 + (int64_t)j1 * C;
        const float* p10 = r1 + (int64_t)j0 * C;
        const float* p11 = r1 + (int64_t)j1 * C;
        float z[CB];
        float m = -INFINITY;
#pragma unroll
        for (int c0 = 0; c0 < CB; c0 += V)
          if (c0 < C) {
            float v00[V], v01[V], v10[V], v11[V];
            load_channels<V>(p00 + c0, v00);
            load_channels<V>(p01 + c0, v01);
            load_channels<V>(p10 + c0, v10);
            load_channels<V>(p11 + c0, v11);
#pragma unroll
            for (int i = 0; i < V; ++i) {
              z[c0 + i] = blend_taps(ty, tx, v00[i], v01[i], v10[i], v11[i]);
              if (z[c0 + i] > m) m = z[c0 + i];
            }
          }
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < CB; ++c)
          if (c < C) {
            z[c] = expf(z[c] - m);
            sum += z[c];
          }
#pragma unroll
        for (int c = 0; c < CB; ++c)
          if (c < C) acc[u][c] += z[c] / sum;      // in view order: bit-identical from call to call
      }
    }
    int cls[PX];
    uint32_t conf[PX];
    const float fk = (float)vs.K;
#pragma unroll
    for (int u = 0; u < PX; ++u) {
      float m = acc[u][0];
      int am = 0;
#pragma unroll
      for (int c = 1; c < CB; ++c)
        if (c < C && acc[u][c] > m) { m = acc[u][c]; am = c; }   // strict, in class order: the lowest class wins a tie
      cls[u] = am;
      conf[u] = (uint32_t)(255.f * m / fk + 0.5f);
    }
    const int64_t pix = ((int64_t)b * H + y) * W + x0;
    emit_quad(s, tid, C, cls, np, pix, mask, frames, overlay, target, counts != nullptr);
    if (confidence) store_quad(confidence + pix, np, conf[0], conf[1], conf[2], conf[3]);
  }
  if (counts) flush_counts(s, tid, C, counts);
}

}  // namespace

extern "C" int asis_predict_mask(void* stream, const float* logits, int B, int h, int w, int C, int H, int W, const uint8_t* encode,
                                 uint8_t* mask, const uint8_t* frames, const uint8_t* palette, const uint8_t* alpha,
                                 uint8_t* overlay, const uint8_t* target, const uint8_t* lut, int64_t* counts) {
  ASIS_REQUIRE(logits && encode && mask, "asis_predict_mask: null pointer (logits, encode and mask are required)");
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "asis_predict_mask: C=%d must be in 1..%d", C, MAXC);
  ASIS_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "asis_predict_mask: non-positive size B=%d h=%d w=%d H=%d W=%d", B, h,
               w, H, W);
  ASIS_REQUIRE(B <= 65535 && h <= 16384 && w <= 16384 && H <= 16384 && W <= 16384,
               "asis_predict_mask: sizes above 16384 (batch above 65535)");
  ASIS_REQUIRE(!overlay || (frames && palette && alpha),
               "asis_predict_mask: overlay requested without frames, palette [C][3] and alpha [C]");
  ASIS_REQUIRE(!counts || (target && lut), "asis_predict_mask: counts requested without a raw mask and its 256-entry label table");
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0, "asis_predict_mask: counts must be 8-byte aligned");
  const int quads = (W + PX - 1) / PX;
  const int64_t n = (int64_t)H * quads;
  // a tap's C channels are contiguous: 16- or 8-byte loads when C and the map's address allow it (same values, same order)
  const uintptr_t la = reinterpret_cast<uintptr_t>(logits);
  const int V = (C % 4 == 0 && la % 16 == 0) ? 4 : ((C % 2 == 0 && la % 8 == 0) ? 2 : 1);
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)B);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
#define ASIS_PREDICT_LAUNCH(VV)                                                                                                   \
  hipLaunchKernelGGL(predict_mask_kernel<VV>, grid, dim3(256), 0, s, logits, h, w, C, H, W, encode, mask, frames, palette, alpha, \
                     overlay, target, lut, cnt)
  if (V == 4) ASIS_PREDICT_LAUNCH(4);
  else if (V == 2) ASIS_PREDICT_LAUNCH(2);
  else ASIS_PREDICT_LAUNCH(1);
#undef ASIS_PREDICT_LAUNCH
  ASIS_CHECK_LAUNCH("asis_predict_mask");
  return ASIS_OK;
}

extern "C" int asis_predict_mask_views(void* stream, const float* const* logits, const int* hs, const int* ws, const int* flips,
                                       int K, int B, int C, int H, int W, const uint8_t* encode, uint8_t* mask, uint8_t* confidence,
                                       const uint8_t* frames, const uint8_t* palette, const uint8_t* alpha, uint8_t* overlay,
                                       const uint8_t* target, const uint8_t* lut, int64_t* counts) {
  ASIS_REQUIRE(K >= 1 && K <= MAXVIEWS, "asis_predict_mask_views: K=%d views, supported 1..%d", K, MAXVIEWS);
  ASIS_REQUIRE(logits && hs && ws && flips && encode && mask,
               "asis_predict_mask_views: null pointer (logits, hs, ws, flips, encode and mask are required)");
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "asis_predict_mask_views: C=%d must be in 1..%d", C, MAXC);
  ASIS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "asis_predict_mask_views: non-positive size B=%d H=%d W=%d", B, H, W);
  ASIS_REQUIRE(B <= 65535 && H <= 16384 && W <= 16384, "asis_predict_mask_views: sizes above 16384 (batch above 65535)");
  ViewSet vs = {};
  vs.K = K;
  uintptr_t la = 0;
  for (int k = 0; k < K; ++k) {
    ASIS_REQUIRE(logits[k], "asis_predict_mask_views: logits[%d] is a null pointer", k);
    ASIS_REQUIRE(hs[k] >= 1 && ws[k] >= 1, "asis_predict_mask_views: non-positive size of view %d: hs=%d ws=%d", k, hs[k], ws[k]);
    ASIS_REQUIRE(hs[k] <= 16384 && ws[k] <= 16384, "asis_predict_mask_views: view %d: hs=%d ws=%d above 16384", k, hs[k], ws[k]);
    vs.p[k] = logits[k];
    vs.h[k] = hs[k];
    vs.w[k] = ws[k];
    vs.flip[k] = flips[k] != 0;
    la |= reinterpret_cast<uintptr_t>(logits[k]);
  }
  ASIS_REQUIRE(!overlay || (frames && palette && alpha),
               "asis_predict_mask_views: overlay requested without frames, palette [C][3] and alpha [C]");
  ASIS_REQUIRE(!counts || (target && lut),
               "asis_predict_mask_views: counts requested without a raw mask and its 256-entry label table");
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0, "asis_predict_mask_views: counts must be 8-byte aligned");
  const int quads = (W + PX - 1) / PX;
  const int64_t n = (int64_t)H * quads;
  // as asis_predict_mask, with the alignment of every map: the wide loads need all K addresses aligned
  const int V = (C % 4 == 0 && la % 16 == 0) ? 4 : ((C % 2 == 0 && la % 8 == 0) ? 2 : 1);
  const int CB = C <= 4 ? 4 : (C <= 8 ? 8 : 16);
  const dim3 grid((unsigned)((n + 255) / 256), (unsigned)B);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
#define ASIS_VIEWS_LAUNCH(VV, CC)                                                                                                \
  hipLaunchKernelGGL((predict_views_kernel<VV, CC>), grid, dim3(256), 0, s, vs, C, H, W, encode, mask, confidence, frames, palette, \
                     alpha, overlay, target, lut, cnt)
#define ASIS_VIEWS_BUCKET(VV)          \
  do {                                 \
    if (CB == 4) ASIS_VIEWS_LAUNCH(VV, 4);       \
    else if (CB == 8) ASIS_VIEWS_LAUNCH(VV, 8);  \
    else ASIS_VIEWS_LAUNCH(VV, 16);    \
  } while (0)
  if (V == 4) ASIS_VIEWS_BUCKET(4);
  else if (V == 2) ASIS_VIEWS_BUCKET(2);
  else ASIS_VIEWS_BUCKET(1);
#undef ASIS_VIEWS_BUCKET
#undef ASIS_VIEWS_LAUNCH
  ASIS_CHECK_LAUNCH("asis_predict_mask_views");
  return ASIS_OK;
}
