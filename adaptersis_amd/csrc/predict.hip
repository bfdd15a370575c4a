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
//   blend_maps            the one body of the two kernels below: K logit maps of their own sizes, some of them mirrored, of one
//                         batch, summed into acc[4][CB] per thread.  Per native pixel and map (in list order): the same taps and
//                         blend, a softmax over the C samples (exp(z - max) / sum, fp32), acc[c] += g * p[c] (the product rounded
//                         on its own: no fma, so g = 1 adds p exactly and a map given twice doubles its term exactly); the mask is
//                         encode[argmax acc] (strict >, lowest class on a tie), the optional confidence (uint8)(255 * acc[pred] /
//                         denominator + 0.5).  A mirrored map keeps the taps and weights of pixel x and mirrors the two column
//                         indices (i -> w - 1 - i): index for index the resize of the column-reversed map.  The maps come in the
//                         kernel arguments (ViewSet, TileSet, by value); the loop over them is a runtime loop around the four
//                         pixels of the thread, so the vertical tap of a map is computed once per thread and only acc[4][CB] and
//                         one pixel's samples are live (CB = C rounded up to 4 / 8 / 16: no scratch).  Where a pixel falls on a
//                         map, and with what weight, is the kernel's own (ViewAt, TileAt).  The thread's quad (thread_quad), the
//                         quad store, overlay and counts (PredictTables) are those of predict_mask_kernel, which keeps its own
//                         core: an argmax over the samples, no softmax.
//   predict_views_kernel  test-time augmentation: K <= 8 views.  The taps of predict_mask_kernel (tap_ac_false of the pixel index),
//                         g = 1, denominator K.
//   predict_tiles_kernel  sliding-window prediction: K <= 32 tiles, tile k an fp32 NHWC map of its own size [B, h, w, C] that holds
//                         the integer rectangle (oy, ox, sy, sx) of a working grid Lh x Lw.
//                         Per native pixel (y, x) of H x W, all in fp32, in this order:
//                             uy = ((float)y + 0.5f) * ((float)Lh / (float)H)          (ux likewise with x, Lw, W)
//                             tile k covers the pixel iff (float)oy <= uy < (float)(oy + sy) and the same in x
//                             s  = (uy - (float)oy) * ((float)h / (float)sy) - 0.5f, s < 0 -> 0
//                             i0 = min((int)s, h - 1), i1 = min(i0 + 1, h - 1), l1 = s - (float)i0, l0 = 1 - l1   (columns likewise)
//                         which is align_corners=False sampling of the tile's map, clamped inside the tile (tap_tile works from
//                         the working-grid coordinate, tap_ac_false from the pixel index: they round differently, so views are
//                         not tiles that cover the grid).  g = 1 (uniform), or g = gy * gx with gy = min(uy - oy, (oy + sy) - uy,
//                         R) / R, where an edge on the border of the working grid (oy == 0, oy + sy == Lh) counts as infinitely
//                         far (ramp); denominator = the sum of g, tiles in list order.  A tile whose rows do not hold uy (one y
//                         per thread; uniform over a wave unless a row is shorter than 256 pixels) or whose columns hold none of
//                         the thread's four ux is skipped before any address is formed.
// Host side: the three entries share their argument checks (check_shared, fill_maps), the choice of V and CB (load_width,
// class_bucket) and one dispatch (dispatch_int), so each launch is written once.
#include <algorithm>
#include <type_traits>

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

// The quad of a thread of the grid (ceil(H * ceil(W / 4) / 256), B): PX pixels from column x0 of row y of frame b, np of them
// inside the row, pix = (b * H + y) * W + x0
struct Quad {
  int b, y, x0, np;
  int64_t pix;
};
__device__ __forceinline__ bool thread_quad(int tid, int H, int W, Quad& q) {   // false: the thread is past the last quad
  const int quads = (W + PX - 1) / PX;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + tid;
  q.b = blockIdx.y;
  q.y = (int)(t / quads);
  q.x0 = (int)(t - (int64_t)q.y * quads) * PX;
  q.np = min(PX, W - q.x0);
  q.pix = ((int64_t)q.b * H + q.y) * W + q.x0;
  return t < (int64_t)H * quads;
}

// The body of predict_views_kernel and predict_tiles_kernel: the maps at.set.p[k] = fp32 NHWC [B, h[k], w[k], C] of a ViewSet or a
// TileSet, in list order, blended into the thread's quad.  `at` (ViewAt, TileAt) places the quad on map k:
//     at.covers(k)          does map k hold any pixel of the quad?  Asked before any address is formed
//     at.row(k)             the vertical tap ty and what the columns of map k need
//     at.holds(row, u)      does the map hold pixel u?
//     at.column(row, u, tx) the horizontal tap of pixel u -> its weight g
//     At::weighted          true: the sum of pixel u is divided by the sum of its g; false: by K
// Per pixel and map: the four taps (a mirrored map, flip[k], keeps taps and weights and mirrors the two column indices), blend_taps
// per class, a softmax (exp(z - max) / sum, fp32), acc[c] += g * p[c] with the product rounded on its own (no fma: g = 1 adds p
// exactly, a map given twice doubles its term exactly).  Then the class (strict >, in class order: the lowest class wins a tie),
// the confidence (uint8)(255 * acc[pred] / denominator + 0.5), and the tail of predict_mask_kernel.  V = channels per load, CB >= C
// = the unrolled class count (4, 8 or 16).  Only acc[4][CB], wsum[4] and one pixel's samples are live: no scratch.
// The register allocation hangs on two things (profiles/predict_refactor_resources.txt).  acc is a local of the function that
// holds the loop over the maps: behind a reference it stays in memory until that function is inlined, the accumulates are then
// packed in pairs that are copied from block to block, and the V = 1 and V = 2 instances need up to twice the registers.  And the
// questions of `at` return a value and take no early exit: an output left unset on one path turns the per-map values, which are
// the same in every lane, into per-lane ones (12 registers in the tiles kernel).
template <int V, int CB, typename At>
__device__ __forceinline__ void blend_maps(const At& at, const Quad& q, PredictTables& s, int tid, int C, uint8_t* __restrict__ mask,
                                           uint8_t* __restrict__ confidence, const uint8_t* __restrict__ frames,
                                           uint8_t* __restrict__ overlay, const uint8_t* __restrict__ target, bool counts) {
  float acc[PX][CB], wsum[PX];
#pragma unroll
  for (int u = 0; u < PX; ++u) {
    wsum[u] = 0.f;
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[u][c] = 0.f;
  }
  for (int k = 0; k < at.set.K; ++k) {
    if (!at.covers(k)) continue;
    const auto row = at.row(k);
    const Tap ty = row.ty;
    const int h = at.set.h[k], w = at.set.w[k];
    const bool flip = at.set.flip[k] != 0;
    const float* lg = at.set.p[k] + (int64_t)q.b * h * w * C;
    const float* r0 = lg + (int64_t)ty.i0 * w * C;
    const float* r1 = lg + (int64_t)ty.i1 * w * C;
#pragma unroll
    for (int u = 0; u < PX; ++u) {
      if (at.holds(row, u)) {
        Tap tx;
        const float g = at.column(row, u, tx);
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
          if (c < C) acc[u][c] += __fmul_rn(g, z[c] / sum);      // in list order: bit-identical from call to call
        if constexpr (At::weighted) wsum[u] += g;
      }
    }
  }
  int cls[PX];
  uint32_t conf[PX];
#pragma unroll
  for (int u = 0; u < PX; ++u) {
    float m = acc[u][0];
    int am = 0;
#pragma unroll
    for (int c = 1; c < CB; ++c)
      if (c < C && acc[u][c] > m) { m = acc[u][c]; am = c; }
    cls[u] = am;
    const float den = At::weighted ? wsum[u] : (float)at.set.K;
    conf[u] = (!At::weighted || den > 0.f) ? (uint32_t)(255.f * m / den + 0.5f) : 0u;   // no weight: a pixel the host check lets through
  }
  emit_quad(s, tid, C, cls, q.np, q.pix, mask, frames, overlay, target, counts);
  if (confidence) store_quad(confidence + q.pix, q.np, conf[0], conf[1], conf[2], conf[3]);
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

  Quad q;
  if (thread_quad(tid, H, W, q)) {
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    const Tap ty = tap_ac_false(q.y, sh, h);
    const float* lg = logits + (int64_t)q.b * h * w * C;
    const float* r0 = lg + (int64_t)ty.i0 * w * C;
    const float* r1 = lg + (int64_t)ty.i1 * w * C;
    int cls[PX];
#pragma unroll
    for (int u = 0; u < PX; ++u) {
      const Tap tx = tap_ac_false(min(q.x0 + u, W - 1), sw, w);
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
    emit_quad(s, tid, C, cls, q.np, q.pix, mask, frames, overlay, target, counts != nullptr);
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

// a quad on view k: the taps of predict_mask_kernel, every pixel with the weight 1, the sum divided by K
struct ViewAt {
  static constexpr bool weighted = false;
  const ViewSet& set;
  int y, x0, H, W;
  struct Row {
    Tap ty;
    int w;
    float sw;
  };
  __device__ __forceinline__ bool covers(int) const { return true; }
  __device__ __forceinline__ Row row(int k) const {
    const int h = set.h[k], w = set.w[k];
    return {tap_ac_false(y, (float)h / (float)H, h), w, (float)w / (float)W};
  }
  __device__ __forceinline__ bool holds(const Row&, int) const { return true; }
  __device__ __forceinline__ float column(const Row& r, int u, Tap& tx) const {
    tx = tap_ac_false(min(x0 + u, W - 1), r.sw, r.w);
    return 1.f;
  }
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

  Quad q;
  if (thread_quad(tid, H, W, q)) {
    ViewAt at = {vs, q.y, q.x0, H, W};
    blend_maps<V, CB>(at, q, s, tid, C, mask, confidence, frames, overlay, target, counts != nullptr);
  }
  if (counts) flush_counts(s, tid, C, counts);
}

// K tiles of one batch in the kernel arguments (1.2 KB of the 4 KB a launch may carry): map k is fp32 NHWC [B, h[k], w[k], C] and
// holds the rectangle rows [oy, oy + sy), columns [ox, ox + sx) of the working grid; flip[k] != 0 mirrors its columns
constexpr int MAXTILES = 32;
struct TileSet {
  const float* p[MAXTILES];
  int h[MAXTILES], w[MAXTILES], oy[MAXTILES], ox[MAXTILES], sy[MAXTILES], sx[MAXTILES], flip[MAXTILES];
  int K, Lh, Lw, ramp_mode;
  float R;
};

// distance weight of one axis: u in [o, o + s), an edge on the border of the working grid [0, L) does not ramp
__device__ __forceinline__ float ramp_weight(float u, int o, int s, int L, float R) {
  const float d0 = o == 0 ? INFINITY : u - (float)o;
  const float d1 = o + s == L ? INFINITY : (float)(o + s) - u;
  return fminf(fminf(d0, d1), R) / R;
}

// source coordinate d (in tile pixels, before the half-pixel shift) -> the tap of tap_ac_false
__device__ __forceinline__ Tap tap_tile(float d, float scale, int in) {
  float s = d * scale - 0.5f;
  if (s < 0.f) s = 0.f;
  Tap t;
  t.i0 = (int)s;
  if (t.i0 > in - 1) t.i0 = in - 1;
  t.i1 = t.i0 + ((t.i0 < in - 1) ? 1 : 0);
  t.l1 = s - (float)t.i0;
  t.l0 = 1.f - t.l1;
  return t;
}

// a quad on tile k, on the working grid: (uy, ux[u]) of its pixels, coverage, tap_tile, the blend weight g and its sum
struct TileAt {
  static constexpr bool weighted = true;
  const TileSet& set;
  const bool ramp;
  float uy, ux[PX];
  struct Row {
    Tap ty;
    int w, ox, sx;
    float fx0, fx1, sw, gy;
  };
  __device__ __forceinline__ TileAt(const TileSet& t, int y, int x0, int H, int W) : set(t), ramp(t.ramp_mode != 0) {
    const float rh = (float)set.Lh / (float)H, rw = (float)set.Lw / (float)W;
    uy = ((float)y + 0.5f) * rh;
#pragma unroll
    for (int u = 0; u < PX; ++u) ux[u] = ((float)min(x0 + u, W - 1) + 0.5f) * rw;
  }
  // asked before any address is formed: false for a tile whose rows do not hold uy (one y per thread; uniform over a wave unless
  // a row is shorter than 256 pixels) or whose columns hold none of the four ux (they ascend)
  __device__ __forceinline__ bool covers(int k) const {
    const int oy = set.oy[k], ox = set.ox[k];
    return uy >= (float)oy && uy < (float)(oy + set.sy[k]) && ux[PX - 1] >= (float)ox && ux[0] < (float)(ox + set.sx[k]);
  }
  __device__ __forceinline__ Row row(int k) const {
    const int oy = set.oy[k], sy = set.sy[k], ox = set.ox[k], sx = set.sx[k], h = set.h[k], w = set.w[k];
    return {tap_tile(uy - (float)oy, (float)h / (float)sy, h), w, ox, sx, (float)ox, (float)(ox + sx), (float)w / (float)sx,
            ramp ? ramp_weight(uy, oy, sy, set.Lh, set.R) : 1.f};
  }
  __device__ __forceinline__ bool holds(const Row& r, int u) const { return ux[u] >= r.fx0 && ux[u] < r.fx1; }
  __device__ __forceinline__ float column(const Row& r, int u, Tap& tx) const {
    tx = tap_tile(ux[u] - r.fx0, r.sw, r.w);
    return ramp ? r.gy * ramp_weight(ux[u], r.ox, r.sx, set.Lw, set.R) : 1.f;
  }
};

// tiles -> mask [B, H, W] (+ confidence [B, H, W]); grid as predict_mask_kernel; V, CB as predict_views_kernel
template <int V, int CB>
__global__ __launch_bounds__(256) void predict_tiles_kernel(const TileSet ts, int C, int H, int W, const uint8_t* __restrict__ encode,
                                                            uint8_t* __restrict__ mask, uint8_t* __restrict__ confidence,
                                                            const uint8_t* __restrict__ frames, const uint8_t* __restrict__ palette,
                                                            const uint8_t* __restrict__ alpha, uint8_t* __restrict__ overlay,
                                                            const uint8_t* __restrict__ target, const uint8_t* __restrict__ lut,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ PredictTables s;
  const int tid = threadIdx.x;
  load_tables(s, tid, C, encode, palette, alpha, overlay != nullptr, lut, counts != nullptr);

  Quad q;
  if (thread_quad(tid, H, W, q)) {
    TileAt at(ts, q.y, q.x0, H, W);
    blend_maps<V, CB>(at, q, s, tid, C, mask, confidence, frames, overlay, target, counts != nullptr);
  }
  if (counts) flush_counts(s, tid, C, counts);
}

// do the intervals [o[k], o[k] + s[k]) cover [0, L)?
bool intervals_cover(const int* rects, int K, int at, int L) {
  int reach = 0;
  while (reach < L) {
    int best = reach;
    for (int k = 0; k < K; ++k) {
      const int o = rects[k * 4 + at], e = o + rects[k * 4 + at + 2];
      if (o <= reach && e > best) best = e;
    }
    if (best == reach) return false;
    reach = best;
  }
  return true;
}

// ---- host side: what the three entries check, choose and launch alike ----------------------------------------------------------
// The checks on what every entry takes; `name` = the entry, `side` = the largest of its heights and widths.
int check_shared(const char* name, int C, int B, int side, const uint8_t* frames, const uint8_t* palette, const uint8_t* alpha,
                 const uint8_t* overlay, const uint8_t* target, const uint8_t* lut, const int64_t* counts) {
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "%s: C=%d must be in 1..%d", name, C, MAXC);
  ASIS_REQUIRE(B <= 65535 && side <= 16384, "%s: sizes above 16384 (batch above 65535)", name);
  ASIS_REQUIRE(!overlay || (frames && palette && alpha), "%s: overlay requested without frames, palette [C][3] and alpha [C]", name);
  ASIS_REQUIRE(!counts || (target && lut), "%s: counts requested without a raw mask and its 256-entry label table", name);
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(counts) & 7) == 0, "%s: counts must be 8-byte aligned", name);
  return ASIS_OK;
}

// The K maps of a ViewSet or TileSet (`noun` = "view" or "tile"): checked, copied into the set; `la` = the OR of their addresses
template <typename Set>
int fill_maps(const char* name, const char* noun, const float* const* logits, const int* hs, const int* ws, const int* flips, int K,
              Set& set, uintptr_t& la) {
  set.K = K;
  la = 0;
  for (int k = 0; k < K; ++k) {
    ASIS_REQUIRE(logits[k], "%s: logits[%d] is a null pointer", name, k);
    ASIS_REQUIRE(hs[k] >= 1 && ws[k] >= 1, "%s: non-positive size of %s %d: hs=%d ws=%d", name, noun, k, hs[k], ws[k]);
    ASIS_REQUIRE(hs[k] <= 16384 && ws[k] <= 16384, "%s: %s %d: hs=%d ws=%d above 16384", name, noun, k, hs[k], ws[k]);
    set.p[k] = logits[k];
    set.h[k] = hs[k];
    set.w[k] = ws[k];
    set.flip[k] = flips[k] != 0;
    la |= reinterpret_cast<uintptr_t>(logits[k]);
  }
  return ASIS_OK;
}

// channels per load: a tap's C channels are contiguous, so 16- or 8-byte loads when C and the address of every map (`la` = their OR)
// allow it (same values, same order)
int load_width(int C, uintptr_t la) { return (C % 4 == 0 && la % 16 == 0) ? 4 : ((C % 2 == 0 && la % 8 == 0) ? 2 : 1); }
// the unrolled class count of the views and tiles kernels
int class_bucket(int C) { return C <= 4 ? 4 : (C <= 8 ? 8 : 16); }

// fn(std::integral_constant<int, N>{}) for the N of the list that n equals (the last one if it equals none), in the manner of
// asis_dispatch16: a launch is written once, with `decltype(v)::value` as the template argument
template <int N, int... Rest, typename F>
void dispatch_int(int n, F&& fn) {
  if constexpr (sizeof...(Rest) == 0) fn(std::integral_constant<int, N>{});
  else if (n == N) fn(std::integral_constant<int, N>{});
  else dispatch_int<Rest...>(n, fn);
}
// fn(V, CB) of predict_views_kernel and predict_tiles_kernel
template <typename F>
void dispatch_v_cb(int C, uintptr_t la, F&& fn) {
  dispatch_int<4, 2, 1>(load_width(C, la), [&](auto v) { dispatch_int<4, 8, 16>(class_bucket(C), [&](auto cb) { fn(v, cb); }); });
}

dim3 quad_grid(int B, int H, int W) { return dim3((unsigned)(((int64_t)H * ((W + PX - 1) / PX) + 255) / 256), (unsigned)B); }

}  // namespace

extern "C" int asis_predict_mask(void* stream, const float* logits, int B, int h, int w, int C, int H, int W, const uint8_t* encode,
                                 uint8_t* mask, const uint8_t* frames, const uint8_t* palette, const uint8_t* alpha,
                                 uint8_t* overlay, const uint8_t* target, const uint8_t* lut, int64_t* counts) {
  const char* name = "asis_predict_mask";
  ASIS_REQUIRE(logits && encode && mask, "asis_predict_mask: null pointer (logits, encode and mask are required)");
  ASIS_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "asis_predict_mask: non-positive size B=%d h=%d w=%d H=%d W=%d", B, h,
               w, H, W);
  if (int rc = check_shared(name, C, B, std::max({h, w, H, W}), frames, palette, alpha, overlay, target, lut, counts)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  dispatch_int<4, 2, 1>(load_width(C, reinterpret_cast<uintptr_t>(logits)), [&](auto v) {
    hipLaunchKernelGGL(predict_mask_kernel<decltype(v)::value>, quad_grid(B, H, W), dim3(256), 0, s, logits, h, w, C, H, W, encode, mask,
                       frames, palette, alpha, overlay, target, lut, cnt);
  });
  ASIS_CHECK_LAUNCH(name);
  return ASIS_OK;
}

extern "C" int asis_predict_mask_views(void* stream, const float* const* logits, const int* hs, const int* ws, const int* flips,
                                       int K, int B, int C, int H, int W, const uint8_t* encode, uint8_t* mask, uint8_t* confidence,
                                       const uint8_t* frames, const uint8_t* palette, const uint8_t* alpha, uint8_t* overlay,
                                       const uint8_t* target, const uint8_t* lut, int64_t* counts) {
  const char* name = "asis_predict_mask_views";
  ASIS_REQUIRE(K >= 1 && K <= MAXVIEWS, "asis_predict_mask_views: K=%d views, supported 1..%d", K, MAXVIEWS);
  ASIS_REQUIRE(logits && hs && ws && flips && encode && mask,
               "asis_predict_mask_views: null pointer (logits, hs, ws, flips, encode and mask are required)");
  ASIS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "asis_predict_mask_views: non-positive size B=%d H=%d W=%d", B, H, W);
  if (int rc = check_shared(name, C, B, std::max(H, W), frames, palette, alpha, overlay, target, lut, counts)) return rc;
  ViewSet vs = {};
  uintptr_t la;
  if (int rc = fill_maps(name, "view", logits, hs, ws, flips, K, vs, la)) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  dispatch_v_cb(C, la, [&](auto v, auto cb) {
    hipLaunchKernelGGL((predict_views_kernel<decltype(v)::value, decltype(cb)::value>), quad_grid(B, H, W), dim3(256), 0, s, vs, C, H, W,
                       encode, mask, confidence, frames, palette, alpha, overlay, target, lut, cnt);
  });
  ASIS_CHECK_LAUNCH(name);
  return ASIS_OK;
}

extern "C" int asis_predict_mask_tiles(void* stream, const float* const* logits, const int* hs, const int* ws, const int* rects,
                                       const int* flips, int K, int Lh, int Lw, int blend, float ramp, int B, int C, int H, int W,
                                       const uint8_t* encode, uint8_t* mask, uint8_t* confidence, const uint8_t* frames,
                                       const uint8_t* palette, const uint8_t* alpha, uint8_t* overlay, const uint8_t* target,
                                       const uint8_t* lut, int64_t* counts) {
  const char* name = "asis_predict_mask_tiles";
  ASIS_REQUIRE(K >= 1 && K <= MAXTILES, "asis_predict_mask_tiles: K=%d tiles, supported 1..%d", K, MAXTILES);
  ASIS_REQUIRE(logits && hs && ws && rects && flips && encode && mask,
               "asis_predict_mask_tiles: null pointer (logits, hs, ws, rects, flips, encode and mask are required)");
  ASIS_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Lh >= 1 && Lw >= 1,
               "asis_predict_mask_tiles: non-positive size B=%d H=%d W=%d Lh=%d Lw=%d", B, H, W, Lh, Lw);
  if (int rc = check_shared(name, C, B, std::max({H, W, Lh, Lw}), frames, palette, alpha, overlay, target, lut, counts)) return rc;
  ASIS_REQUIRE(blend == 0 || blend == 1, "asis_predict_mask_tiles: blend=%d must be 0 (uniform) or 1 (ramp)", blend);
  ASIS_REQUIRE(ramp >= 1.f && ramp <= 16384.f, "asis_predict_mask_tiles: ramp=%g must be in 1..16384 working pixels", (double)ramp);
  TileSet ts = {};
  ts.Lh = Lh;
  ts.Lw = Lw;
  ts.ramp_mode = blend;
  ts.R = ramp;
  uintptr_t la;
  if (int rc = fill_maps(name, "tile", logits, hs, ws, flips, K, ts, la)) return rc;
  for (int k = 0; k < K; ++k) {
    const int oy = rects[k * 4], ox = rects[k * 4 + 1], sy = rects[k * 4 + 2], sx = rects[k * 4 + 3];
    ASIS_REQUIRE(sy >= 1 && sx >= 1 && sy <= Lh && sx <= Lw && oy >= 0 && ox >= 0 && oy <= Lh - sy && ox <= Lw - sx,
                 "asis_predict_mask_tiles: rectangle of tile %d (oy=%d ox=%d sy=%d sx=%d) is empty or outside the working grid %dx%d",
                 k, oy, ox, sy, sx, Lh, Lw);
    ts.oy[k] = oy;
    ts.ox[k] = ox;
    ts.sy[k] = sy;
    ts.sx[k] = sx;
  }
  // the rule: the row intervals of the rectangles cover [0, Lh) and their column intervals cover [0, Lw).  Necessary for every
  // pixel to lie in a tile, and sufficient for a set that holds a full grid of windows (every row origin with every column origin)
  ASIS_REQUIRE(intervals_cover(rects, K, 0, Lh), "asis_predict_mask_tiles: the tiles' rows do not cover the working grid's %d rows", Lh);
  ASIS_REQUIRE(intervals_cover(rects, K, 1, Lw), "asis_predict_mask_tiles: the tiles' columns do not cover the working grid's %d columns",
               Lw);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  unsigned long long* cnt = reinterpret_cast<unsigned long long*>(counts);
  dispatch_v_cb(C, la, [&](auto v, auto cb) {
    hipLaunchKernelGGL((predict_tiles_kernel<decltype(v)::value, decltype(cb)::value>), quad_grid(B, H, W), dim3(256), 0, s, ts, C, H, W,
                       encode, mask, confidence, frames, palette, alpha, overlay, target, lut, cnt);
  });
  ASIS_CHECK_LAUNCH(name);
  return ASIS_OK;
}
