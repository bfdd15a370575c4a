// Stage-4 tail + classifier of the decode head with the 3x3 conv commuted with the x2 upsampling
// (`decoders.py:131-135`: BatchNorm2d, ReLU, Upsample(2, bilinear, align_corners=True), Conv2d(64, classes, 3, padding=1)).
//
// The upsampling acts per channel and is linear, the conv is linear: the 1x1 part of each of the nine taps runs BEFORE the
// upsampling, on a quarter of the pixels and with 9 * classes channels instead of 64.  With a = relu(raw * scale + shift) at [H, W]
// and Wz[(tap, k), c] = w[c, k, tap]:
//   forward   z[tap, c] = sum_k a[k] Wz[(tap, k), c]                                   cls_lowres_z_kernel      (reads raw once)
//             out[c](y, x) = bias[c] + sum_tap [(y+dy, x+dx) inside] up(z[tap, c])(y+dy, x+dx)   cls_lowres_gather_kernel
//   backward  e[tap, c] = up^T(shift_tap(d[c]))            (a pixel whose shifted position falls outside is dropped)
//             g = relu'(.) * (Wz^T e),   sum g | sum g*xhat,   dW[c, k, tap] = sum_pixels a[k] e[tap, c]      cls_lowres_bwd_kernel
// The 64-channel map never exists at [2H, 2W]: no upsampled operand pair forward, no fp32 dU backward.  Everything is fp32 and every
// sum runs in a fixed order (no atomics): two calls give the same bits.
#include "asis_common.h"

namespace {

constexpr int CIN = 64;
constexpr int TS = 16;  // backward: low-resolution tile of TS x TS pixels = one pixel per thread in the e phase
constexpr int WS = 2 * TS + 5;  // side of the gradient window a tile reads: rows 2 ti0 - 2 .. 2 (ti0 + TS - 1) + 4

// source taps of output index o for align_corners=True: the expressions of bwd.hip / the upsample kernels in convmisc.hip
__device__ __forceinline__ void tap_ac_true(int o, float r, int in, int& i0, int& i1, float& l0, float& l1) {
  const float s = r * (float)o;
  i0 = (int)s;
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

// classifier weight fp32 [C][64][3][3] -> LDS [tap][c][k]: a lane's four channels of one (tap, c) are one 16-byte read
template <int C>
__device__ __forceinline__ void stage_weights(const float* __restrict__ w, float* wl) {
  for (int i = threadIdx.x; i < 9 * C * CIN; i += blockDim.x) {
    const int k = i % CIN, tc = i / CIN, c = tc % C, t = tc / C;
    wl[i] = w[(c * CIN + k) * 9 + t];
  }
}

// z fp32 [B][H][9][W][C] (tap-planar rows: the gather below reads runs of neighbouring columns of one tap).  16 lanes per pixel,
// four channels each; the 16 partial sums of every output meet in a DPP row sum.
template <int C>
__global__ __launch_bounds__(256) void cls_lowres_z_kernel(const float* __restrict__ raw, const float* __restrict__ scale,
                                                           const float* __restrict__ shift, const float* __restrict__ w,
                                                           float* __restrict__ z, int64_t rows, int H, int W) {
  constexpr int NE = 9 * C, NV = (NE + 15) / 16;
  __shared__ __attribute__((aligned(16))) float wl[NE * CIN];
  stage_weights<C>(w, wl);
  __syncthreads();
  const int l16 = threadIdx.x & 15, pg = threadIdx.x >> 4;
  const float4 sc = reinterpret_cast<const float4*>(scale)[l16], sh = reinterpret_cast<const float4*>(shift)[l16];
  // the trip count is the same for every lane of a wave (row16_sum needs all 64 active); a pixel past the end computes zeros
  for (int64_t base = (int64_t)blockIdx.x * 16; base < rows; base += (int64_t)gridDim.x * 16) {
    const int64_t pix = base + pg;
    const bool live = pix < rows;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      const float4 v = reinterpret_cast<const float4*>(raw)[pix * (CIN / 4) + l16];
      a.x = fmaxf(v.x * sc.x + sh.x, 0.f);
      a.y = fmaxf(v.y * sc.y + sh.y, 0.f);
      a.z = fmaxf(v.z * sc.z + sh.z, 0.f);
      a.w = fmaxf(v.w * sc.w + sh.w, 0.f);
    }
    float keep[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) keep[q] = 0.f;
#pragma unroll
    for (int n = 0; n < NE; ++n) {
      const float4 wv = reinterpret_cast<const float4*>(wl + n * CIN)[l16];
      const float s = row16_sum(a.x * wv.x + a.y * wv.y + a.z * wv.z + a.w * wv.w);
      if (l16 == (n & 15)) keep[n >> 4] = s;
    }
    if (live) {
      const int j = (int)(pix % W);
      const int64_t bi = pix / W;                      // b * H + i
      float* zr = z + (bi * 9 * W + j) * C;            // + t * W * C + c
#pragma unroll
      for (int q = 0; q < NV; ++q) {
        const int n = 16 * q + l16;
        if (n < NE) zr[(int64_t)(n / C) * W * C + (n % C)] = keep[q];
      }
    }
  }
}

template <int C> struct VecC { float v[C]; };
template <int C> __device__ __forceinline__ VecC<C> load_c(const float* p) {
  VecC<C> r;
  if constexpr (C == 2) {
    const float2 t = *reinterpret_cast<const float2*>(p);
    r.v[0] = t.x; r.v[1] = t.y;
  } else if constexpr (C == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) r.v[c] = p[c];
  }
  return r;
}

// out[b, y, x, :] = bias + sum over the taps inside the map of the bilinear sample of z[tap] at (y + dy, x + dx).
// grid = (column chunks of 64, row groups of 4, images); one output pixel per thread.
template <int C>
__global__ __launch_bounds__(256) void cls_lowres_gather_kernel(const float* __restrict__ z, const float* __restrict__ bias,
                                                                float* __restrict__ out, int H, int W) {
  const int OH = 2 * H, OW = 2 * W;
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), b = blockIdx.z;
  if (x >= OW || y >= OH) return;
  const float rh = (float)(H - 1) / (float)(OH - 1), rw = (float)(W - 1) / (float)(OW - 1);
  int yi0[3], yi1[3], xi0[3], xi1[3];
  float yl0[3], yl1[3], xl0[3], xl1[3];
  bool yok[3], xok[3];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const int Y = y + d - 1, X = x + d - 1;
    yok[d] = (unsigned)Y < (unsigned)OH;
    xok[d] = (unsigned)X < (unsigned)OW;
    tap_ac_true(yok[d] ? Y : 0, rh, H, yi0[d], yi1[d], yl0[d], yl1[d]);
    tap_ac_true(xok[d] ? X : 0, rw, W, xi0[d], xi1[d], xl0[d], xl1[d]);
  }
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = bias ? bias[c] : 0.f;
  const float* zb = z + (int64_t)b * H * 9 * W * C;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky) {
    if (!yok[ky]) continue;
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      if (!xok[kx]) continue;
      const int t = ky * 3 + kx;
      const float* r0 = zb + ((int64_t)yi0[ky] * 9 + t) * W * C;
      const float* r1 = zb + ((int64_t)yi1[ky] * 9 + t) * W * C;
      const VecC<C> v00 = load_c<C>(r0 + xi0[kx] * C), v01 = load_c<C>(r0 + xi1[kx] * C);
      const VecC<C> v10 = load_c<C>(r1 + xi0[kx] * C), v11 = load_c<C>(r1 + xi1[kx] * C);
      // the four-term blend in the order of the upsample kernels: (i0, j0), (i0, j1), (i1, j0), (i1, j1)
      const float w00 = yl0[ky] * xl0[kx], w01 = yl0[ky] * xl1[kx], w10 = yl1[ky] * xl0[kx], w11 = yl1[ky] * xl1[kx];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        float u = 0.f;
        u += w00 * v00.v[c];
        u += w01 * v01.v[c];
        u += w10 * v10.v[c];
        u += w11 * v11.v[c];
        acc[c] += u;
      }
    }
  }
  float* o = out + (((int64_t)b * OH + y) * OW + x) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) o[c] = acc[c];
}

// the first C channels of one pixel of the 16-bit gradient (hi + optional rounding residual) as fp32
template <typename T, int C>
__device__ __forceinline__ void load_d(const T* __restrict__ ph, const T* __restrict__ pl, float* d) {
  float h[4], l[4] = {0.f, 0.f, 0.f, 0.f};
  if constexpr (C == 2) {
    unpack2<T>(*reinterpret_cast<const uint32_t*>(ph), h[0], h[1]);
    if (pl) unpack2<T>(*reinterpret_cast<const uint32_t*>(pl), l[0], l[1]);
  } else {
    const uint2 a = *reinterpret_cast<const uint2*>(ph);
    unpack2<T>(a.x, h[0], h[1]);
    unpack2<T>(a.y, h[2], h[3]);
    if (pl) {
      const uint2 q = *reinterpret_cast<const uint2*>(pl);
      unpack2<T>(q.x, l[0], l[1]);
      unpack2<T>(q.y, l[2], l[3]);
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) d[c] = h[c] + l[c];
}

// One workgroup walks low-resolution tiles of TS x TS pixels (grid-stride, a fixed run per workgroup), per tile:
//   staging   (2 classes; with 3 and 4 the e phase loads from memory, see STAGE) the tile's WS x WS window
//             of d = d16 + d_lo as fp32 into LDS, zeros outside the map: one load pair per window pixel instead of 49 per thread
//   e phase   one thread per pixel (i, j): e[tap][c] = sum_{Y, X} wy(Y, i) wx(X, j) d[c](Y - dy, X - dx) over the <= 5 x 5 output
//             positions whose bilinear taps touch the pixel (Y in 2i-1 .. 2i+3: the run of a x2 align-corners map, the last one
//             only by rounding; weights from tap_ac_true), separably: the 7-wide row sums h[dx] first, then the rows.  -> LDS
//   k phase   16 lanes per pixel, four of the 64 channels each: g = relu'(.) * sum_{tap,c} w[c,k,tap] e[tap,c], the BatchNorm
//             partial sums, and the lane's 9 C x 4 weight-gradient sums a[k] e[tap,c], kept in registers over the whole run.
// At the end the 16 pixel groups are summed through LDS in a fixed order: one partial row [2][64] and one slab row per workgroup.
template <typename T, int C>
__global__ __launch_bounds__(256) void cls_lowres_bwd_kernel(const T* __restrict__ dh, const T* __restrict__ dl, int CoP,
                                                             const float* __restrict__ raw, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, const float* __restrict__ w,
                                                             float* __restrict__ g, float* __restrict__ partial,
                                                             float* __restrict__ slabs, int H, int W, int tiles_x, int tiles_y,
                                                             int ntiles) {
  constexpr int NE = 9 * C;
  __shared__ __attribute__((aligned(16))) float wl[NE * CIN];
  __shared__ __attribute__((aligned(16))) float el[256 * NE];  // e of the tile's pixels; reused by the final reductions (>= 256 * 4 C floats)
  __shared__ float wyt[TS * 5], wxt[TS * 5];
  constexpr bool STAGE = C == 2;   // the headline; 3 classes: the window's 147 values per thread cost half the occupancy, 4: no room
  __shared__ __attribute__((aligned(16))) float dwin[STAGE ? WS * WS * C : 4];
  stage_weights<C>(w, wl);
  const int OH = 2 * H, OW = 2 * W;
  const float rh = (float)(H - 1) / (float)(OH - 1), rw = (float)(W - 1) / (float)(OW - 1);
  const int l16 = threadIdx.x & 15, pg = threadIdx.x >> 4;
  const float4 sc = reinterpret_cast<const float4*>(scale)[l16], sh = reinterpret_cast<const float4*>(shift)[l16];
  const float4 mu = reinterpret_cast<const float4*>(mean)[l16], is = reinterpret_cast<const float4*>(invstd)[l16];
  float acc[NE][4];
#pragma unroll
  for (int n = 0; n < NE; ++n)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[n][q] = 0.f;
  float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / (tiles_x * tiles_y), tr = tile - b * (tiles_x * tiles_y);
    const int ti0 = (tr / tiles_x) * TS, tj0 = (tr % tiles_x) * TS;
    __syncthreads();  // the previous tile's k phase has read el and the tap tables (first trip: wl is staged)
    if (threadIdx.x < 2 * TS * 5) {
      // tap tables of the tile: weight of output index 2 i - 1 + m (m = 0..4) on source index i, rows then columns
      const int isx = threadIdx.x / (TS * 5), q = threadIdx.x - isx * (TS * 5);
      const int i = (isx ? tj0 : ti0) + q / 5, in = isx ? W : H;
      const int o = 2 * i - 1 + q % 5;
      float wt = 0.f;
      if (i < in && o >= 0 && o < 2 * in) {
        int a0, a1; float l0, l1;
        tap_ac_true(o, isx ? rw : rh, in, a0, a1, l0, l1);
        wt = ((a0 == i) ? l0 : 0.f) + ((a1 == i) ? l1 : 0.f);
      }
      (isx ? wxt : wyt)[q] = wt;
    }
    if constexpr (STAGE) {
      for (int p = threadIdx.x; p < WS * WS; p += 256) {
        const int r = p / WS;
        const int row = 2 * ti0 - 2 + r, col = 2 * tj0 - 2 + (p - r * WS);
        float dv[C];
#pragma unroll
        for (int c = 0; c < C; ++c) dv[c] = 0.f;
        if ((unsigned)row < (unsigned)OH && (unsigned)col < (unsigned)OW) {
          const int64_t off = (((int64_t)b * OH + row) * OW + col) * CoP;
          load_d<T, C>(dh + off, dl ? dl + off : nullptr, dv);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) dwin[p * C + c] = dv[c];
      }
    }
    __syncthreads();
    {  // ---- e phase
      const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
      const int i = ti0 + ti, j = tj0 + tj;
      float e[3][3][C];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int c = 0; c < C; ++c) e[ky][kx][c] = 0.f;
      if (i < H && j < W) {
        float wy[5], wx[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) { wy[m] = wyt[ti * 5 + m]; wx[m] = wxt[tj * 5 + m]; }
#pragma unroll
        for (int u = 0; u < 7; ++u) {          // gradient row 2 i - 2 + u = Y - dy
          const int row = 2 * i - 2 + u;
          float dv[7][C];
          if constexpr (!STAGE) {
            if ((unsigned)row >= (unsigned)OH) continue;
          }
#pragma unroll
          for (int v = 0; v < 7; ++v) {        // gradient column 2 j - 2 + v = X - dx
            const int col = 2 * j - 2 + v;
            if constexpr (STAGE) {             // window row 2 ti + u, column 2 tj + v (zeros outside the map)
              const VecC<C> q = load_c<C>(dwin + ((2 * ti + u) * WS + 2 * tj + v) * C);
#pragma unroll
              for (int c = 0; c < C; ++c) dv[v][c] = q.v[c];
            } else if ((unsigned)col < (unsigned)OW) {
              const int64_t off = (((int64_t)b * OH + row) * OW + col) * CoP;
              load_d<T, C>(dh + off, dl ? dl + off : nullptr, dv[v]);
            } else {
#pragma unroll
              for (int c = 0; c < C; ++c) dv[v][c] = 0.f;
            }
          }
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            float h[C];
#pragma unroll
            for (int c = 0; c < C; ++c) h[c] = 0.f;
#pragma unroll
            for (int m = 0; m < 5; ++m)        // X = 2 j - 1 + m, column X - dx = 2 j - 2 + (m + 2 - kx)
#pragma unroll
              for (int c = 0; c < C; ++c) h[c] += wx[m] * dv[m + 2 - kx][c];
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {   // Y = row + dy = 2 i - 1 + (u - 2 + ky)
              const int m = u - 2 + ky;
              if (m < 0 || m > 4) continue;
#pragma unroll
              for (int c = 0; c < C; ++c) e[ky][kx][c] += wy[m] * h[c];
            }
          }
        }
      }
      float* ep = el + threadIdx.x * NE;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
#pragma unroll
          for (int c = 0; c < C; ++c) ep[(ky * 3 + kx) * C + c] = e[ky][kx][c];
    }
    __syncthreads();
    // ---- k phase: trip `it` = tile row it, pixel group pg = tile column
    for (int it = 0; it < TS; ++it) {
      const int i = ti0 + it, j = tj0 + pg;
      if (i >= H) break;
      if (j >= W) continue;
      const int64_t idx = (((int64_t)b * H + i) * W + j) * (CIN / 4) + l16;
      const float4 xv = reinterpret_cast<const float4*>(raw)[idx];
      const float y0 = xv.x * sc.x + sh.x, y1 = xv.y * sc.y + sh.y, y2 = xv.z * sc.z + sh.z, y3 = xv.w * sc.w + sh.w;
      const float a0 = fmaxf(y0, 0.f), a1 = fmaxf(y1, 0.f), a2 = fmaxf(y2, 0.f), a3 = fmaxf(y3, 0.f);
      const float* ep = el + (it * TS + pg) * NE;
      float4 gs = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int n = 0; n < NE; ++n) {
        const float ev = ep[n];
        const float4 wv = reinterpret_cast<const float4*>(wl + n * CIN)[l16];
        gs.x += wv.x * ev; gs.y += wv.y * ev; gs.z += wv.z * ev; gs.w += wv.w * ev;
        acc[n][0] += a0 * ev; acc[n][1] += a1 * ev; acc[n][2] += a2 * ev; acc[n][3] += a3 * ev;
      }
      float4 gg;   // the ReLU mask: the fp32 expression of upsample_bn_relu_bwd_kernel
      gg.x = (xv.x * sc.x + sh.x > 0.f) ? gs.x : 0.f;
      gg.y = (xv.y * sc.y + sh.y > 0.f) ? gs.y : 0.f;
      gg.z = (xv.z * sc.z + sh.z > 0.f) ? gs.z : 0.f;
      gg.w = (xv.w * sc.w + sh.w > 0.f) ? gs.w : 0.f;
      reinterpret_cast<float4*>(g)[idx] = gg;
      s1.x += gg.x; s1.y += gg.y; s1.z += gg.z; s1.w += gg.w;
      s2.x += gg.x * (xv.x - mu.x) * is.x;
      s2.y += gg.y * (xv.y - mu.y) * is.y;
      s2.z += gg.z * (xv.z - mu.z) * is.z;
      s2.w += gg.w * (xv.w - mu.w) * is.w;
    }
  }

  // ---- the workgroup's sums: 16 pixel groups in ascending order
  float4* red = reinterpret_cast<float4*>(el);
  __syncthreads();
  red[threadIdx.x] = s1;
  red[256 + threadIdx.x] = s2;
  __syncthreads();
  if (pg == 0) {
    for (int q = 1; q < 16; ++q) {
      const float4 a = red[q * 16 + l16], bq = red[256 + q * 16 + l16];
      s1.x += a.x; s1.y += a.y; s1.z += a.z; s1.w += a.w;
      s2.x += bq.x; s2.y += bq.y; s2.z += bq.z; s2.w += bq.w;
    }
    reinterpret_cast<float4*>(partial + ((int64_t)blockIdx.x * 2 + 0) * CIN)[l16] = s1;
    reinterpret_cast<float4*>(partial + ((int64_t)blockIdx.x * 2 + 1) * CIN)[l16] = s2;
  }
  float* row = slabs + (int64_t)blockIdx.x * C * CIN * 9;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c)
      red[c * 256 + threadIdx.x] = make_float4(acc[t * C + c][0], acc[t * C + c][1], acc[t * C + c][2], acc[t * C + c][3]);
    __syncthreads();
    for (int o = threadIdx.x; o < C * CIN; o += 256) {
      const int c = o / CIN, k = o - c * CIN;
      float s = 0.f;
      for (int q = 0; q < 16; ++q) s += el[(c * 256 + q * 16) * 4 + k];
      row[(c * CIN + k) * 9 + t] = s;
    }
  }
}

int tiles_of(int n) { return (n + TS - 1) / TS; }

}  // namespace

// workgroups of the backward = rows of `partial` and of `slabs`: an equal run of tiles each, at most 1024
extern "C" int asis_cls_lowres_nblk(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 1;
  const int64_t ntiles = (int64_t)B * tiles_of(H) * tiles_of(W);
  const int64_t per = (ntiles + 1023) / 1024;
  return (int)((ntiles + per - 1) / per);
}

extern "C" int asis_cls_lowres_fwd(void* stream, const float* raw, const float* scale, const float* shift, const float* w,
                                   const float* bias, float* z, float* out, int B, int H, int W, int Cin, int Cout) {
  ASIS_REQUIRE(raw && scale && shift && w && z && out, "asis_cls_lowres_fwd: null pointer");
  ASIS_REQUIRE(Cin == CIN && Cout >= 2 && Cout <= 4 && B > 0 && B <= 65535 && H >= 2 && W >= 2 && H <= 65535 * 2 && W < (1 << 24),
               "asis_cls_lowres_fwd: Cin=%d must be 64, Cout=%d in 2..4, the map %d x %d x %d at least 2 x 2", Cin, Cout, B, H, W);
  ASIS_REQUIRE(asis_aligned16(raw) && asis_aligned16(scale) && asis_aligned16(shift) && asis_aligned16(z) && asis_aligned16(out),
               "asis_cls_lowres_fwd: alignment");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t rows = (int64_t)B * H * W;
  const dim3 gz(asis_grid(rows, 16, 2048)), gg((2 * W + 63) / 64, (2 * H + 3) / 4, B);
#define ASIS_CLS_FWD(CO)                                                                                            \
  do {                                                                                                              \
    hipLaunchKernelGGL((cls_lowres_z_kernel<CO>), gz, dim3(256), 0, s, raw, scale, shift, w, z, rows, H, W);       \
    hipLaunchKernelGGL((cls_lowres_gather_kernel<CO>), gg, dim3(256), 0, s, (const float*)z, bias, out, H, W);     \
  } while (0)
  if (Cout == 2) ASIS_CLS_FWD(2);
  else if (Cout == 3) ASIS_CLS_FWD(3);
  else ASIS_CLS_FWD(4);
#undef ASIS_CLS_FWD
  ASIS_CHECK_LAUNCH("asis_cls_lowres_fwd");
  return ASIS_OK;
}

extern "C" int asis_cls_lowres_bwd(void* stream, int dtype, const void* d16, const void* d_lo, int CoP, const float* raw,
                                   const float* scale, const float* shift, const float* mean, const float* invstd, const float* w,
                                   float* g, float* partial, float* slabs, int nblk, int B, int H, int W, int Cin, int Cout) {
  ASIS_REQUIRE(d16 && raw && scale && shift && mean && invstd && w && g && partial && slabs, "asis_cls_lowres_bwd: null pointer");
  ASIS_REQUIRE(Cin == CIN && Cout >= 2 && Cout <= 4 && B > 0 && H >= 2 && W >= 2 && H < (1 << 24) && W < (1 << 24),
               "asis_cls_lowres_bwd: Cin=%d must be 64, Cout=%d in 2..4, the map %d x %d x %d at least 2 x 2", Cin, Cout, B, H, W);
  ASIS_REQUIRE(CoP >= Cout && CoP % 4 == 0, "asis_cls_lowres_bwd: CoP=%d must be a multiple of 4 and >= Cout=%d", CoP, Cout);
  ASIS_REQUIRE(nblk == asis_cls_lowres_nblk(B, H, W), "asis_cls_lowres_bwd: nblk=%d, asis_cls_lowres_nblk gives %d", nblk,
               asis_cls_lowres_nblk(B, H, W));
  ASIS_REQUIRE(asis_aligned16(d16) && (!d_lo || asis_aligned16(d_lo)) && asis_aligned16(raw) && asis_aligned16(scale) &&
               asis_aligned16(shift) && asis_aligned16(mean) && asis_aligned16(invstd) && asis_aligned16(g) && asis_aligned16(partial),
               "asis_cls_lowres_bwd: alignment");
  ASIS_DT_OK(dtype, "asis_cls_lowres_bwd");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int tx = tiles_of(W), ty = tiles_of(H);
  const int64_t nt = (int64_t)B * tx * ty;
  ASIS_REQUIRE(nt < (1 << 30), "asis_cls_lowres_bwd: too many tiles");
  const int ntiles = (int)nt;
  if (int rc = asis_dispatch16(dtype, "asis_cls_lowres_bwd", [&](auto t) {
        using T = decltype(t);
        const T* dh = static_cast<const T*>(d16);
        const T* dl = static_cast<const T*>(d_lo);
#define ASIS_CLS_BWD(CO)                                                                                                          \
  hipLaunchKernelGGL((cls_lowres_bwd_kernel<T, CO>), dim3(nblk), dim3(256), 0, s, dh, dl, CoP, raw, scale, shift, mean, invstd, w, g, \
                     partial, slabs, H, W, tx, ty, ntiles)
        if (Cout == 2) ASIS_CLS_BWD(2);
        else if (Cout == 3) ASIS_CLS_BWD(3);
        else ASIS_CLS_BWD(4);
#undef ASIS_CLS_BWD
      })) return rc;
  ASIS_CHECK_LAUNCH("asis_cls_lowres_bwd");
  return ASIS_OK;
}
