// Input gradient of a decoder stage's 3x3 conv COMMUTED with the transposed x2 upsampling of the stage below
// (`decoders.py:109-130`: Conv2d(Ck, Co, 3, padding=1) of stage i+1 behind BatchNorm2d, ReLU, Upsample(2, bilinear,
// align_corners=True) of stage i).  up^T acts on space and W_tap^T on channels, so
//   up^T( sum_tap W_tap^T shift_tap(d) ) = sum_tap W_tap^T up^T(shift_tap(d))
// and the channel product runs at [H, W] instead of [2H, 2W]: a quarter of the MFMA work, and the fp32 dU [B, 2H, 2W, Ck] is never
// written or read.  This is the wide-channel (MFMA) form of cls_lowres_bwd_kernel (clslowres.hip):
//   e[tap, c](i, j) = 1/4 sum_{Y, X} wy(Y, i) wx(X, j) d[c](Y - dy, X - dx)     d = d16 + d_lo; a position outside the map is dropped
//   g[k] = (raw[k] scale[k] + shift[k] > 0) ? 4 sum_{tap, c} w[c, k, tap] e[tap, c] : 0,   partial = sum g | sum g xhat
// The factor 1/4 (a pixel receives up to ~4x a gradient value) keeps e's f16 hi plane finite wherever d16 was; it is exact.
// Product: three 16-bit MFMA parts e_hi W_hi + e_lo W_hi + e_hi W_lo, fp32 accumulation.  No atomics, every sum in a fixed order.
#include "asis_common.h"

namespace {

constexpr int TY = 8, TX = 16;                  // low-resolution tile: 128 pixels = 8 MFMA blocks of one tile row each
constexpr int WR = 2 * TY + 5, WC = 2 * TX + 5; // gradient window of a tile: rows 2 ti0 - 2 .. 2 (ti0 + TY - 1) + 4
constexpr int WIN = WR * WC;
constexpr int WCH = (WC + 1) / 2;                 // window columns of one parity
constexpr int CC = 16;                          // gradient channels per K chunk
constexpr int KB = 5;                           // MFMA K blocks per chunk: k = tap * 16 + c, 144 values + 16 zeros
constexpr int EL = 168;                         // e rows: [pixel][hi: 144 values + zeros | lo at + EL], both planes behind one address
constexpr int ES = 344;                         // row pitch in 16-bit values (688 B: the 16 rows of a b128 read hit 16 different slots)
constexpr int NT = 512;                         // 8 waves = 2 (tile-row halves) x 4 (slices of Ck)
constexpr int NPF = (2 * WIN + NT - 1) / NT;    // 16-byte window loads per thread and plane
constexpr int MAXCK = 512;
constexpr size_t WIN_BYTES = (size_t)WR * 2 * WCH * CC * sizeof(float);
constexpr size_t E_BYTES = (size_t)TY * TX * ES * 2;   // hi and lo
constexpr size_t LDS_BYTES = WIN_BYTES + E_BYTES + (size_t)4 * MAXCK * sizeof(float) + (size_t)(TY + TX) * 5 * sizeof(float);

// LDS offset (floats) of window pixel (row, col).  SW: even and odd columns apart — the e phase reads columns 2 tj + v for 16 tj at
// once, all of one parity, and side by side they are consecutive 64-byte records.  It pays where the e phase reads 8 bytes per lane
// (512 k-channels: 339 -> 287 us); with 16-byte reads it measured neutral and costs registers, so those keep the plain rows.
template <bool SW> __device__ __forceinline__ int widx(int row, int col) {
  return SW ? ((row * 2 + (col & 1)) * WCH + (col >> 1)) * CC : (row * WC + col) * CC;
}

// source taps of output index o for align_corners=True: the expressions of bwd.hip / clslowres.hip
__device__ __forceinline__ void tap_ac_true(int o, float r, int in, int& i0, int& i1, float& l0, float& l1) {
  const float s = r * (float)o;
  i0 = (int)s;
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  l1 = s - (float)i0;
  l0 = 1.f - l1;
}

// w fp32 [Co][Ck][3][3] -> hi | lo planes [Co / 16][KB][Ck][32]: per chunk of 16 gradient channels and K block the 32 values
// k = tap * 16 + c of one k-channel are contiguous (one MFMA operand lane reads 8 of them); taps >= 9 are zeros
template <typename T>
__global__ __launch_bounds__(256) void dgrad_lowres_pack_kernel(const float* __restrict__ w, T* __restrict__ hi, T* __restrict__ lo,
                                                                int Ck, int64_t total) {
  for (int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (int64_t)gridDim.x * 256) {
    const int kk = (int)(o & 31);
    const int64_t r = o >> 5;
    const int n = (int)(r % Ck);
    const int64_t r2 = r / Ck;
    const int kb = (int)(r2 % KB), ch = (int)(r2 / KB);
    const int k = kb * 32 + kk, tap = k >> 4, c = ch * CC + (k & 15);
    const float v = tap < 9 ? w[((int64_t)c * Ck + n) * 9 + tap] : 0.f;
    hi[o] = to_t16<T>(v);
    lo[o] = to_t16<T>(lo_part<T>(v));
  }
}

// One workgroup walks tiles of TY x TX low-resolution pixels (grid-stride); per tile and chunk of 16 gradient channels:
//   staging   the tile's WR x WC window of d = d16 + d_lo as fp32 into LDS, zeros outside the map (never the neighbouring image);
//             the loads of chunk c + 1 are issued before the MFMA phase of chunk c and land in LDS after it
//   e phase   one thread per (pixel, 4 channels): the separable sums of cls_lowres_bwd_kernel (3 horizontal shifts per window row,
//             then the rows), written as hi + lo 16-bit planes [pixel][tap * 16 + c] = the MFMA operand rows
//   MFMA      wave (wm, wn) owns tile rows 4 wm .. 4 wm + 3 and the k-channels 16 NB wn .. 16 NB (wn + 1) - 1; the packed weights come
//             straight from memory (L2-resident: every workgroup reads the same chunk), accumulators stay in registers over the chunks
// Epilogue: D[n][pixel] (weights as the first operand), so a lane holds four consecutive k-channels of one pixel: ReLU mask, float4
// g store, BatchNorm sums over the tile's pixels by DPP row sums into the workgroup's LDS row (each slot has one owner).
template <typename T, int NB>
__global__ __launch_bounds__(NT) void dgrad_lowres_kernel(const T* __restrict__ dh, const T* __restrict__ dl, const T* __restrict__ wh,
                                                          const T* __restrict__ wl, const float* __restrict__ raw,
                                                          const float* __restrict__ scale, const float* __restrict__ shift,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          float* __restrict__ g, float* __restrict__ partial, int H, int W, int Co,
                                                          int tiles_x, int tiles_y, int ntiles) {
  constexpr int CK = 64 * NB;
  // registers: 16 NB accumulators per lane.  Up to 128 k-channels a window is held across the MFMA phase; with 512 the e phase
  // also takes its four channels in two passes
  constexpr bool PF = NB < 4;
  constexpr int EC = NB < 8 ? 4 : 2;
  constexpr bool SW = NB == 8;
  using v8 = typename T16<T>::v8;
  extern __shared__ __attribute__((aligned(16))) char lds[];
  float* const win = reinterpret_cast<float*>(lds);
  T* const eh = reinterpret_cast<T*>(lds + WIN_BYTES);
  T* const el = eh + EL;
  float* const sums = reinterpret_cast<float*>(lds + WIN_BYTES + E_BYTES);  // [wm][2][CK]
  float* const wyt = sums + 4 * MAXCK;                                           // [TY][5], carries the factor 1/4
  float* const wxt = wyt + TY * 5;                                               // [TX][5]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 2, wn = wave & 3, l15 = lane & 15, q = lane >> 4;
  const int OH = 2 * H, OW = 2 * W;
  const float rh = (float)(H - 1) / (float)(OH - 1), rw = (float)(W - 1) / (float)(OW - 1);
  const int nch = Co / CC;
  for (int i = t; i < TY * TX * (EL - 9 * CC); i += NT) {   // the zero tail of every e row (k = 144 .. 167): never written again
    const int p = i / (EL - 9 * CC), k = 9 * CC + i % (EL - 9 * CC);
    eh[p * ES + k] = (T)0.f;
    el[p * ES + k] = (T)0.f;
  }
  for (int i = t; i < 4 * CK; i += NT) sums[i] = 0.f;

  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int b = tile / (tiles_x * tiles_y), tr = tile - b * (tiles_x * tiles_y);
    const int ti0 = (tr / tiles_x) * TY, tj0 = (tr % tiles_x) * TX;
    if (t < (TY + TX) * 5) {
      // tap tables of the tile: weight of output index 2 i - 1 + m (m = 0..4) on source index i, rows then columns
      const int isx = t >= TY * 5, qq = isx ? t - TY * 5 : t;
      const int i = (isx ? tj0 : ti0) + qq / 5, in = isx ? W : H;
      const int o = 2 * i - 1 + qq % 5;
      float wt = 0.f;
      if (i < in && o >= 0 && o < 2 * in) {
        int a0, a1; float l0, l1;
        tap_ac_true(o, isx ? rw : rh, in, a0, a1, l0, l1);
        wt = ((a0 == i) ? l0 : 0.f) + ((a1 == i) ? l1 : 0.f);
      }
      if (isx) wxt[qq] = wt; else wyt[qq] = 0.25f * wt;
    }
    uint4 ph[NPF], pl[NPF];
    uint32_t poff[NPF];   // byte offset of the thread's window pixels inside image b (uniform base + 32-bit lane offset), ~0u = outside
#pragma unroll
    for (int r = 0; r < NPF; ++r) {
      const int it = t + NT * r, px = it >> 1, hf = it & 1;
      const int row = px / WC, col = px - row * WC;
      const int Y = 2 * ti0 - 2 + row, X = 2 * tj0 - 2 + col;
      poff[r] = (it < 2 * WIN && (unsigned)Y < (unsigned)OH && (unsigned)X < (unsigned)OW)
                    ? (uint32_t)(((Y * OW + X) * Co + hf * 8) * sizeof(T)) : ~0u;
    }
    const int64_t img = (int64_t)b * OH * OW * Co;
    auto prefetch = [&](int ch) {
      const char* bh_ = reinterpret_cast<const char*>(dh + img + ch * CC);
      const char* bl_ = reinterpret_cast<const char*>(dl ? dl + img + ch * CC : nullptr);
#pragma unroll
      for (int r = 0; r < NPF; ++r) {
        ph[r] = make_uint4(0u, 0u, 0u, 0u);
        pl[r] = ph[r];
        if (poff[r] != ~0u) {
          ph[r] = *reinterpret_cast<const uint4*>(bh_ + poff[r]);
          if (dl) pl[r] = *reinterpret_cast<const uint4*>(bl_ + poff[r]);
        }
      }
    };
    auto stage = [&]() {
#pragma unroll
      for (int r = 0; r < NPF; ++r) {
        const int it = t + NT * r;
        if (it < 2 * WIN) {
          float h[8], l[8];
          unpack2<T>(ph[r].x, h[0], h[1]); unpack2<T>(ph[r].y, h[2], h[3]); unpack2<T>(ph[r].z, h[4], h[5]); unpack2<T>(ph[r].w, h[6], h[7]);
          unpack2<T>(pl[r].x, l[0], l[1]); unpack2<T>(pl[r].y, l[2], l[3]); unpack2<T>(pl[r].z, l[4], l[5]); unpack2<T>(pl[r].w, l[6], l[7]);
          const int px = it >> 1, row = px / WC;
          float4* wp = reinterpret_cast<float4*>(win + widx<SW>(row, px - row * WC) + (it & 1) * 8);
          wp[0] = make_float4(h[0] + l[0], h[1] + l[1], h[2] + l[2], h[3] + l[3]);
          wp[1] = make_float4(h[4] + l[4], h[5] + l[5], h[6] + l[6], h[7] + l[7]);
        }
      }
    };
    if constexpr (PF) prefetch(0);
    f32x4 acc[4][NB];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) acc[m][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int ch = 0; ch < nch; ++ch) {
      if constexpr (!PF) prefetch(ch);
      stage();
      __syncthreads();  // window and tap tables are in place; every wave has finished the MFMA phase that read e
      {  // ---- e phase: pixel (ti, tj) of the tile, channels 4 cg .. 4 cg + 3 of the chunk, EC of them per pass
        const int p = t >> 2, cg = t & 3, ti = p >> 4, tj = p & 15;
        const int i = ti0 + ti, j = tj0 + tj;
        const bool live = i < H && j < W;
        float wy[5], wx[5];
#pragma unroll
        for (int m = 0; m < 5; ++m) { wy[m] = wyt[ti * 5 + m]; wx[m] = wxt[tj * 5 + m]; }
#pragma unroll 1
        for (int c0 = 4 * cg; c0 < 4 * cg + 4; c0 += EC) {
          float e[3][3][EC];
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
              for (int c = 0; c < EC; ++c) e[ky][kx][c] = 0.f;
          if (live) {
#pragma unroll
            for (int u = 0; u < 7; ++u) {          // gradient row 2 i - 2 + u = Y - dy: window row 2 ti + u
              float dv[7][EC];
#pragma unroll
              for (int v = 0; v < 7; ++v) {        // gradient column 2 j - 2 + v = X - dx: window column 2 tj + v
                const float* wp = win + (SW ? (((2 * ti + u) * 2 + (v & 1)) * WCH + tj + (v >> 1)) * CC   // = widx(2 ti + u, 2 tj + v)
                                             : widx<false>(2 * ti + u, 2 * tj + v)) + c0;
                if constexpr (EC == 4) {
                  const float4 d = *reinterpret_cast<const float4*>(wp);
                  dv[v][0] = d.x; dv[v][1] = d.y; dv[v][2] = d.z; dv[v][3] = d.w;
                } else {
                  const float2 d = *reinterpret_cast<const float2*>(wp);
                  dv[v][0] = d.x; dv[v][1] = d.y;
                }
              }
#pragma unroll
              for (int kx = 0; kx < 3; ++kx) {
                float h[EC];
#pragma unroll
                for (int c = 0; c < EC; ++c) h[c] = 0.f;
#pragma unroll
                for (int m = 0; m < 5; ++m)        // X = 2 j - 1 + m, column X - dx = 2 j - 2 + (m + 2 - kx)
#pragma unroll
                  for (int c = 0; c < EC; ++c) h[c] += wx[m] * dv[m + 2 - kx][c];
#pragma unroll
                for (int ky = 0; ky < 3; ++ky) {   // Y = row + dy = 2 i - 1 + (u - 2 + ky)
                  const int m = u - 2 + ky;
                  if (m < 0 || m > 4) continue;
#pragma unroll
                  for (int c = 0; c < EC; ++c) e[ky][kx][c] += wy[m] * h[c];
                }
              }
              __builtin_amdgcn_sched_barrier(0);   // one window row at a time: all 49 loads up front would not fit the register file
            }
          }
#pragma unroll
          for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
              const float* v = e[ky][kx];
              const int o = p * ES + (ky * 3 + kx) * CC + c0;
              if constexpr (EC == 4) {
                *reinterpret_cast<uint2*>(eh + o) = make_uint2(pack2<T>(v[0], v[1]), pack2<T>(v[2], v[3]));
                *reinterpret_cast<uint2*>(el + o) =
                    make_uint2(pack2<T>(lo_part<T>(v[0]), lo_part<T>(v[1])), pack2<T>(lo_part<T>(v[2]), lo_part<T>(v[3])));
              } else {
                *reinterpret_cast<uint32_t*>(eh + o) = pack2<T>(v[0], v[1]);
                *reinterpret_cast<uint32_t*>(el + o) = pack2<T>(lo_part<T>(v[0]), lo_part<T>(v[1]));
              }
            }
        }
      }
      __syncthreads();
      if constexpr (PF) {
        if (ch + 1 < nch) prefetch(ch + 1);
      }
      // ---- MFMA phase: D[n][pixel] += W'[n][k] e[pixel][k]
      const T* whc = wh + (int64_t)ch * KB * CK * 32;
      const T* wlc = wl + (int64_t)ch * KB * CK * 32;
      // uniform base + one 32-bit lane offset for every fragment of the chunk
      const uint32_t wlane = (uint32_t)(((wn * NB * 16 + l15) * 32 + 8 * q) * sizeof(T));
      auto ldw = [&](const T* base, int step) {   // step = kb * NB + nb
        const int kb = step / NB, nb = step - kb * NB;
        const char* ub = reinterpret_cast<const char*>(base + (kb * CK + nb * 16) * 32);
        return __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(ub + wlane));
      };
      // the weight fragments of step s + PD are fetched before the MFMAs of step s; the fence keeps the scheduler from hoisting more
      // of them (every fragment of the chunk at once does not fit the register file beside the accumulators)
      constexpr int PD = 2, NS = KB * NB;   // two steps ahead: 564 -> 529, 420 -> 378, 339 -> 309 us against one (12 images, 588^2)
      v8 qh[PD], ql[PD];
#pragma unroll
      for (int s2 = 0; s2 < PD; ++s2) { qh[s2] = ldw(whc, s2); ql[s2] = ldw(wlc, s2); }
      v8 ah[4], al[4];
#pragma unroll
      for (int step = 0; step < NS; ++step) {
        const int kb = step / NB, nb = step - kb * NB;
        if (nb == 0) {
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const int o = ((wm * 4 + m) * 16 + l15) * ES + kb * 32 + 8 * q;
            ah[m] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(eh + o));
            al[m] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(el + o));
          }
        }
        const v8 bh = qh[step % PD], bl = ql[step % PD];
        if (step + PD < NS) { qh[step % PD] = ldw(whc, step + PD); ql[step % PD] = ldw(wlc, step + PD); }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          acc[m][nb] = T16<T>::mfma16(bh, ah[m], acc[m][nb]);
          acc[m][nb] = T16<T>::mfma16(bh, al[m], acc[m][nb]);
          acc[m][nb] = T16<T>::mfma16(bl, ah[m], acc[m][nb]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // ---- epilogue: lane (q, l15) holds k-channels n0 .. n0 + 3 of the pixels (ti0 + 4 wm + m, tj0 + l15)
    // the per-channel vectors are read here, per tile (L1 hits): hoisted out of the tile loop they would take 16 NB registers
    const float *scp = scale, *shp = shift, *mup = mean, *isp = invstd;
    asm volatile("" : "+s"(scp), "+s"(shp), "+s"(mup), "+s"(isp));
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int n0 = (wn * NB + nb) * 16 + 4 * q;
      const float4 sc = *reinterpret_cast<const float4*>(scp + n0), sh = *reinterpret_cast<const float4*>(shp + n0);
      const float4 mu = *reinterpret_cast<const float4*>(mup + n0), is = *reinterpret_cast<const float4*>(isp + n0);
      float4 s1 = make_float4(0.f, 0.f, 0.f, 0.f), s2 = s1;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int i = ti0 + wm * 4 + m, j = tj0 + l15;
        if (i < H && j < W) {
          const int64_t idx = (((int64_t)b * H + i) * W + j) * CK + n0;
          const float4 xv = *reinterpret_cast<const float4*>(raw + idx);
          const f32x4 a = acc[m][nb];
          float4 gg;   // the ReLU mask: the fp32 expression of upsample_bn_relu_bwd_kernel
          gg.x = (xv.x * sc.x + sh.x > 0.f) ? 4.f * a[0] : 0.f;
          gg.y = (xv.y * sc.y + sh.y > 0.f) ? 4.f * a[1] : 0.f;
          gg.z = (xv.z * sc.z + sh.z > 0.f) ? 4.f * a[2] : 0.f;
          gg.w = (xv.w * sc.w + sh.w > 0.f) ? 4.f * a[3] : 0.f;
          *reinterpret_cast<float4*>(g + idx) = gg;
          s1.x += gg.x; s1.y += gg.y; s1.z += gg.z; s1.w += gg.w;
          s2.x += gg.x * (xv.x - mu.x) * is.x;
          s2.y += gg.y * (xv.y - mu.y) * is.y;
          s2.z += gg.z * (xv.z - mu.z) * is.z;
          s2.w += gg.w * (xv.w - mu.w) * is.w;
        }
      }
      // the 16 pixels of the tile rows: DPP row sums (all 64 lanes are active here), then the slot's one owner adds
      s1.x = row16_sum(s1.x); s1.y = row16_sum(s1.y); s1.z = row16_sum(s1.z); s1.w = row16_sum(s1.w);
      s2.x = row16_sum(s2.x); s2.y = row16_sum(s2.y); s2.z = row16_sum(s2.z); s2.w = row16_sum(s2.w);
      if (l15 == 0) {
        float4* a1 = reinterpret_cast<float4*>(sums + (wm * 2 + 0) * CK + n0);
        float4* a2 = reinterpret_cast<float4*>(sums + (wm * 2 + 1) * CK + n0);
        float4 u = *a1, v = *a2;
        u.x += s1.x; u.y += s1.y; u.z += s1.z; u.w += s1.w;
        v.x += s2.x; v.y += s2.y; v.z += s2.z; v.w += s2.w;
        *a1 = u;
        *a2 = v;
      }
    }
  }

  __syncthreads();
  for (int c = t; c < 2 * CK; c += NT)   // [2][CK]: the two tile-row halves, upper first
    partial[(int64_t)blockIdx.x * 2 * CK + c] = sums[c] + sums[2 * CK + c];
}

int tiles_y_of(int H) { return (H + TY - 1) / TY; }
int tiles_x_of(int W) { return (W + TX - 1) / TX; }

// the kernel's 147.8 KB of dynamic LDS need the attribute on the device the launch goes to: set before every launch (it is cheap)
template <typename T, int NB> int set_lds() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&dgrad_lowres_kernel<T, NB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)LDS_BYTES) != hipSuccess;
}

int g_wg_cap = 2048;   // most workgroups of one launch: asis_dgrad_lowres_cap

}  // namespace

// workgroups = rows of `partial`: an equal run of tiles each, at most the cap (2048); 0 for a map that is none
extern "C" int asis_dgrad_lowres_nblk(int B, int H, int W) {
  if (B < 1 || H < 1 || W < 1) return 0;
  const int64_t ntiles = (int64_t)B * tiles_y_of(H) * tiles_x_of(W);
  const int64_t per = (ntiles + g_wg_cap - 1) / g_wg_cap;
  return (int)((ntiles + per - 1) / per);
}

// sets the most workgroups a launch may have (1 .. 65536; anything else restores 2048) and returns the former value: with a small cap
// a small map runs several tiles per workgroup, the path of the large maps (tests; tuning)
extern "C" int asis_dgrad_lowres_cap(int cap) {
  const int old = g_wg_cap;
  g_wg_cap = (cap >= 1 && cap <= 65536) ? cap : 2048;
  return old;
}

extern "C" int asis_dgrad_lowres_pack(void* stream, int dtype, const float* w, void* w_hi, void* w_lo, int Co, int Ck) {
  ASIS_REQUIRE(w && w_hi && w_lo, "asis_dgrad_lowres_pack: null pointer");
  ASIS_REQUIRE(Co >= CC && Co % CC == 0 && Co <= 4096 && (Ck == 128 || Ck == 256 || Ck == 512),
               "asis_dgrad_lowres_pack: Co=%d must be a multiple of 16, Ck=%d one of 128, 256, 512", Co, Ck);
  ASIS_REQUIRE(asis_aligned16(w_hi) && asis_aligned16(w_lo), "asis_dgrad_lowres_pack: alignment");
  ASIS_DT_OK(dtype, "asis_dgrad_lowres_pack");
  const int64_t total = (int64_t)(Co / CC) * KB * Ck * 32;
  if (int rc = asis_dispatch16(dtype, "asis_dgrad_lowres_pack", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((dgrad_lowres_pack_kernel<T>), dim3(asis_grid(total, 256, 2048)), dim3(256), 0,
                           reinterpret_cast<hipStream_t>(stream), w, static_cast<T*>(w_hi), static_cast<T*>(w_lo), Ck, total);
      })) return rc;
  ASIS_CHECK_LAUNCH("asis_dgrad_lowres_pack");
  return ASIS_OK;
}

extern "C" int asis_dgrad_lowres(void* stream, int dtype, const void* d16, const void* d_lo, const void* w_hi, const void* w_lo,
                                 const float* raw, const float* scale, const float* shift, const float* mean, const float* invstd,
                                 float* g, float* partial, int nblk, int B, int H, int W, int Co, int Ck) {
  ASIS_REQUIRE(d16 && w_hi && w_lo && raw && scale && shift && mean && invstd && g && partial, "asis_dgrad_lowres: null pointer");
  ASIS_REQUIRE(B > 0 && H >= 2 && W >= 2 && H < (1 << 24) && W < (1 << 24), "asis_dgrad_lowres: the map %d x %d x %d must be at least 2 x 2",
               B, H, W);
  ASIS_REQUIRE(Co >= CC && Co % CC == 0 && Co <= 4096 && (Ck == 128 || Ck == 256 || Ck == 512),
               "asis_dgrad_lowres: Co=%d must be a multiple of 16, Ck=%d one of 128, 256, 512", Co, Ck);
  ASIS_REQUIRE((int64_t)H * W * Co < (1 << 27), "asis_dgrad_lowres: %d x %d x %d: one image of the gradient must stay below 2^30 bytes", H, W, Co);
  ASIS_REQUIRE(nblk == asis_dgrad_lowres_nblk(B, H, W), "asis_dgrad_lowres: nblk=%d, asis_dgrad_lowres_nblk gives %d", nblk,
               asis_dgrad_lowres_nblk(B, H, W));
  ASIS_REQUIRE(asis_aligned16(d16) && (!d_lo || asis_aligned16(d_lo)) && asis_aligned16(w_hi) && asis_aligned16(w_lo) &&
               asis_aligned16(raw) && asis_aligned16(scale) && asis_aligned16(shift) && asis_aligned16(mean) && asis_aligned16(invstd) &&
               asis_aligned16(g) && asis_aligned16(partial), "asis_dgrad_lowres: alignment");
  ASIS_DT_OK(dtype, "asis_dgrad_lowres");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int tx = tiles_x_of(W), ty = tiles_y_of(H);
  const int64_t nt = (int64_t)B * tx * ty;
  ASIS_REQUIRE(nt < (1 << 30), "asis_dgrad_lowres: too many tiles");
  const int ntiles = (int)nt;
  int bad = 0;
  if (int rc = asis_dispatch16(dtype, "asis_dgrad_lowres", [&](auto t) {
        using T = decltype(t);
        const T* dh = static_cast<const T*>(d16);
        const T* dl = static_cast<const T*>(d_lo);
        const T* wh = static_cast<const T*>(w_hi);
        const T* wl = static_cast<const T*>(w_lo);
#define ASIS_DGRAD_LOWRES(NBV)                                                                                                       \
  do {                                                                                                                               \
    bad = set_lds<T, NBV>();                                                                                                         \
    if (!bad)                                                                                                                        \
      hipLaunchKernelGGL((dgrad_lowres_kernel<T, NBV>), dim3(nblk), dim3(NT), LDS_BYTES, s, dh, dl, wh, wl, raw, scale, shift, mean, \
                         invstd, g, partial, H, W, Co, tx, ty, ntiles);                                                             \
  } while (0)
        if (Ck == 128) ASIS_DGRAD_LOWRES(2);
        else if (Ck == 256) ASIS_DGRAD_LOWRES(4);
        else ASIS_DGRAD_LOWRES(8);
#undef ASIS_DGRAD_LOWRES
      })) return rc;
  if (bad) ASIS_FAIL(ASIS_ELAUNCH, "asis_dgrad_lowres: %zu bytes of LDS refused", LDS_BYTES);
  ASIS_CHECK_LAUNCH("asis_dgrad_lowres");
  return ASIS_OK;
}
