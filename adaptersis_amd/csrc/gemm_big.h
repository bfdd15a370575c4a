// Large-tile LDS-DMA GEMM kernel (included by gemm.hip and by scripts/gemm_lab.hip).
#pragma once
#include <type_traits>

#include "asis_common.h"

namespace {
// ------------------------------------------------------------------------------------------------
// Large-tile dense GEMM: 256 x (256|128) x 64 tile, 8 waves, LDS-DMA (global_load_lds_dwordx4) staging
// with NS LDS stages and a counted vmcnt so NS-1 K tiles stay in flight across the one barrier per
// K tile.  The 128^2 register-staged kernel above is latency/inflow bound (~10 B/clk/CU reach the CU
// while one 32 KB tile per workgroup is in flight: 64 FLOP/B x 10 B/clk = ~15 % of the MFMA peak,
// which is what it measures); this kernel doubles the FLOP per staged byte and keeps 2 tiles
// (96-128 KB per CU) in flight.  Forms in production (gemm.hip): PH8 + M16 = the 8-phase 256x256x64 main loop on 16x16x32 MFMAs
// (every K >= 1024 GEMM with >= 128 tiles, wide convolutions; 16-bit outputs leave through a 16-bit LDS slab), the
// 256x128x32 two-workgroup form for the rest.  LDS image = the same XOR-swizzled 128-B rows; since LDS-DMA writes
// lane-linear (base + lane*16) the swizzle is applied to the per-lane SOURCE address instead
// (cdna_hip_programming.md rule 21).  Rows/cols beyond M/N are clamped on load and masked on store.
// ------------------------------------------------------------------------------------------------
// 16 zero bytes: the LDS-DMA source of implicit-im2col lanes that fall into the conv padding
__device__ __attribute__((aligned(16))) uint4 g_zero_page[1];

// Which epilogue gemm_big_kernel runs for a batch entry / K part (cbase, res: its output offset and its residual): true = the
// vector epilogue (16-byte accesses of C, bias_n, scale_n and res, four columns per lane), false = the scalar fallback.  ONE
// predicate for the kernel and for gemm_plan (gemm.hip): the fallback writes no statistics, applies no GELU' and knows no K
// parts, so the plan refuses such launches instead of letting the kernel drop them.
__host__ __device__ __forceinline__ bool gemm_big_vec_epilogue(const asis_gemm_desc& d, int64_t cbase, const float* res) {
  return ((d.N & 3) == 0) && ((d.ldc & 3) == 0) && ((cbase & 3) == 0) && (!res || (d.ldr & 3) == 0) &&
         ((reinterpret_cast<uintptr_t>(d.C) & 15) == 0) && (!res || (reinterpret_cast<uintptr_t>(res) & 15) == 0) &&
         (!d.bias_n || (reinterpret_cast<uintptr_t>(d.bias_n) & 15) == 0) &&
         (!d.scale_n || (reinterpret_cast<uintptr_t>(d.scale_n) & 15) == 0);
}

template <typename T, int WM, int WN, int TM, int TN, int NS, int DBG = 0, bool CONV = false, bool SPLIT = false, int BKT = 64,
          int OCC = 2, bool PH8 = false, bool M16 = false, int LNF = 0, bool MXC = false>
__global__ __launch_bounds__(WM * WN * 64, OCC) void gemm_big_kernel(const asis_gemm_desc d, const int GROUP_M_FLAGS) {
  const int GROUP_M = GROUP_M_FLAGS & 0xffff;        // raster group height; bit 16 (lab): fp32 slab epilogue for every output type
  static_assert(!PH8 || (WM == 2 && WN == 4 && TM == 4 && TN == 2 && NS == 2 && BKT == 64),
                "the 8-phase main loop is written for the 256x256x64 tile, 2x4 waves of 128x64");
  // MXC: split convolution whose lo operands are in the MX form (asis_common.h: two fp8 bytes per element, activations
  // (hi8, lo8), weights (lo8, hi8)): TWO K parts instead of three — (A, B) on the 16-bit MFMA, then (A_mx, B_mx) on
  // v_mfma_scale_f32_16x16x128_f8f6f4, whose byte-with-byte products are both correction terms at once.  Same LDS image, same
  // staging and fragment reads as a 16-bit part (a row of a K tile is 128 bytes = 64 elements either way); the two ks
  // fragments of a lane are the two halves of its 32-byte fp8 operand (K pairing: scripts/mx_probe.hip).
  // Dense MXC (round 4: the split-precision linear layers of config.precise_level 2): the same two parts, K tiles alternating
  // 16-bit / MX over the same k offset, A rows by plain per-lane pointers.
  static_assert(!MXC || (SPLIT && M16 && BKT == 64 && (CONV || PH8)), "the MX correction pass is built for split operands on 16x16 MFMAs");
  typedef int v4i_ __attribute__((ext_vector_type(4)));
  typedef int v8i_ __attribute__((ext_vector_type(8)));
  auto cat8 = [](auto lo8, auto hi8) -> v8i_ {
    return __builtin_shufflevector(__builtin_bit_cast(v4i_, lo8), __builtin_bit_cast(v4i_, hi8), 0, 1, 2, 3, 4, 5, 6, 7);
  };
  const int mx_sc = MXC ? mx_code<T>(*d.mx_amax_a, *d.mx_amax_b) : 0;   // E8M0 scale of the correction pass (wave-uniform)
  // The scaled MFMA through inline asm with the accumulator TIED (dst = C): the builtin's result landed in a fresh register
  // tuple (v_mfma_scale ... v[66:69], ..., v[166:169]), i.e. four copies per MFMA and 19 spilled VGPRs in the 8-phase form —
  // the correction pass ran at half the speed of the 16-bit parts it replaces.  Operands are complete when it issues (every
  // call site sits behind the fragment reads' s_waitcnt lgkmcnt(0)); its result is next touched tiles later.
  auto mfma_mx = [](f32x4& acc, v8i_ a, v8i_ b, int sa, int sb) {
    asm volatile("v_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]" : "+v"(acc) : "v"(a), "v"(b), "v"(sa), "v"(sb));
  };
  const int mx_one = 127;
  // M16: the wave tile is built from v_mfma_f32_16x16x32 (one K = 32 step per MFMA) instead of 32x32x16: same FLOP per
  // cycle and the same LDS bytes per FLOP, but the chip holds a higher clock under this shape (MI355X_MICROARCH.md,
  // DVFS give-back item 7: 1.12-1.14x the FLOP/s of the 32x32x16 loop with LDS-fed operands on random data)
  typedef typename T16<T>::v8 v8;
  constexpr int BM2 = WM * TM * 32, BN2 = WN * TN * 32;
  constexpr int BKB = BKT;                           // K tile (64 or 32)
  constexpr int CPR = BKB / 8;                       // 16-byte chunks per LDS row
  constexpr int RPI = 64 / CPR;                      // rows covered by one 1-KB LDS-DMA wave-instruction
  constexpr int SWS = (CPR == 8) ? 1 : 2;            // swizzle: chunk ^= (row >> SWS) & (CPR-1)  (conflict-free b128 reads)
  constexpr int STAGE = (BM2 + BN2) * BKB;           // elements per stage
  constexpr int NWV = WM * WN;                       // waves per workgroup (8, or 4 with 128x64 wave tiles)
  constexpr int GA = BM2 / RPI / NWV, GB = BN2 / RPI / NWV;  // LDS-DMA wave-instructions per wave and K tile
  constexpr int G = GA + GB;
  __shared__ __attribute__((aligned(16))) T lds[NS * STAGE];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wid / WN, wn = wid - wm * WN;
  uint64_t dbg_c0 = 0, dbg_r0 = 0;
  if (DBG & 4) asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(dbg_c0), "=s"(dbg_r0)::"memory");
  const int tiles_n = (d.N + BN2 - 1) / BN2;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  // grouped raster: 8 row tiles x tiles_n column tiles per band, column-major inside the band, so the ~64 tiles an
  // XCD runs at once cover ~8x8 tiles (A and W slices of a few MB: both stay in that XCD's 4 MB L2) instead of
  // 2 rows x 32 columns (all of W re-fetched per band: measured 2.8x the algorithmic reads, profiles/r01_pmc_traffic)
  const int tiles_m = (d.M + BM2 - 1) / BM2;
  const int band = bid / (GROUP_M * tiles_n);
  const int first_m = band * GROUP_M;
  const int band_m = (tiles_m - first_m) < GROUP_M ? (tiles_m - first_m) : GROUP_M;
  const int in_band = bid - band * GROUP_M * tiles_n;
  const int tile_n = in_band / band_m;
  const int tile_m = first_m + (in_band - tile_n * band_m);
  const int m0 = tile_m * BM2, n0 = tile_n * BN2;
  const int bz = blockIdx.y;
  const T* __restrict__ A = reinterpret_cast<const T*>(d.A) + (int64_t)bz * d.strideA;
  const T* __restrict__ B = reinterpret_cast<const T*>(d.B) + (int64_t)bz * d.strideB;

  // per-lane source pointers (row clamped, chunk pre-swizzled) for this wave's DMA instructions
  const T* asrc[GA];
  const T* bsrc[GB];
  int a_ih0[GA], a_iw0[GA];  // CONV: top-left input pixel of this lane's output pixel
  // MXC instances (at the register limit): the same per-lane state in half the registers — 32-bit element offsets from the
  // wave-uniform operand bases (the host checks that both tensors hold < 2^31 elements) and (ih0 + pad, iw0 + pad) packed
  uint32_t a_pix[GA], a_hw[GA], b_off[GB];
  const int lr = lane / CPR, lc = lane % CPR;
  // LDS image swizzle (applied to the DMA source chunk and to the fragment reads alike): chunk ^= swz(row).
  // 32x32x16 fragments (lane -> row lane&31, chunk 2ks + lane>>5): (row >> SWS) & (CPR-1).  16x16x32 fragments (lane -> row
  // lane&15, chunk lane>>4, 64-byte rows): a b128 read is served in the lane groups {0-3,12-15,20-27} ... of
  // MI355X_MICROARCH.md §LDS; rows r, r+4, r+8, r+12 share their 64-byte bank quarter, so their chunks must differ inside
  // a group: s(r) = (-(r >> 2)) & 3 gives {0, 1^3, 1^2, 1} = {0, 2, 3, 1} for the first group and likewise for the others.
  // With 128-byte rows (BK = 64) the standard swizzle (row >> 1) & 7 is conflict-free for both fragment shapes.
  auto swz = [&](int row) -> int { return (M16 && CPR == 4) ? ((-(row >> 2)) & 3) : ((row >> SWS) & (CPR - 1)); };
  // first tile row / column of the 8-row group that this wave's j-th LDS-DMA instruction stages.  Default: the wave's
  // own stripe.  PH8: instructions 0,1 stage the row halves 0 of both wave rows ({0..63, 128..191}), 2,3 the halves 1;
  // for B the column halves 0 / 1 of the four wave columns — the order in which the phases consume them.
  auto grp_a = [&](int j) -> int {
    if (PH8) { const int g = wid * 2 + (j & 1); return (g < 8 ? 0 : 128) + (j >> 1) * 64 + (g & 7) * 8; }
    return (wid * GA + j) * RPI;
  };
  auto grp_b = [&](int j) -> int {
    if (PH8) { const int g = wid * 2 + (j & 1); return (g >> 2) * 64 + (j >> 1) * 32 + (g & 3) * 8; }
    return (wid * GB + j) * RPI;
  };
#pragma unroll
  for (int j = 0; j < GA; ++j) {
    const int row = grp_a(j) + lr;
    int gr = m0 + row;
    gr = gr < d.M ? gr : d.M - 1;
    if (CONV) {  // implicit im2col: A is NHWC [B,H,W,Cin]; a K tile (64) lies inside one tap (Cin % 64 == 0)
      const int ohw = d.OH * d.OW;
      const int b = gr / ohw;
      const int rem = gr - b * ohw;
      const int oh = rem / d.OW, ow = rem - oh * d.OW;
      a_ih0[j] = oh * d.stride - d.pad;
      a_iw0[j] = ow * d.stride - d.pad;
      asrc[j] = A + (int64_t)b * d.H * d.W * d.Cin + ((lc ^ swz(row)) << 3);
      a_pix[j] = (uint32_t)(b * d.H * d.W * d.Cin + ((lc ^ swz(row)) << 3));
      a_hw[j] = ((uint32_t)(oh * d.stride) << 16) | (uint32_t)(ow * d.stride);
    } else {
      a_ih0[j] = a_iw0[j] = 0;
      asrc[j] = A + (int64_t)gr * d.lda + ((lc ^ swz(row)) << 3);
    }
  }
#pragma unroll
  for (int j = 0; j < GB; ++j) {
    const int row = grp_b(j) + lr;
    int gr = n0 + row;
    gr = gr < d.N ? gr : d.N - 1;
    bsrc[j] = B + (int64_t)gr * d.ldb + ((lc ^ swz(row)) << 3);
    b_off[j] = (uint32_t)(gr * (int)d.ldb + ((lc ^ swz(row)) << 3));
  }
  // SPLIT: the reduction runs over three K-long parts: (A, B), (A_lo, B), (A, B_lo); the lo halves share the
  // layout of the hi ones, so a part only changes the base pointers by a constant element offset.
  // One-sided split (only A_lo or only B_lo given: the WEIGHT operand of a linear layer, whose rounding error is the same
  // for every token and therefore adds up coherently through the blocks, tests/precision_probe.py): two parts.
  const int64_t a_lo_off = (SPLIT && d.A_lo) ? (reinterpret_cast<const T*>(d.A_lo) - reinterpret_cast<const T*>(d.A)) : 0;
  const int64_t b_lo_off = (SPLIT && d.B_lo) ? (reinterpret_cast<const T*>(d.B_lo) - reinterpret_cast<const T*>(d.B)) : 0;
  const int nparts = !SPLIT ? 1 : (MXC ? 2 : (CONV ? 3 : ((d.A_lo && d.B_lo) ? 3 : 2)));   // convolutions always carry both halves
  // part p > 0 of a two-part reduction adds the one lo operand that exists; of a three-part one: 1 = A_lo, 2 = B_lo
  auto part_offs = [&](int part, int64_t& aoff, int64_t& boff) {
    aoff = (part == 1 && d.A_lo) ? a_lo_off : 0;
    boff = ((part == 2) || (part == 1 && !d.A_lo)) ? b_lo_off : 0;
  };
  // ksplit > 1: blockIdx.y is a K part, not a batch entry (the host passes zero A/B batch strides)
  const int ksp = d.ksplit > 1 ? d.ksplit : 1;
  const int nt1 = d.K / ksp / BKB;
  const int kt_base = ksp > 1 ? bz * nt1 : 0;
  const int ntap_part = CONV ? (d.KH * d.KW) / ksp : 1;  // conv K parts are whole taps (kernel rows for a 3x3 in three)
  const int tap_base = (CONV && ksp > 1) ? bz * ntap_part : 0;
  typedef __attribute__((address_space(3))) void* lds_ptr;
  typedef const __attribute__((address_space(1))) void* glb_ptr;
  auto issue = [&](int t) {
    T* st = lds + (t % NS) * STAGE;
    int kt = t;
    int64_t aoff = 0, boff = 0;
    int k0;
    if (CONV) {
      // Reduction order of a convolution: channel chunk outermost, then the taps, then (SPLIT) the three hi/lo parts.
      // A chunk of 64 channels of the ~2.3 image rows a 256-pixel tile touches is ~75 KB; all 9 taps and all parts of it
      // are consumed back to back, so they hit in L1 / L2.  Tap-major order (the layout order of the packed weights)
      // came back to the same pixels only after a whole sweep over Cin, by which time the 64 tiles resident on an XCD
      // had pushed them out of its 4 MB L2: 3.2x the tensor bytes in L2 fills (profiles/r01_pmc_traffic.json).
      int tt = t, part = 0;
      if (SPLIT && MXC) {  // two parts: 16-bit (A, B), then the MX pair (A_mx, B_mx)
        tt = t >> 1;
        part = t & 1;
        aoff = part ? a_lo_off : 0;
        boff = part ? b_lo_off : 0;
      } else if (SPLIT) {  // CONV: three parts, compile-time divisor (a runtime one costs ~30 instructions per issue)
        tt = t / 3;
        part = t - 3 * tt;
        aoff = part == 1 ? a_lo_off : 0;
        boff = part == 2 ? b_lo_off : 0;
      }
      const int c = tt / ntap_part, tl = tt - c * ntap_part;
      k0 = (tap_base + tl) * d.Cin + c * BKB;
    } else {
      if (SPLIT && MXC) {
        kt = t >> 1;
        aoff = (t & 1) ? a_lo_off : 0;
        boff = (t & 1) ? b_lo_off : 0;
      } else if (SPLIT) {
        const int part = t / nt1;
        kt = t - part * nt1;
        part_offs(part, aoff, boff);
      }
      k0 = (kt + kt_base) * BKB;
    }
    if (CONV) {
      const int tap = k0 / d.Cin, ci0 = k0 - tap * d.Cin;
      const int kh = tap / d.KW, kw = tap - kh * d.KW;
#pragma unroll
      for (int j = 0; j < GA; ++j) {
        const T* src;
        if constexpr (MXC) {
          const int ih = (int)(a_hw[j] >> 16) - d.pad + kh, iw = (int)(a_hw[j] & 0xffffu) - d.pad + kw;
          src = ((unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W)
                    ? A + aoff + (a_pix[j] + (uint32_t)((ih * d.W + iw) * d.Cin + ci0))
                    : reinterpret_cast<const T*>(g_zero_page);
        } else {
          const int ih = a_ih0[j] + kh, iw = a_iw0[j] + kw;
          src = ((unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W)
                    ? asrc[j] + aoff + ((int64_t)ih * d.W + iw) * d.Cin + ci0
                    : reinterpret_cast<const T*>(g_zero_page);
        }
        __builtin_amdgcn_global_load_lds((glb_ptr)src, (lds_ptr)(st + grp_a(j) * BKB), 16, 0, 0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < GA; ++j)
        __builtin_amdgcn_global_load_lds((glb_ptr)(asrc[j] + aoff + k0), (lds_ptr)(st + grp_a(j) * BKB), 16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < GB; ++j) {
      const T* src = MXC ? B + boff + (b_off[j] + (uint32_t)k0) : bsrc[j] + boff + k0;
      __builtin_amdgcn_global_load_lds((glb_ptr)src, (lds_ptr)(st + BM2 * BKB + grp_b(j) * BKB), 16, 0, 0);
    }
  };

  f32x16 acc[M16 ? 1 : TM][M16 ? 1 : TN];
  f32x4 acc16[M16 ? TM * 2 : 1][M16 ? TN * 2 : 1];   // M16: 16x16 C^T tiles, lane (r = lane&15, q = lane>>4) owns row r, columns 4q..4q+3
  if constexpr (M16) {
#pragma unroll
    for (int i = 0; i < TM * 2; ++i)
#pragma unroll
      for (int j = 0; j < TN * 2; ++j) acc16[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
  }

  const int nt = nparts * nt1;
  const int fr = lane & 31, fh = lane >> 5;
  if constexpr (PH8) {
    // ---- 8-phase main loop (cdna_hip_programming.md "The 256^2 8-phase template", re-derived for 32x32x16 MFMAs — M16: 16
    // v_mfma_f32_16x16x32 per phase instead of 8 of 32x32x16, the production form since round 2: higher sustained clock — and
    // this kernel's C^T accumulators).  A K tile is consumed in four phases, one 64x32 quadrant of the wave's 128x64
    // tile each: (rows 0, cols 0) (rows 0, cols 1) (rows 1, cols 1) (rows 1, cols 0).  A phase is
    //     [LDS reads of the fragments this phase adds | 2 LDS-DMA instructions of the NEXT K tile | counted vmcnt]
    //     s_barrier  [8 MFMAs]  s_barrier
    // and the two wave rows run one barrier interval apart, so on every SIMD one wave issues MFMAs while the other
    // does its LDS reads and staging.  Staging order of tile t+1 during tile t: A half 0 (phase 0), B half 0 (1),
    // B half 1 (2), A half 1 (3); a half is read two or more phases after the vmcnt + barrier that retire it:
    //     phase 0 waits for B1 of tile t (<= 4 newer instructions outstanding), phase 1 for A1 of tile t,
    //     phase 3 for A0 and B0 of tile t+1; the buffer of tile t-1 is free from its phase 3 on (no LDS reads there).
    // Source of the K tile being staged (wave-uniform): advanced once per tile, no division in the loop.  Plain GEMM: k0 only;
    // SPLIT: the hi/lo part offsets; CONV: channel chunk -> tap -> (SPLIT) part, the same order as `issue` of the plain loop.
    int sk0 = kt_base * BKB, s_part = 0, s_kt = 0;           // dense: k offset, part, K tile inside the part
    int64_t s_aoff = 0, s_boff = 0;
    int s_tl = 0, s_c = 0;                                     // CONV: tap inside this K part, channel chunk
    const int kh0 = CONV ? tap_base / d.KW : 0, kw0 = CONV ? tap_base - kh0 * d.KW : 0;
    int s_kh = kh0, s_kw = kw0;
    if (CONV) sk0 = tap_base * d.Cin;
    auto advance_src = [&]() {
      if (CONV) {
        if (SPLIT && MXC) {
          ++s_part;
          s_aoff = s_part == 1 ? a_lo_off : 0;
          s_boff = s_part == 1 ? b_lo_off : 0;
          if (s_part < 2) return;
          s_part = 0;
        } else if (SPLIT) {
          ++s_part;
          s_aoff = s_part == 1 ? a_lo_off : 0;
          s_boff = s_part == 2 ? b_lo_off : 0;
          if (s_part < 3) return;
          s_part = 0;
          s_aoff = s_boff = 0;
        }
        if (++s_tl == ntap_part) {
          s_tl = 0; ++s_c; s_kh = kh0; s_kw = kw0;
        } else if (++s_kw == d.KW) {
          s_kw = 0; ++s_kh;
        }
        sk0 = (tap_base + s_tl) * d.Cin + s_c * BKB;
      } else if constexpr (MXC) {   // dense MX: the 16-bit tile and the correction tile of one k offset back to back
        ++s_part;
        s_aoff = s_part == 1 ? a_lo_off : 0;
        s_boff = s_part == 1 ? b_lo_off : 0;
        if (s_part < 2) return;
        s_part = 0;
        ++s_kt;
        sk0 = (s_kt + kt_base) * BKB;
      } else {
        if (++s_kt == nt1) {        // SPLIT only: next part, K restarts
          s_kt = 0; ++s_part;
          part_offs(s_part, s_aoff, s_boff);
        }
        sk0 = (s_kt + kt_base) * BKB;
      }
    };
    auto dma_a = [&](int t, int j) {
      const T* src;
      if constexpr (CONV && MXC) {
        const int ih = (int)(a_hw[j] >> 16) - d.pad + s_kh, iw = (int)(a_hw[j] & 0xffffu) - d.pad + s_kw;
        src = ((unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W)
                  ? A + s_aoff + (a_pix[j] + (uint32_t)((ih * d.W + iw) * d.Cin + s_c * BKB))
                  : reinterpret_cast<const T*>(g_zero_page);
      } else if (CONV) {
        const int ih = a_ih0[j] + s_kh, iw = a_iw0[j] + s_kw;
        src = ((unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W)
                  ? asrc[j] + s_aoff + ((int64_t)ih * d.W + iw) * d.Cin + s_c * BKB
                  : reinterpret_cast<const T*>(g_zero_page);
      } else {
        src = asrc[j] + s_aoff + sk0;
      }
      __builtin_amdgcn_global_load_lds((glb_ptr)src, (lds_ptr)(lds + (t & 1) * STAGE + grp_a(j) * BKB), 16, 0, 0);
    };
    auto dma_b = [&](int t, int j) {
      const T* src = MXC ? B + s_boff + (b_off[j] + (uint32_t)sk0) : bsrc[j] + s_boff + sk0;
      __builtin_amdgcn_global_load_lds((glb_ptr)src, (lds_ptr)(lds + (t & 1) * STAGE + BM2 * BKB + grp_b(j) * BKB), 16, 0, 0);
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dma_a(0, j);
      dma_b(0, j);
    }
    advance_src();   // the source now describes tile 1, staged during tile 0's phases
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wm == 1) __builtin_amdgcn_s_barrier();  // stagger the second wave row by one barrier interval
    // Fragment registers per phase (32 + 16 + 16 either way).  32x32x16 form: af[i][ks] = rows 32 i .. of the row half, K step
    // ks of four; b*f[ks] = the 32 columns of a column half.  16x16x32 form (M16): af[2 i + ii][ks] = rows 16 (2 i + ii) ..,
    // K step ks of two, flattened as af[(2 i + ii) >> 1][((2 i + ii) & 1) * 2 + ks]; b*f[jj * 2 + ks] = columns 16 jj ...
    // With 128-byte LDS rows the (row >> 1) & 7 swizzle is conflict-free for both fragment shapes.
    v8 af[2][4], b0f[4], b1f[4];
    const int r16 = lane & 15, q16 = lane >> 4;
    auto rd_a = [&](const T* As, int rh) {
      if constexpr (M16) {
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4) {
          const int row = (wm * TM + rh * 2) * 32 + t4 * 16 + r16;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            af[t4 >> 1][(t4 & 1) * 2 + ks] =
                __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(As + row * BKB + (((4 * ks + q16) ^ ((row >> 1) & 7)) << 3)));
        }
      } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = (wm * TM + rh * 2 + i) * 32 + fr;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
          af[i][ks] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(As + row * BKB + (((2 * ks + fh) ^ ((row >> 1) & 7)) << 3)));
      }
      }
    };
    auto rd_b = [&](const T* Bs, int ch, v8* bf) {
      if constexpr (M16) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          const int col = (wn * TN + ch) * 32 + jj * 16 + r16;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
            bf[jj * 2 + ks] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(Bs + col * BKB + (((4 * ks + q16) ^ ((col >> 1) & 7)) << 3)));
        }
      } else {
      const int col = (wn * TN + ch) * 32 + fr;
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
        bf[ks] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(Bs + col * BKB + (((2 * ks + fh) ^ ((col >> 1) & 7)) << 3)));
      }
    };
    auto mma = [&](int rh, int ch, const v8* bf) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_setprio(1);
      if constexpr (M16) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
              acc16[rh * 4 + t4][ch * 2 + jj] = T16<T>::mfma16(bf[jj * 2 + ks], af[t4 >> 1][(t4 & 1) * 2 + ks], acc16[rh * 4 + t4][ch * 2 + jj]);
      } else {
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[rh * 2 + i][ch] = T16<T>::mfma32(bf[ks], af[i][ks], acc[rh * 2 + i][ch]);
      }
      __builtin_amdgcn_s_setprio(0);
    };
    // MXC: the fragments live in 8-register vectors (the two ks halves of a lane = the 32-byte operand of the scaled fp8 MFMA;
    // the 16-bit MFMAs take the halves as sub-registers), so that no operand tuple is assembled by copies
    v8i_ af8[4], b0f8[2], b1f8[2];
    auto rd_a8 = [&](const T* As, int rh) {
#pragma unroll
      for (int t4 = 0; t4 < 4; ++t4) {
        const int row = (wm * TM + rh * 2) * 32 + t4 * 16 + r16;
        af8[t4] = cat8(*reinterpret_cast<const v4i_*>(As + row * BKB + (((q16) ^ ((row >> 1) & 7)) << 3)),
                       *reinterpret_cast<const v4i_*>(As + row * BKB + (((4 + q16) ^ ((row >> 1) & 7)) << 3)));
      }
    };
    auto rd_b8 = [&](const T* Bs, int ch, v8i_* bf8) {
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int col = (wn * TN + ch) * 32 + jj * 16 + r16;
        bf8[jj] = cat8(*reinterpret_cast<const v4i_*>(Bs + col * BKB + (((q16) ^ ((col >> 1) & 7)) << 3)),
                       *reinterpret_cast<const v4i_*>(Bs + col * BKB + (((4 + q16) ^ ((col >> 1) & 7)) << 3)));
      }
    };
    auto half8 = [](v8i_ x, int ks) -> v8 {
      return ks ? __builtin_bit_cast(v8, __builtin_shufflevector(x, x, 4, 5, 6, 7)) : __builtin_bit_cast(v8, __builtin_shufflevector(x, x, 0, 1, 2, 3));
    };
    auto mma8 = [&](int rh, int ch, const v8i_* bf8, auto mx_tag) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_setprio(1);
      if constexpr (decltype(mx_tag)::value) {   // 8 scaled fp8 MFMAs (K = 128 bytes each) in place of 16 16-bit ones
#pragma unroll
        for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) mfma_mx(acc16[rh * 4 + t4][ch * 2 + jj], bf8[jj], af8[t4], mx_sc, mx_one);
      } else {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int t4 = 0; t4 < 4; ++t4)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
              acc16[rh * 4 + t4][ch * 2 + jj] = T16<T>::mfma16(half8(bf8[jj], ks), half8(af8[t4], ks), acc16[rh * 4 + t4][ch * 2 + jj]);
      }
      __builtin_amdgcn_s_setprio(0);
    };
    auto RA = [&](const T* As, int rh) { if constexpr (MXC) rd_a8(As, rh); else rd_a(As, rh); };
    auto RB = [&](const T* Bs, int ch, int which) {
      if constexpr (MXC) rd_b8(Bs, ch, which ? b1f8 : b0f8); else rd_b(Bs, ch, which ? b1f : b0f);
    };
    // one K tile; MXC: even tiles are 16-bit tiles, odd tiles correction tiles — two bodies per loop trip instead of a
    // wave-uniform branch in every phase (with the branch the allocator spilled ~30 VGPRs into this loop)
    auto ktile = [&](int t, auto mx_tag) {
      auto MM = [&](int rh, int ch, int which) {
        if constexpr (MXC) mma8(rh, ch, which ? b1f8 : b0f8, mx_tag); else mma(rh, ch, which ? b1f : b0f);
      };
      const T* As = lds + (t & 1) * STAGE;
      const T* Bs = As + BM2 * BKB;
      const bool more = t + 1 < nt;
      // phase 0
      RA(As, 0);
      RB(Bs, 0, 0);
      if (more) { dma_a(t + 1, 0); dma_a(t + 1, 1); asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }
      else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      MM(0, 0, 0);
      __builtin_amdgcn_s_barrier();
      // phase 1
      RB(Bs, 1, 1);
      if (more) { dma_b(t + 1, 0); dma_b(t + 1, 1); asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      MM(0, 1, 1);
      __builtin_amdgcn_s_barrier();
      // phase 2
      RA(As, 1);
      if (more) { dma_b(t + 1, 2); dma_b(t + 1, 3); }
      __builtin_amdgcn_s_barrier();
      MM(1, 1, 1);
      __builtin_amdgcn_s_barrier();
      // phase 3
      if (more) { dma_a(t + 1, 2); dma_a(t + 1, 3); asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }
      advance_src();
      __builtin_amdgcn_s_barrier();
      MM(1, 0, 0);
      __builtin_amdgcn_s_barrier();
    };
    if constexpr (MXC) {
      for (int t = 0; t < nt; t += 2) {     // nt = 2 x (K tiles of one part): always even
        ktile(t, std::false_type{});
        ktile(t + 1, std::true_type{});
      }
    } else {
      for (int t = 0; t < nt; ++t) ktile(t, std::false_type{});
    }
    if (wm == 0) __builtin_amdgcn_s_barrier();  // balance the stagger
  } else {
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (s < nt) issue(s);

  for (int t = 0; t < nt; ++t) {
    // tile t has landed once at most (NS-2) newer tiles of this wave are still outstanding
    if (nt - t - 1 >= NS - 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NS - 2) * G) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (!(DBG & 1) && t + NS - 1 < nt) issue(t + NS - 1);
    const T* As = lds + (t % NS) * STAGE;
    const T* Bs = As + BM2 * BKB;
    if (MXC && (t & 1)) {
      if constexpr (MXC) {   // correction tile: both K halves of every fragment, one scaled fp8 MFMA per 16x16 output block
        const int r16 = lane & 15, q16 = lane >> 4;
        v8 af0[TM * 2], af1[TM * 2], bf0[TN * 2], bf1[TN * 2];
#pragma unroll
        for (int i = 0; i < TM * 2; ++i) {
          const int row = (wm * TM * 2 + i) * 16 + r16;
          af0[i] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(As + row * BKB + (((q16) ^ swz(row)) << 3)));
          af1[i] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(As + row * BKB + (((4 + q16) ^ swz(row)) << 3)));
        }
#pragma unroll
        for (int j = 0; j < TN * 2; ++j) {
          const int col = (wn * TN * 2 + j) * 16 + r16;
          bf0[j] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(Bs + col * BKB + (((q16) ^ swz(col)) << 3)));
          bf1[j] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(Bs + col * BKB + (((4 + q16) ^ swz(col)) << 3)));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < TM * 2; ++i)
#pragma unroll
          for (int j = 0; j < TN * 2; ++j)
            mfma_mx(acc16[i][j], cat8(bf0[j], bf1[j]), cat8(af0[i], af1[i]), mx_sc, mx_one);
      }
    } else if constexpr (M16) {
      // one K = 32 step per tile: 2TM A fragments + 2TN B fragments (one ds_read_b128 each), then (2TM)(2TN) MFMAs;
      // the first MFMAs need only the first fragments, so the compiler's counted lgkmcnt lets them start early
      const int r16 = lane & 15, q16 = lane >> 4;
#pragma unroll
      for (int ks = 0; ks < BKB / 32; ++ks) {
        v8 af[TM * 2], bf[TN * 2];
#pragma unroll
        for (int i = 0; i < TM * 2; ++i) {
          const int row = (wm * TM * 2 + i) * 16 + r16;
          af[i] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(As + row * BKB + (((4 * ks + q16) ^ swz(row)) << 3)));
        }
#pragma unroll
        for (int j = 0; j < TN * 2; ++j) {
          const int col = (wn * TN * 2 + j) * 16 + r16;
          bf[j] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(Bs + col * BKB + (((4 * ks + q16) ^ swz(col)) << 3)));
        }
#pragma unroll
        for (int i = 0; i < TM * 2; ++i)
#pragma unroll
          for (int j = 0; j < TN * 2; ++j) acc16[i][j] = T16<T>::mfma16(bf[j], af[i], acc16[i][j]);  // D[n][m]: lane = output row
      }
    } else if (!(DBG & 2)) {
      // fragments of k-step ks+1 are fetched from LDS while the MFMAs of k-step ks run (register double buffer)
      v8 af[2][TM], bf[2][TN];
      auto fetch = [&](int ks, int slot) {
        const int chunk = 2 * ks + fh;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const int row = (wm * TM + i) * 32 + fr;
          af[slot][i] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(As + row * BKB + ((chunk ^ ((row >> SWS) & (CPR - 1))) << 3)));
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const int col = (wn * TN + j) * 32 + fr;
          bf[slot][j] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(Bs + col * BKB + ((chunk ^ ((col >> SWS) & (CPR - 1))) << 3)));
        }
      };
      constexpr int KS = BKB / 16;
      fetch(0, 0);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        if (ks < KS - 1) fetch(ks + 1, (ks + 1) & 1);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j)
            acc[i][j] = T16<T>::mfma32(bf[ks & 1][j], af[ks & 1][i], acc[i][j]);  // D[n][m]: lane = output row
      }
    }
  }
  }  // !PH8

  // ---- epilogue (same semantics as gemm_kernel) ----
  if (DBG & 4) {  // lab only: keep the accumulators live, store one value per lane
    if (blockIdx.x == gridDim.x / 2 && tid == 0) {  // shader clock under load: s_memtime ticks per 100 MHz s_memrealtime tick
      uint64_t c1, r1;
      asm volatile("s_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(c1), "=s"(r1)::"memory");
      uint64_t* o = reinterpret_cast<uint64_t*>(d.C);
      o[0] = c1 - dbg_c0;
      o[1] = r1 - dbg_r0;
    }
    float z = 0.f;
    if constexpr (M16) {
#pragma unroll
      for (int i = 0; i < TM * 2; ++i)
#pragma unroll
        for (int j = 0; j < TN * 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) z += acc16[i][j][r];
    } else {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) z += acc[i][j][r];
    }
    if (z == 123.456f) reinterpret_cast<float*>(d.C)[tid] = z;
    return;
  }
  // Accumulators are C^T tiles (mfma(B, A)): lane (fr, fh) owns output row m = ..+fr and, per register
  // group g, the 4 consecutive columns n = 8g + 4fh + (0..3): vector loads of bias / LayerScale / residual
  // and 8- or 16-byte stores instead of 2-byte ones (the 2-byte form cost as much as the whole K loop).
  const int64_t cbase = (int64_t)bz * d.strideC;
  const float* __restrict__ res = d.res ? d.res + (int64_t)bz * d.strideR : nullptr;
  const bool vec = gemm_big_vec_epilogue(d, cbase, res);
  if constexpr (M16 && PH8) {
    // 16-bit outputs without residual / statistics (q|k, fc1 + GELU): bias and activation are applied in the accumulator
    // layout (a lane owns 4 consecutive columns of one row), the result is converted to 16 bits BEFORE the LDS transposition
    // (half the slab bytes: 8-byte writes, 16-byte reads) and leaves as 16-byte stores, 8 rows x 128 bytes per instruction —
    // half as many, twice as wide as the fp32 slab path's.  This form's epilogue is fully exposed (one workgroup per CU).
    if (vec && !d.out_f32 && !res && !d.res16 && !d.C_lo && !d.rowstats && !d.stats && !d.scale_n && d.act != ASIS_ACT_GELU_GRAD && !(DBG & 8) &&
        (d.N & 7) == 0 && (d.ldc & 7) == 0 && (cbase & 7) == 0 && !(GROUP_M_FLAGS >> 16)) {
      constexpr int SW16 = TN * 32 + 8;                 // slab row in 16-bit elements (144 bytes: conflict-free 8-byte writes)
      __syncthreads();                                  // every wave is done with the staging buffers
      T* slab16 = reinterpret_cast<T*>(lds) + wid * (32 * SW16);
      const int r16 = lane & 15, q16 = lane >> 4;
      const int rr8 = lane >> 3, c8 = lane & 7;
      // LayerNorm folded into the weight (asis_gemm_desc.ln_mr / ln_cs; dense launches only): v = rstd * (acc - mean * cs) +
      // bias, statistics per output ROW (ln_cols == 0: A rows are the tokens) or per output COLUMN (ln_cols != 0: the swapped
      // V^T GEMM, B rows are the tokens of batch entry bz; cs is then per output row).  Without it the arithmetic below is
      // the plain acc + bias (no LN operand is touched).
      const bool ln_on = LNF != 0 && !CONV && d.ln_mr != nullptr, ln_c = ln_on && d.ln_cols != 0;   // LNF: the instance that implements the fields
      const float2* const mrp = reinterpret_cast<const float2*>(d.ln_mr) + (ln_c ? (int64_t)bz * (d.strideB / d.ldb) : 0);
      float4 bj[TN * 2], cj[TN * 2];
      float2 mc[TN * 2][4];   // ln_c: (mean, rstd) of this lane's four columns per 16-column block
#pragma unroll
      for (int j = 0; j < TN * 2; ++j) {
        const int colj = n0 + (wn * TN * 2 + j) * 16 + 4 * q16;
        bj[j] = (d.bias_n && kt_base == 0 && colj < d.N) ? *reinterpret_cast<const float4*>(d.bias_n + colj) : make_float4(0.f, 0.f, 0.f, 0.f);
        cj[j] = (ln_on && !ln_c && colj < d.N) ? *reinterpret_cast<const float4*>(d.ln_cs + colj) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          mc[j][e] = make_float2(0.f, 1.f);
          if (ln_c) mc[j][e] = mrp[colj + e < d.N ? colj + e : d.N - 1];
        }
      }
      // ASIS_ACT_SILU_MUL (SwiGLU in the epilogue; dense launches, routed here by the dispatcher only): B rows come interleaved in
      // groups of 16 ([x1 rows 16g .. 16g+15 | x2 rows 16g .. 16g+15]), so a lane's 16-column blocks 2t / 2t+1 hold x1 / x2 of the
      // SAME four hidden columns: h = silu(x1 + b1) * (x2 + b2) in the accumulator layout, half as many 16-bit columns out
      // ([M, N / 2], row stride ldc) — the fp32 pre-activation [M, N] never reaches HBM.
      const bool sg = d.act == ASIS_ACT_SILU_MUL;
      const int colr = sg ? (n0 >> 1) + wn * TN * 16 + (lane & 3) * 8 : n0 + wn * TN * 32 + c8 * 8;
      const bool cokr = colr < (sg ? (d.N >> 1) : d.N);
      T* const Cw = reinterpret_cast<T*>(d.C) + cbase + colr;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii) {
          float bm1 = 0.f, nmean = -0.f, rstd = 1.f, csr = 0.f;
          const int rowb = m0 + (wm * TM + i) * 32 + ii * 16 + r16;
          const int rowbc = rowb < d.M ? rowb : d.M - 1;
          if (d.bias_m) bm1 = d.bias_m[rowbc];   // per-row bias (the V^T GEMM: rows are the output features)
          if (ln_on && !ln_c) {
            const float2 mr = mrp[rowbc];
            nmean = -mr.x;
            rstd = mr.y;
          }
          if (ln_c) csr = d.ln_cs[rowbc];
          float4 vg = make_float4(0.f, 0.f, 0.f, 0.f);   // SwiGLU: the gate half (x1) of the current block pair
#pragma unroll
          for (int j = 0; j < TN * 2; ++j) {
            float4 v;
            if (ln_c) {
              v = make_float4(__builtin_fmaf(__builtin_fmaf(-mc[j][0].x, csr, acc16[2 * i + ii][j][0]), mc[j][0].y, bj[j].x + bm1),
                              __builtin_fmaf(__builtin_fmaf(-mc[j][1].x, csr, acc16[2 * i + ii][j][1]), mc[j][1].y, bj[j].y + bm1),
                              __builtin_fmaf(__builtin_fmaf(-mc[j][2].x, csr, acc16[2 * i + ii][j][2]), mc[j][2].y, bj[j].z + bm1),
                              __builtin_fmaf(__builtin_fmaf(-mc[j][3].x, csr, acc16[2 * i + ii][j][3]), mc[j][3].y, bj[j].w + bm1));
            } else if (ln_on) {
              v = make_float4(__builtin_fmaf(__builtin_fmaf(nmean, cj[j].x, acc16[2 * i + ii][j][0]), rstd, bj[j].x + bm1),
                              __builtin_fmaf(__builtin_fmaf(nmean, cj[j].y, acc16[2 * i + ii][j][1]), rstd, bj[j].y + bm1),
                              __builtin_fmaf(__builtin_fmaf(nmean, cj[j].z, acc16[2 * i + ii][j][2]), rstd, bj[j].z + bm1),
                              __builtin_fmaf(__builtin_fmaf(nmean, cj[j].w, acc16[2 * i + ii][j][3]), rstd, bj[j].w + bm1));
            } else {
              v = make_float4(acc16[2 * i + ii][j][0] + bj[j].x + bm1, acc16[2 * i + ii][j][1] + bj[j].y + bm1,
                              acc16[2 * i + ii][j][2] + bj[j].z + bm1, acc16[2 * i + ii][j][3] + bj[j].w + bm1);
            }
            if (sg) {
              if (j & 1) {
                uint2 pk;
                pk.x = pack2<T>(silu_mul(vg.x, v.x), silu_mul(vg.y, v.y));
                pk.y = pack2<T>(silu_mul(vg.z, v.z), silu_mul(vg.w, v.w));
                *reinterpret_cast<uint2*>(slab16 + (ii * 16 + r16) * SW16 + 16 * (j >> 1) + 4 * q16) = pk;
              } else {
                vg = v;
              }
              continue;
            }
            if (d.act == ASIS_ACT_GELU) gelu_erf4(v.x, v.y, v.z, v.w);
            else if (d.act == ASIS_ACT_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            uint2 pk;
            pk.x = pack2<T>(v.x, v.y);
            pk.y = pack2<T>(v.z, v.w);
            *reinterpret_cast<uint2*>(slab16 + (ii * 16 + r16) * SW16 + 16 * j + 4 * q16) = pk;
          }
        }
        if (sg) {   // 32 rows x (TN * 16) hidden columns: 4 lanes x 16 bytes per row, 16 rows per instruction
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const int lrow = p * 16 + (lane >> 2);
            const int row = m0 + (wm * TM + i) * 32 + lrow;
            const uint4 w = *reinterpret_cast<const uint4*>(slab16 + lrow * SW16 + (lane & 3) * 8);
            if (row < d.M && cokr) *reinterpret_cast<uint4*>(Cw + (int64_t)row * d.ldc) = w;
          }
          continue;
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int lrow = p * 8 + rr8;
          const int row = m0 + (wm * TM + i) * 32 + lrow;
          const uint4 w = *reinterpret_cast<const uint4*>(slab16 + lrow * SW16 + c8 * 8);
          if (row < d.M && cokr) *reinterpret_cast<uint4*>(Cw + (int64_t)row * d.ldc) = w;
        }
      }
      return;
    }
  }
  if constexpr (LNF != 0 && M16 && PH8 && !CONV && !SPLIT) {
    if (d.C_lo || d.rowstats || d.res16) {
      // LayerNorm-fold PRODUCER epilogue (proj, fc2; include/asis_hip.h): v = res + scale * (acc + bias) with the residual as
      // fp32 or as two 16-bit planes, the result as fp32 or as two planes (+ per-row partial sums of v for the next LayerNorm).
      // A lane owns EIGHT consecutive columns of a row here (8 lanes per row, 8 rows per pass), so that a plane access is one
      // 16-byte instruction exactly like an fp32 access of four columns: the planes cost no more load / store instructions than
      // the fp32 tensors they replace (the generic path below, four columns per lane, needed twice as many 8-byte ones).
      // Host contract (asis_gemm): N % 8 == 0, ldc / ldr / ldr16 multiples of 8 elements, 16-byte aligned pointers, batch 1.
      constexpr int SW = TN * 32 + 4;
      __syncthreads();
      float* slab = reinterpret_cast<float*>(lds) + wid * (32 * SW);
      const int rr = lane >> 3, c8 = lane & 7;
      const int col = n0 + wn * TN * 32 + c8 * 8;
      const bool cok = col < d.N;
      const int colc = cok ? col : 0;
      float4 ba = make_float4(0.f, 0.f, 0.f, 0.f), bb = ba, sa = make_float4(1.f, 1.f, 1.f, 1.f), sb = sa;
      if (cok && d.bias_n) { ba = *reinterpret_cast<const float4*>(d.bias_n + col); bb = *reinterpret_cast<const float4*>(d.bias_n + col + 4); }
      if (cok && d.scale_n) { sa = *reinterpret_cast<const float4*>(d.scale_n + col); sb = *reinterpret_cast<const float4*>(d.scale_n + col + 4); }
      const bool res_planes = d.res16 != nullptr;
      const float* const zp = reinterpret_cast<const float*>(g_zero_page);
      const float* const resp = d.res ? d.res + colc : zp;
      const int64_t ldr_e = d.res ? d.ldr : 0;
      const T* const r16h = reinterpret_cast<const T*>(d.res16) + colc;
      const T* const r16l = reinterpret_cast<const T*>(d.res16_lo) + colc;
      T* const Clo = reinterpret_cast<T*>(d.C_lo);
      float* const rstats = d.rowstats;
      const int sgroups = (d.N + 63) >> 6, sgrp = (n0 + wn * TN * 32) >> 6;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int j = 0; j < TN * 2; ++j)
            *reinterpret_cast<float4*>(slab + (ii * 16 + (lane & 15)) * SW + 16 * j + 4 * (lane >> 4)) =
                make_float4(acc16[2 * i + ii][j][0], acc16[2 * i + ii][j][1], acc16[2 * i + ii][j][2], acc16[2 * i + ii][j][3]);
        uint4 ra[4], rb[4];   // residual of the four passes: fp32 (two 16-byte pieces) or (hi | lo) planes (16 bytes each)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int row = m0 + (wm * TM + i) * 32 + q * 8 + rr;
          const int rowc = row < d.M ? row : d.M - 1;
          if (res_planes) {
            ra[q] = *reinterpret_cast<const uint4*>(r16h + (int64_t)rowc * d.ldr16);
            rb[q] = *reinterpret_cast<const uint4*>(r16l + (int64_t)rowc * d.ldr16);
          } else {
            ra[q] = *reinterpret_cast<const uint4*>(resp + (int64_t)rowc * ldr_e);
            rb[q] = *reinterpret_cast<const uint4*>(resp + (int64_t)rowc * ldr_e + (d.res ? 4 : 0));
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int lrow = q * 8 + rr;
          const int row = m0 + (wm * TM + i) * 32 + lrow;
          float4 va = *reinterpret_cast<const float4*>(slab + lrow * SW + c8 * 8);
          float4 vb = *reinterpret_cast<const float4*>(slab + lrow * SW + c8 * 8 + 4);
          float4 xa, xb;
          if (res_planes) {   // hi + lo is exact in fp32 (two non-overlapping 11-bit pieces)
            float h[8], l[8];
            unpack2<T>(ra[q].x, h[0], h[1]); unpack2<T>(ra[q].y, h[2], h[3]); unpack2<T>(ra[q].z, h[4], h[5]); unpack2<T>(ra[q].w, h[6], h[7]);
            unpack2<T>(rb[q].x, l[0], l[1]); unpack2<T>(rb[q].y, l[2], l[3]); unpack2<T>(rb[q].z, l[4], l[5]); unpack2<T>(rb[q].w, l[6], l[7]);
            xa = make_float4(h[0] + l[0], h[1] + l[1], h[2] + l[2], h[3] + l[3]);
            xb = make_float4(h[4] + l[4], h[5] + l[5], h[6] + l[6], h[7] + l[7]);
          } else {
            xa = __builtin_bit_cast(float4, ra[q]);
            xb = __builtin_bit_cast(float4, rb[q]);
          }
          float st_s = 0.f, st_q = 0.f;
          if (row < d.M && cok) {
            va.x = (va.x + ba.x) * sa.x + xa.x; va.y = (va.y + ba.y) * sa.y + xa.y; va.z = (va.z + ba.z) * sa.z + xa.z; va.w = (va.w + ba.w) * sa.w + xa.w;
            vb.x = (vb.x + bb.x) * sb.x + xb.x; vb.y = (vb.y + bb.y) * sb.y + xb.y; vb.z = (vb.z + bb.z) * sb.z + xb.z; vb.w = (vb.w + bb.w) * sb.w + xb.w;
            if (d.out_f32) {
              float* const cp = reinterpret_cast<float*>(d.C) + (int64_t)row * d.ldc + col;
              *reinterpret_cast<float4*>(cp) = va;
              *reinterpret_cast<float4*>(cp + 4) = vb;
            } else {
              uint4 ph;
              ph.x = pack2<T>(va.x, va.y); ph.y = pack2<T>(va.z, va.w); ph.z = pack2<T>(vb.x, vb.y); ph.w = pack2<T>(vb.z, vb.w);
              *reinterpret_cast<uint4*>(reinterpret_cast<T*>(d.C) + (int64_t)row * d.ldc + col) = ph;
              if (Clo) {
                uint4 pl;
                pl.x = pack2<T>(lo_part<T>(va.x), lo_part<T>(va.y)); pl.y = pack2<T>(lo_part<T>(va.z), lo_part<T>(va.w));
                pl.z = pack2<T>(lo_part<T>(vb.x), lo_part<T>(vb.y)); pl.w = pack2<T>(lo_part<T>(vb.z), lo_part<T>(vb.w));
                *reinterpret_cast<uint4*>(Clo + (int64_t)row * d.ldc + col) = pl;
              }
            }
            st_s = ((va.x + va.y) + (va.z + va.w)) + ((vb.x + vb.y) + (vb.z + vb.w));
            st_q = ((va.x * va.x + va.y * va.y) + (va.z * va.z + va.w * va.w)) + ((vb.x * vb.x + vb.y * vb.y) + (vb.z * vb.z + vb.w * vb.w));
          }
          if (rstats) {   // wave-uniform; the 8 lanes of half a DPP row hold the 64 columns of one output row
            st_s = row8_sum(st_s);
            st_q = row8_sum(st_q);
            // sgrp < sgroups: a 256-column tile that overhangs N (N % 256 != 0) holds wave column groups past the last 64-column group
            if (c8 == 0 && row < d.M && sgrp < sgroups) *reinterpret_cast<float2*>(rstats + ((int64_t)row * sgroups + sgrp) * 2) = make_float2(st_s, st_q);
          }
        }
      }
      return;
    }
  }
  if (vec) {
    // Transpose each 32 x (TN*32) slab of the wave tile through a private LDS slab so that global
    // accesses are full lines: TN*8 consecutive lanes cover one row (16 B = 4 columns per lane).
    constexpr int SW = TN * 32 + 4;                    // padded slab row (floats): conflict-free b128 writes
    constexpr int LPR = TN * 8;                        // lanes per row when reading back
    constexpr int RPP = 64 / LPR;                      // rows per pass
    __syncthreads();                                   // every wave is done with the staging buffers
    float* slab = reinterpret_cast<float*>(lds) + wid * (32 * SW);
    const int rr = lane / LPR, ch = lane - rr * LPR;
    const int col = n0 + wn * TN * 32 + ch * 4;
    const bool cok = col < d.N;
    float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f), s4 = make_float4(1.f, 1.f, 1.f, 1.f);
    if (cok && d.bias_n && kt_base == 0) b4 = *reinterpret_cast<const float4*>(d.bias_n + col);  // K parts: part 0 only
    if (cok && d.scale_n) s4 = *reinterpret_cast<const float4*>(d.scale_n + col);
    float4 st_s = make_float4(0.f, 0.f, 0.f, 0.f), st_q = st_s;  // BatchNorm partial sums of this lane's columns
    // Residual / per-row bias / GELU'(pre-activation) operands of a whole 32-row slab are fetched up front, from
    // addresses clamped into the tensors (a zero page stands in for an absent operand), so their latency runs under
    // the LDS transpose instead of once per pass: a load inside `if (row < M && ...)` is waited for on the spot.
    constexpr int NP = 32 / RPP;
    const float* const zp = reinterpret_cast<const float*>(g_zero_page);
    const bool has_aux = d.act == ASIS_ACT_GELU_GRAD;
    const int colc = cok ? col : 0;
    const float* const resp = (res && !(DBG & 32)) ? res + colc : zp;  // DBG & 32 (lab): no residual fetch
    const int64_t ldr_e = (res && !(DBG & 32)) ? d.ldr : 0;
    const float* const bmp = d.bias_m ? d.bias_m : zp;
    const int bm_e = d.bias_m ? 1 : 0;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      if constexpr (M16) {
#pragma unroll
        for (int ii = 0; ii < 2; ++ii)
#pragma unroll
          for (int j = 0; j < TN * 2; ++j)
            *reinterpret_cast<float4*>(slab + (ii * 16 + (lane & 15)) * SW + 16 * j + 4 * (lane >> 4)) =
                make_float4(acc16[2 * i + ii][j][0], acc16[2 * i + ii][j][1], acc16[2 * i + ii][j][2], acc16[2 * i + ii][j][3]);
      } else {
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<float4*>(slab + fr * SW + 32 * j + 8 * g + 4 * fh) =
              make_float4(acc[i][j][4 * g + 0], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
      }
      // issued after the slab writes (the accumulator registers of this slab are free again), PG passes at a time:
      // a whole slab's worth spills in the 128-register form of the kernel
      constexpr int PG = (OCC >= 4 && NP > 4) ? 4 : NP;
#pragma unroll
      for (int p0 = 0; p0 < NP; p0 += PG) {
        float4 r4[PG];
        float bmv[PG];
        uint2 pw[PG];
#pragma unroll
        for (int q = 0; q < PG; ++q) {
          const int row = m0 + (wm * TM + i) * 32 + (p0 + q) * RPP + rr;
          const int rowc = row < d.M ? row : d.M - 1;
          r4[q] = *reinterpret_cast<const float4*>(resp + (int64_t)rowc * ldr_e);
          bmv[q] = bmp[rowc * bm_e];
          pw[q] = make_uint2(0u, 0u);
        }
        if (has_aux) {
#pragma unroll
          for (int q = 0; q < PG; ++q) {
            const int row = m0 + (wm * TM + i) * 32 + (p0 + q) * RPP + rr;
            const int rowc = row < d.M ? row : d.M - 1;
            pw[q] = *reinterpret_cast<const uint2*>(reinterpret_cast<const T*>(d.aux) + (int64_t)rowc * d.ld_aux + colc);
          }
        }
#pragma unroll
        for (int q = 0; q < PG; ++q) {
          const int lrow = (p0 + q) * RPP + rr;
          const int row = m0 + (wm * TM + i) * 32 + lrow;
          float4 v = *reinterpret_cast<const float4*>(slab + lrow * SW + ch * 4);
          if (row < d.M && cok) {
            const float bm1 = bmv[q];
            v.x += b4.x + bm1; v.y += b4.y + bm1; v.z += b4.z + bm1; v.w += b4.w + bm1;
            if (d.act == ASIS_ACT_GELU) gelu_erf4(v.x, v.y, v.z, v.w);
            else if (has_aux) {  // input-gradient GEMM of fc2 fused with GELU's backward
              float g0, g1, g2, g3;
              unpack2<T>(pw[q].x, g0, g1);
              unpack2<T>(pw[q].y, g2, g3);
              v.x *= gelu_erf_grad_fast(g0); v.y *= gelu_erf_grad_fast(g1); v.z *= gelu_erf_grad_fast(g2); v.w *= gelu_erf_grad_fast(g3);
            }
            else if (d.act == ASIS_ACT_RELU) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
            v.x *= s4.x; v.y *= s4.y; v.z *= s4.z; v.w *= s4.w;
            v.x += r4[q].x; v.y += r4[q].y; v.z += r4[q].z; v.w += r4[q].w;
            if ((DBG & 8) && v.x != 123.456f) {  // lab: everything but the global stores
            } else if (d.out_f32) {
              *reinterpret_cast<float4*>(reinterpret_cast<float*>(d.C) + cbase + (int64_t)row * d.ldc + col) = v;
            } else {
              uint2 pk;
              pk.x = pack2<T>(v.x, v.y);
              pk.y = pack2<T>(v.z, v.w);
              *reinterpret_cast<uint2*>(reinterpret_cast<T*>(d.C) + cbase + (int64_t)row * d.ldc + col) = pk;
            }
            st_s.x += v.x; st_s.y += v.y; st_s.z += v.z; st_s.w += v.w;
            st_q.x += v.x * v.x; st_q.y += v.y * v.y; st_q.z += v.z * v.z; st_q.w += v.w * v.w;
          }
        }
      }
    }
    if (d.stats) {
      // lanes ch + LPR*rr hold the same columns: fold rr with xor-shuffles, then the WM row blocks through LDS.
      // stats rows are per 128 rows (asis_gemm_tiles_m): a tile writes its first row and zeroes the others it covers.
      for (int o = LPR; o < 64; o <<= 1) {
        st_s.x += __shfl_xor(st_s.x, o, 64); st_s.y += __shfl_xor(st_s.y, o, 64);
        st_s.z += __shfl_xor(st_s.z, o, 64); st_s.w += __shfl_xor(st_s.w, o, 64);
        st_q.x += __shfl_xor(st_q.x, o, 64); st_q.y += __shfl_xor(st_q.y, o, 64);
        st_q.z += __shfl_xor(st_q.z, o, 64); st_q.w += __shfl_xor(st_q.w, o, 64);
      }
      __syncthreads();  // slabs are dead; reuse the head of LDS: red[wm][2][BN2]
      float* red = reinterpret_cast<float*>(lds);
      if (rr == 0) {
        *reinterpret_cast<float4*>(red + (wm * 2 + 0) * BN2 + wn * TN * 32 + ch * 4) = st_s;
        *reinterpret_cast<float4*>(red + (wm * 2 + 1) * BN2 + wn * TN * 32 + ch * 4) = st_q;
      }
      __syncthreads();
      if (tid < BN2 && n0 + tid < d.N) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int w2 = 0; w2 < WM; ++w2) {
          s += red[(w2 * 2 + 0) * BN2 + tid];
          q += red[(w2 * 2 + 1) * BN2 + tid];
        }
        const int c = n0 + tid;
        constexpr int RB = BM2 / 128;  // stats rows (of 128 output rows each) this tile covers: the first takes the sums
        const int64_t r0 = (int64_t)tile_m * RB;
        d.stats[(r0 * 2 + 0) * d.N + c] = s;
        d.stats[(r0 * 2 + 1) * d.N + c] = q;
#pragma unroll
        for (int e = 1; e < RB; ++e)
          if ((r0 + e) * 128 < d.M) {
            d.stats[((r0 + e) * 2 + 0) * d.N + c] = 0.f;
            d.stats[((r0 + e) * 2 + 1) * d.N + c] = 0.f;
          }
      }
    }
    return;
  }
  // scalar fallback (N or a leading dimension not a multiple of 4)
  auto scalar_out = [&](int row, int c, float a, float bmv) {
    float x = a + (d.bias_n ? d.bias_n[c] : 0.f) + bmv;
    if (d.act == ASIS_ACT_GELU) x = gelu_erf(x);
    else if (d.act == ASIS_ACT_RELU) x = fmaxf(x, 0.f);
    if (d.scale_n) x *= d.scale_n[c];
    if (res) x += res[(int64_t)row * d.ldr + c];
    if (d.out_f32) reinterpret_cast<float*>(d.C)[cbase + (int64_t)row * d.ldc + c] = x;
    else reinterpret_cast<T*>(d.C)[cbase + (int64_t)row * d.ldc + c] = to_t16<T>(x);
  };
  if constexpr (M16) {
#pragma unroll
    for (int i = 0; i < TM * 2; ++i) {
      const int row = m0 + (wm * TM * 2 + i) * 16 + (lane & 15);
      if (row >= d.M) continue;
      const float bmv = d.bias_m ? d.bias_m[row] : 0.f;
#pragma unroll
      for (int j = 0; j < TN * 2; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = n0 + (wn * TN * 2 + j) * 16 + 4 * (lane >> 4) + e;
          if (c < d.N) scalar_out(row, c, acc16[i][j][e], bmv);
        }
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = m0 + (wm * TM + i) * 32 + fr;
    const bool rok = row < d.M;
    const float bmv = (d.bias_m && rok) ? d.bias_m[row] : 0.f;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int col = n0 + (wn * TN + j) * 32 + 8 * g + 4 * fh;
        if (!rok || col >= d.N) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = col + e;
          if (c < d.N) {
            float x = acc[i][j][4 * g + e] + (d.bias_n ? d.bias_n[c] : 0.f) + bmv;
            if (d.act == ASIS_ACT_GELU) x = gelu_erf(x);
            else if (d.act == ASIS_ACT_RELU) x = fmaxf(x, 0.f);
            if (d.scale_n) x *= d.scale_n[c];
            if (res) x += res[(int64_t)row * d.ldr + c];
            if (d.out_f32) reinterpret_cast<float*>(d.C)[cbase + (int64_t)row * d.ldc + c] = x;
            else reinterpret_cast<T*>(d.C)[cbase + (int64_t)row * d.ldc + c] = to_t16<T>(x);
          }
        }
      }
    }
  }
}


}  // namespace
