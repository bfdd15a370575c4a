// MFMA GEMM / implicit-GEMM convolution for gfx950.
//
//   C[M,N] = epilogue( A[M,K] * B[N,K]^T )      16-bit operands, fp32 accumulate
//
// Tiling (wave64, v_mfma_f32_32x32x16_{f16,bf16}):
//   workgroup 256 threads = 4 waves (2x2), tile 128x128x64, each wave a 64x64 sub-tile
//   = 2x2 MFMA 32x32 accumulators (64 acc VGPRs).  A and B tiles are staged
//   global -> VGPR -> LDS (register staging lets the A loader be an arbitrary per-lane
//   gather with zero fill: that is what turns the same kernel into a 3x3 implicit-GEMM
//   convolution on NHWC activations).  Two LDS buffers (64 KiB) -> 2 workgroups / CU;
//   the global loads of tile t+1 are issued before the MFMAs of tile t and written to the
//   other buffer after them (one barrier per K tile).
//   LDS image: [row][64 k] (128-B rows); the 16-B chunk index is XOR-swizzled with
//   (row>>1)&7, which makes the ds_read_b128 fragment reads (16-lane groups
//   {0-3,12-15,20-27}...) conflict-free (MI355X_MICROARCH.md §LDS).
//   Block ids are remapped XCD-aware so the N tiles of one M tile share an L2.
//
// Reference sites replaced: see include/asis_hip.h (asis_gemm).
#include <stdlib.h>

#include "asis_common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64, NTHREADS = 256;

template <typename T, bool CONV>
__global__ __launch_bounds__(NTHREADS, 2) void gemm_kernel(const asis_gemm_desc d) {
  typedef typename T16<T>::v8 v8;
  __shared__ __attribute__((aligned(16))) T lds[2 * (BM + BN) * BK];  // 64 KiB

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;

  const int tiles_n = (d.N + BN - 1) / BN;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int tile_m = bid / tiles_n;
  const int tile_n = bid - tile_m * tiles_n;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int bz = blockIdx.y;

  const T* __restrict__ A = reinterpret_cast<const T*>(d.A) + (int64_t)bz * d.strideA;
  const T* __restrict__ B = reinterpret_cast<const T*>(d.B) + (int64_t)bz * d.strideB;

  // ---- loader geometry: thread -> (row lrow + 32*i, 16-byte chunk lchk) -----------------
  const int lrow = tid >> 3;
  const int lchk = tid & 7;
  int64_t a_off[4];  // dense: element offset of row start; conv: pixel index base of image b
  int a_ih0[4], a_iw0[4];
  bool a_ok[4], b_ok[4];
  int64_t b_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + lrow + 32 * i;
    a_ok[i] = m < d.M;
    if (CONV) {
      const int mm = a_ok[i] ? m : 0;
      const int ohw = d.OH * d.OW;
      const int b = mm / ohw;
      const int rem = mm - b * ohw;
      const int oh = rem / d.OW;
      const int ow = rem - oh * d.OW;
      a_ih0[i] = oh * d.stride - d.pad;
      a_iw0[i] = ow * d.stride - d.pad;
      a_off[i] = (int64_t)b * d.H * d.W;
    } else {
      a_off[i] = (int64_t)m * d.lda;
      a_ih0[i] = a_iw0[i] = 0;
    }
    const int n = n0 + lrow + 32 * i;
    b_ok[i] = n < d.N;
    b_off[i] = (int64_t)n * d.ldb;
  }

  uint4 ra[4], rb[4];
  auto load_tile = [&](int k0) {
    const int kk = k0 + lchk * 8;
    const bool kok = kk < d.K;
    int kh = 0, kw = 0, ci = kk;
    if (CONV) {
      const int tap = kk / d.Cin;
      ci = kk - tap * d.Cin;
      kh = tap / d.KW;
      kw = tap - kh * d.KW;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (CONV) {
        const int ih = a_ih0[i] + kh, iw = a_iw0[i] + kw;
        if (a_ok[i] && kok && (unsigned)ih < (unsigned)d.H && (unsigned)iw < (unsigned)d.W)
          v = *reinterpret_cast<const uint4*>(A + (a_off[i] + (int64_t)ih * d.W + iw) * d.Cin + ci);
      } else {
        if (a_ok[i] && kok) v = *reinterpret_cast<const uint4*>(A + a_off[i] + kk);
      }
      ra[i] = v;
      uint4 w = make_uint4(0, 0, 0, 0);
      if (b_ok[i] && kok) w = *reinterpret_cast<const uint4*>(B + b_off[i] + kk);
      rb[i] = w;
    }
  };
  auto store_tile = [&](int buf) {
    T* As = lds + buf * ((BM + BN) * BK);
    T* Bs = As + BM * BK;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = lrow + 32 * i;
      const int sw = (lchk ^ ((row >> 1) & 7)) << 3;
      *reinterpret_cast<uint4*>(As + row * BK + sw) = ra[i];
      *reinterpret_cast<uint4*>(Bs + row * BK + sw) = rb[i];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nt = (d.K + BK - 1) / BK;
  load_tile(0);
  store_tile(0);
  __syncthreads();

  const int fr = lane & 31, fh = lane >> 5;
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) load_tile((t + 1) * BK);
    const T* As = lds + buf * ((BM + BN) * BK);
    const T* Bs = As + BM * BK;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      v8 af[2], bf[2];
      const int chunk = 2 * ks + fh;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int row = wr * 64 + i * 32 + fr;
        af[i] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(As + row * BK + ((chunk ^ ((row >> 1) & 7)) << 3)));
        const int col = wc * 64 + i * 32 + fr;
        bf[i] = __builtin_bit_cast(v8, *reinterpret_cast<const uint4*>(Bs + col * BK + ((chunk ^ ((col >> 1) & 7)) << 3)));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = T16<T>::mfma32(af[i], bf[j], acc[i][j]);
    }
    if (t + 1 < nt) store_tile(buf ^ 1);
    __syncthreads();
  }

  // ---- epilogue ---------------------------------------------------------------------------
  const int64_t cbase = (int64_t)bz * d.strideC;
  const float* __restrict__ res = d.res ? d.res + (int64_t)bz * d.strideR : nullptr;
  float csum[2] = {0.f, 0.f}, csq[2] = {0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int col = n0 + wc * 64 + j * 32 + fr;
    const bool cok = col < d.N;
    const float bn = (d.bias_n && cok) ? d.bias_n[col] : 0.f;
    const float sc = (d.scale_n && cok) ? d.scale_n[col] : 1.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = m0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        if (row < d.M && cok) {
          float v = acc[i][j][r] + bn;
          if (d.bias_m) v += d.bias_m[row];
          if (d.act == ASIS_ACT_GELU) v = gelu_erf(v);
          else if (d.act == ASIS_ACT_RELU) v = fmaxf(v, 0.f);
          v *= sc;
          if (res) v += res[(int64_t)row * d.ldr + col];
          if (d.out_f32) reinterpret_cast<float*>(d.C)[cbase + (int64_t)row * d.ldc + col] = v;
          else reinterpret_cast<T*>(d.C)[cbase + (int64_t)row * d.ldc + col] = to_t16<T>(v);
          csum[j] += v;
          csq[j] += v * v;
        }
      }
    }
  }
  if (d.stats) {
    // deterministic per-(tile_m, column) partial sums: lanes l / l+32 hold the same column,
    // waves wr=0/1 the two row halves; combine through LDS (free after the last barrier).
    float* red = reinterpret_cast<float*>(lds);  // [2 wr][2 kind][128 col]
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float s = csum[j] + __shfl_xor(csum[j], 32, 64);
      float q = csq[j] + __shfl_xor(csq[j], 32, 64);
      if (fh == 0) {
        red[(wr * 2 + 0) * BN + wc * 64 + j * 32 + fr] = s;
        red[(wr * 2 + 1) * BN + wc * 64 + j * 32 + fr] = q;
      }
    }
    __syncthreads();
    if (tid < BN) {
      const int col = n0 + tid;
      if (col < d.N) {
        d.stats[((int64_t)tile_m * 2 + 0) * d.N + col] = red[0 * BN + tid] + red[2 * BN + tid];
        d.stats[((int64_t)tile_m * 2 + 1) * d.N + col] = red[1 * BN + tid] + red[3 * BN + tid];
      }
    }
  }
}

#include "gemm_big.h"
#include "gemm_p8.h"

// ---- host side: options -> plan -> launch ---------------------------------------------------------------------------------
static int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
static int env_positive(const char* name, int dflt) { const int v = env_int(name, dflt); return v > 0 ? v : dflt; }

// Every switch of the dispatcher, read from the environment once, on first use ("p8" also through asis_gemm_set_option).
struct GemmOpts {
  int group_m = env_positive("ASIS_GEMM_GROUPM", 4);  // raster group height of the large-tile kernels
  // the large-tile LDS-DMA kernels (gemm_big.h); 0 forces the 128x128 register-staged kernel, 2 / 3 keep the older 256x256 /
  // 256x128x64 dense forms selectable for A/B runs
  int big = env_int("ASIS_GEMM_BIG", 1);
  // 1: dense launches with at least one 256x256 tile per CU run on the PERSISTENT form of the 8-phase kernel (gemm_p8.h: one
  // workgroup per CU walks its tiles, the next tile's first K tile is staged during the last K tile of the current one, the
  // epilogue's stores drain under the next tile) when K <= 2048 (at K = 4096 a tile is 64 K tiles long and the per-tile savings
  // no longer pay for the static tile lists: 347 vs 341 us); split-precision halves (A_lo / B_lo) are further K parts of the
  // same stream; 2 = any K, from 16 tiles on (tests); 3 = any K; 0 = never
  int p8 = env_int("ASIS_GEMM_P8", 1);
  // 0 = never; 1 = K >= 2048 (fc2 / its input gradient: 343 vs 476 us at 42348x1024x4096) and, since the phases run on
  // 16x16x32 MFMAs (ph8_m16: fc2 391 -> 350 us in isolation), the unbatched K >= 1024 GEMMs too (in the step: qk 222 -> 214 us,
  // proj 160 -> 139, fc1 457 -> 441, adapter projections 242 -> 216; +3.5 % on the step) — the batched ragged V^T GEMM lost
  // there at first (66 vs 72 us: coarser tile quantisation) and wins since the form's 16-bit outputs are converted before the
  // LDS transposition (+0.9 % on the step); (only when there are at least 128 of its 256x256 tiles: a launch that cannot fill
  // the chip is better off with twice as many 256x128 tiles); 3 = K >= 2048 only (the round-1 rule); 2 = wherever the shape allows
  int ph8 = env_int("ASIS_GEMM_8P", 1);
  int ph8_mink = env_int("ASIS_GEMM_8P_MINK", 1024);  // lab: the K >= 1024 of the rule above (not of the LayerNorm-fold launches)
  // the phases issue 16 v_mfma_f32_16x16x32 instead of 8 32x32x16 (same FLOP, higher clock); the persistent, LayerNorm-fold and
  // SwiGLU forms exist on these phases only
  int ph8_m16 = env_int("ASIS_GEMM_8P_M16", 1);
  int ph8_slab32 = env_int("ASIS_GEMM_8P_SLAB32", 0);  // lab: 16-bit outputs through the fp32 slab epilogue like the others
  int m16 = env_int("ASIS_GEMM_M16", 1);               // 16x16x32 MFMAs in the default dense form
  int mx_ph8 = env_int("ASIS_MX_PH8", 1);              // lab: 0 = MX convolutions on the generic large-tile forms only
  int conv_bk32 = env_int("ASIS_CONV_BK32", 0);        // 32-wide K tiles in the 256x128 split convolution
  // <= 64 output channels: 512x64 tile, 8 waves of 64x64 (1 KB of LDS fragment reads per MFMA; the 256x64 form's 32x64 wave
  // tiles need 1.5 KB and are LDS-bound), one workgroup per CU: +0.6 % on the step (0: old form)
  int conv_t512 = env_int("ASIS_CONV_T512", 1);
  int conv_m16 = env_int("ASIS_CONV_M16", 0);          // 16x16x32 MFMAs in the split convs
  // convolutions with whole 256-column tiles on the 8-phase 256x256x64 main loop (gemm_big.h): the long reductions of the
  // decoder convs are where that loop is at its best (K = 9 * Cin * 3 parts)
  int conv_8p = env_int("ASIS_CONV_8P", 1);
};
static GemmOpts& gemm_opts() { static GemmOpts o; return o; }

// One enumerator per kernel instantiation the dispatcher can reach (what each is for: include/asis_hip.h, asis_gemm_plan).
// Names: tile, then variant (m16 = 16x16x32 MFMAs, split = A_lo / B_lo K parts, mx = MX lo operands, ln = LayerNorm fold).
#define ASIS_GEMM_FORMS(X)                                                                                                  \
  X(P8, "p8") X(P8_LN, "p8_ln") X(PH8_M16, "ph8_m16") X(PH8_M32, "ph8_m32") X(PH8_LN, "ph8_ln") X(PH8_MX, "ph8_mx")         \
  X(BIG_256x128_M16, "big_256x128_m16") X(BIG_256x128, "big_256x128") X(BIG_256x128_K64, "big_256x128_k64")                 \
  X(BIG_256x256, "big_256x256") X(BIG_256x128_SPLIT, "big_256x128_split") X(BIG_256x64_SPLIT, "big_256x64_split")           \
  X(CONV_PH8, "conv_ph8") X(CONV_256x128, "conv_256x128") X(CONV_256x64, "conv_256x64") X(CONV_PH8_SPLIT, "conv_ph8_split") \
  X(CONV_512x64_SPLIT, "conv_512x64_split") X(CONV_512x64_SPLIT_M16, "conv_512x64_split_m16")                               \
  X(CONV_256x128_SPLIT, "conv_256x128_split") X(CONV_256x128_SPLIT_M16, "conv_256x128_split_m16")                           \
  X(CONV_256x128_SPLIT_BK32, "conv_256x128_split_bk32") X(CONV_256x64_SPLIT, "conv_256x64_split")                           \
  X(CONV_PH8_MX, "conv_ph8_mx") X(CONV_512x64_MX, "conv_512x64_mx") X(CONV_256x128_MX, "conv_256x128_mx")                   \
  X(CONV_256x64_MX, "conv_256x64_mx") X(GENERIC, "generic") X(GENERIC_CONV, "generic_conv")
#define X(id, name) F_##id,
enum GemmForm { ASIS_GEMM_FORMS(X) F_COUNT };
#undef X
#define X(id, name) name,
const char* const kFormNames[F_COUNT] = {ASIS_GEMM_FORMS(X)};
#undef X

struct GemmPlan {
  int form, grid_x, grid_y, block;
  int group_m;   // second kernel argument of the large-tile forms: GemmOpts::group_m | 0x10000 (fp32 slab epilogue, lab)
  const char* why;   // of a refusal that has a message of its own (the vector-epilogue requirement), else null
};
// The first property that keeps batch entry / K part bz off the vector epilogue (gemm_big.h: gemm_big_vec_epilogue is the
// predicate; this only words its refusal).
const char* vec_epilogue_misfit(const asis_gemm_desc& d, int bz) {
  auto off16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) != 0; };
  if (d.N % 4 || d.ldc % 4) return "N and ldc must be multiples of 4";
  if (off16(d.C)) return "C must be 16-byte aligned";
  if (bz > 0 && d.strideC % 4) return "strideC must be a multiple of 4";
  if (d.res && d.ldr % 4) return "ldr must be a multiple of 4";
  if (d.res && off16(d.res + (int64_t)bz * d.strideR)) return "res must be 16-byte aligned in every batch entry (strideR a multiple of 4)";
  if (d.bias_n && off16(d.bias_n)) return "bias_n must be 16-byte aligned";
  if (d.scale_n && off16(d.scale_n)) return "scale_n must be 16-byte aligned";
  return "an operand is off its 16-byte boundary";
}

// Which form a validated descriptor runs on, and its launch geometry; ASIS_EINVAL when no form takes it (p->why: a refusal with
// a message of its own).  Pure: no HIP call, pointers are only tested for null and alignment.  The order of the cascade is behaviour.
int gemm_plan(const asis_gemm_desc& d, const GemmOpts& o, GemmPlan* p) {
  auto al = [](const void* q, int a) { return (reinterpret_cast<uintptr_t>(q) & (a - 1)) == 0; };
  auto tiles = [&](int bm, int bn) { return (int64_t)((d.M + bm - 1) / bm) * ((d.N + bn - 1) / bn); };
  auto take = [&](GemmForm f, int64_t gx, int gy, int block = 512, int flags = 0) {
    *p = GemmPlan{f, (int)gx, gy, block, o.group_m | flags, nullptr};
    // the large-tile kernel (every form but these four) chooses its epilogue at run time (gemm_big_vec_epilogue): statistics,
    // GELU' and K parts exist in the vector epilogue only
    const bool big_kernel = f != F_GENERIC && f != F_GENERIC_CONV && f != F_P8 && f != F_P8_LN;
    if (big_kernel && (d.stats || d.act == ASIS_ACT_GELU_GRAD || d.ksplit > 1))
      for (int bz = 0; bz < (gy > 1 ? 2 : 1); ++bz)
        if (!gemm_big_vec_epilogue(d, (int64_t)bz * d.strideC, d.res ? d.res + (int64_t)bz * d.strideR : nullptr)) {
          p->why = vec_epilogue_misfit(d, bz);
          return (int)ASIS_EINVAL;
        }
    return (int)ASIS_OK;
  };
  const bool vec_ok = (d.N % 4 == 0) && (d.ldc % 4 == 0);
  const bool split = d.A_lo != nullptr || d.B_lo != nullptr;
  const bool mx_pair = d.mx_amax_a && d.mx_amax_b && d.A_lo && d.B_lo;
  const bool ph8_m16 = o.ph8_m16 != 0;
  const int64_t t256 = tiles(256, 256);              // 256x256 tiles: the grid of every 8-phase form
  const int ky = d.ksplit > 1 ? d.ksplit : 1;        // grid.y of a convolution: its K parts
  // the 8-phase K rule (GemmOpts::ph8) and the convolution shapes of the 8-phase loop: whole 256-column tiles
  auto ph8_k = [&](int mink) { return o.ph8 == 2 || d.K >= 2048 || (o.ph8 == 1 && d.K >= mink && t256 * d.batch >= 128); };
  const bool conv_ph8_shape = d.N >= 256 && (d.N % 256 == 0 || d.N >= 1024) && d.batch == 1;
  // the 256-row large tile of the split / convolution forms: 128 columns, 64 for <= 64 output channels
  const int bn = d.N > 64 ? 128 : 64;

  if (d.act == ASIS_ACT_GELU_GRAD) {  // only the vector epilogue of the large-tile kernels implements it
    const bool ok = o.big && !d.conv && !split && !d.stats && d.aux && d.K % 32 == 0 && d.M >= 256 && d.N >= 128 && vec_ok &&
                    d.ld_aux % 4 == 0 && d.batch == 1 && al(d.aux, 8) && al(d.C, 16) && !d.bias_m;
    if (!ok) return ASIS_EINVAL;
  }
  if (d.act == ASIS_ACT_SILU_MUL) {
    // SwiGLU epilogue: lives in the 16-bit fast path of the 8-phase 16x16-MFMA instances (gemm_big.h) — the launch goes there
    // directly or is refused (a fall-through to another epilogue would write x1 | x2 as if they were outputs)
    const bool ok = o.big && ph8_m16 && !d.conv && (mx_pair || !split) && !d.out_f32 && !d.res && !d.res16 && !d.C_lo && !d.rowstats &&
                    !d.stats && !d.scale_n && !d.bias_m && !d.ln_mr && !d.aux && d.batch == 1 && d.ksplit <= 1 && d.K % 64 == 0 && d.M >= 256 &&
                    d.N >= 256 && d.N % 32 == 0 && d.ldc % 8 == 0 && d.ldc >= d.N / 2 && al(d.C, 16) && (!d.bias_n || al(d.bias_n, 16)) &&
                    (int64_t)d.N * d.ldb < (1ll << 31);
    if (!ok) return ASIS_EINVAL;
    return take(mx_pair ? F_PH8_MX : F_PH8_M16, t256, 1);
  }
  if (d.ksplit > 1 && !(o.big && d.conv)) return ASIS_EINVAL;
  {  // the persistent 8-phase kernel (GemmOpts::p8)
    const int kparts = 1 + (d.A_lo ? 1 : 0) + (d.B_lo ? 1 : 0);
    if (o.p8 && o.big && ph8_m16 && !d.conv && !d.stats && d.batch == 1 && !d.bias_m && !d.ln_cols && !d.C_lo && !d.rowstats && !d.res16 &&
        !d.mx_amax_a && !d.mx_amax_b &&
        d.ksplit <= 1 && d.K % 64 == 0 &&
        d.M >= 256 && d.N >= 256 && t256 >= (o.p8 == 2 ? 16 : 256) && d.K >= 128 && (o.p8 >= 2 || d.K * kparts <= 2048) &&
        (int64_t)d.M * d.lda * 2 < (1ll << 32) && (int64_t)d.N * d.ldb * 2 < (1ll << 32) && d.N % 8 == 0 && d.ldc % 8 == 0 &&
        al(d.C, 16) && (!d.res || (al(d.res, 16) && d.ldr % 4 == 0)) && (!d.bias_n || al(d.bias_n, 16)) && (!d.scale_n || al(d.scale_n, 16)) &&
        (d.act != ASIS_ACT_GELU_GRAD || (d.aux && al(d.aux, 8) && d.ld_aux % 4 == 0)))
      return take(d.ln_mr ? F_P8_LN : F_P8, t256 >= 256 ? 256 : (int)(t256 / 8) * 8, 1);
  }
  // LayerNorm-fold fields (C_lo / rowstats / res16 / ln_mr): implemented by the persistent kernel above and by the dense 8-phase
  // one-tile-per-workgroup form below; anything else is refused (the caller runs asis_layernorm and plain launches)
  const bool lnx = d.C_lo || d.rowstats || d.res16 || d.ln_mr;
  if (lnx) {
    const bool ph8_ok = o.ph8 && ph8_m16 && o.big && !split && !d.conv && !d.stats && d.K % 64 == 0 && d.M >= 256 && d.N >= 256 &&
                        ph8_k(1024) &&
                        d.N % 8 == 0 && d.ldc % 8 == 0 && (!d.res16 || (d.res16_lo && d.ldr16 % 8 == 0 && d.ldr16 >= d.N && al(d.res16, 16) && al(d.res16_lo, 16))) &&
                        (!d.C_lo || !d.out_f32) && (!d.ln_mr || d.ln_cs) &&
                        // producer launches (dedicated 8-columns-per-lane epilogue of gemm_big.h): plain v = res + scale * (acc + bias)
                        (!(d.C_lo || d.rowstats || d.res16) ||
                         ((!d.res || (d.ldr % 8 == 0 && al(d.res, 16))) && (!d.C_lo || al(d.C_lo, 16)) && al(d.C, 16) &&
                          (!d.bias_n || al(d.bias_n, 16)) && (!d.scale_n || al(d.scale_n, 16)) && d.batch == 1 && !d.bias_m &&
                          d.act == ASIS_ACT_NONE && !d.ln_mr));
    if (!ph8_ok) return ASIS_EINVAL;
  }
  if (split) {  // one pass over the virtual 3K reduction; only on the large-tile kernel
    const bool ok = o.big && d.K % BK == 0 && d.M >= 256 && d.N >= 32 && vec_ok && (d.out_f32 || !d.conv) &&
                    (!d.conv || (d.Cin % BK == 0 && d.A_lo && d.B_lo));
    if (!ok) return ASIS_EINVAL;
    if (d.ksplit > 1 && (d.batch != 1 || d.stats || (d.KH * d.KW) % d.ksplit != 0 || !d.out_f32 || d.res)) return ASIS_EINVAL;
    const int64_t gx = tiles(256, bn), gx512 = tiles(512, 64);
    const int gy = d.ksplit > 1 ? d.ksplit : d.batch;
    if (d.mx_amax_a || d.mx_amax_b) {
      // MX form of the lo operands (include/asis_hip.h): two K parts, the second on the block-scaled fp8 MFMA; 16x16 MFMA
      // instances of the three convolution tile forms
      if (!mx_pair) return ASIS_EINVAL;
      if (!d.conv) {   // dense: the 8-phase one-tile-per-workgroup form, K tiles alternating 16-bit / MX
        if (!(d.K % 64 == 0 && d.N >= 256 && d.batch == 1 && d.ksplit <= 1 && !d.stats && (int64_t)d.N * d.ldb < (1ll << 31))) return ASIS_EINVAL;
        return take(F_PH8_MX, t256, 1);
      }
      if ((int64_t)d.B_ * d.H * d.W * d.Cin >= (1ll << 31) || (int64_t)d.N * d.ldb >= (1ll << 31) || d.H >= 65536 || d.W >= 65536) return ASIS_EINVAL;
      if (o.mx_ph8 && conv_ph8_shape) return take(F_CONV_PH8_MX, t256, ky);
      if (bn == 64 && d.ksplit <= 1 && d.M >= 512) return take(F_CONV_512x64_MX, gx512, 1);
      return take(bn == 128 ? F_CONV_256x128_MX : F_CONV_256x64_MX, gx, gy);
    }
    if (d.conv && o.conv_8p && conv_ph8_shape) return take(F_CONV_PH8_SPLIT, t256, ky);
    if (d.conv && bn == 64 && o.conv_t512 && d.ksplit <= 1 && d.M >= 512) return take(o.conv_m16 ? F_CONV_512x64_SPLIT_M16 : F_CONV_512x64_SPLIT, gx512, 1);
    if (d.conv) {
      if (bn == 64) return take(F_CONV_256x64_SPLIT, gx, gy);
      return take(o.conv_bk32 ? F_CONV_256x128_SPLIT_BK32 : o.conv_m16 ? F_CONV_256x128_SPLIT_M16 : F_CONV_256x128_SPLIT, gx, gy);
    }
    return take(bn == 128 ? F_BIG_256x128_SPLIT : F_BIG_256x64_SPLIT, gx, gy);
  }
  const bool dense_big = o.big && !d.conv && !d.stats && d.M >= 256;
  if (o.ph8 && ph8_k(o.ph8_mink) && dense_big && d.K % 64 == 0 && d.N >= 256) {
    // 256x256x64 tile, 8-phase main loop (one workgroup per CU: 128 KB of LDS)
    if (!ph8_m16) return take(F_PH8_M32, t256, d.batch);
    if (lnx) return take(F_PH8_LN, t256, d.batch);
    return take(F_PH8_M16, t256, d.batch, 512, o.ph8_slab32 ? 0x10000 : 0);
  }
  if (dense_big && d.K % 32 == 0 && d.N >= 128) {
    // 256x128x32 tile, 3 LDS stages (72 KB) and <= 128 VGPRs: TWO workgroups per CU, so one workgroup's epilogue
    // (HBM-write bound) overlaps the other's K loop: +12-15 % over the 1-workgroup 256x256x64 / 256x128x64 forms
    // on the fc1 shape (scripts/gemm_lab.hip).
    if (o.big == 2 && d.N >= 2048) return take(F_BIG_256x256, t256, d.batch);
    return take(o.big >= 2 ? F_BIG_256x128_K64 : o.m16 ? F_BIG_256x128_M16 : F_BIG_256x128, tiles(256, 128), d.batch);
  }
  // implicit-GEMM convolution on the same kernel: K tiles must lie inside one tap, and BatchNorm statistics
  // come from the vectorised epilogue
  if (o.big && d.conv && d.Cin % BK == 0 && d.M >= 256 && d.N >= 32 && vec_ok && d.out_f32) {
    if (d.ksplit > 1 && (d.stats || (d.KH * d.KW) % d.ksplit != 0 || d.res)) return ASIS_EINVAL;
    if (o.conv_8p && conv_ph8_shape) return take(F_CONV_PH8, t256, ky);
    return take(bn == 128 ? F_CONV_256x128 : F_CONV_256x64, tiles(256, bn), ky);
  }
  if (d.ksplit > 1) return ASIS_EINVAL;  // K parts exist on the large-tile conv forms only
  return take(d.conv ? F_GENERIC_CONV : F_GENERIC, tiles(BM, BN), d.batch, NTHREADS);
}

// One launch per form: the template instantiations of this file.
template <typename T>
void launch(hipStream_t s, const asis_gemm_desc& d, const GemmPlan& p) {
  const dim3 grid(p.grid_x, p.grid_y), block(p.block);
  const int gm = p.group_m;
  switch (p.form) {
    case F_P8: hipLaunchKernelGGL((gemm_p8_kernel<T, 0>), grid, block, 0, s, d, gm); break;
    case F_P8_LN: hipLaunchKernelGGL((gemm_p8_kernel<T, 1>), grid, block, 0, s, d, gm); break;
    case F_PH8_M16: hipLaunchKernelGGL((gemm_big_kernel<T, 2, 4, 4, 2, 2, 0, false, false, 64, 1, true, true>), grid, block, 0, s, d, gm); break;
    case F_PH8_M32: hipLaunchKernelGGL((gemm_big_kernel<T, 2, 4, 4, 2, 2, 0, false, false, 64, 1, true>), grid, block, 0, s, d, gm); break;
    case F_PH8_LN: hipLaunchKernelGGL((gemm_big_kernel<T, 2, 4, 4, 2, 2, 0, false, false, 64, 1, true, true, 1>), grid, block, 0, s, d, gm); break;
    case F_PH8_MX: hipLaunchKernelGGL((gemm_big_kernel<T, 2, 4, 4, 2, 2, 0, false, true, 64, 1, true, true, 0, true>), grid, block, 0, s, d, gm); break;
    case F_BIG_256x128_M16: hipLaunchKernelGGL((gemm_big_kernel<T, 4, 2, 2, 2, 3, 0, false, false, 32, 4, false, true>), grid, block, 0, s, d, gm); break;
    case F_BIG_256x128: hipLaunchKernelGGL((gemm_big_kernel<T, 4, 2, 2, 2, 3, 0, false, false, 32, 4>), grid, block, 0, s, d, gm); break;
    case F_BIG_256x128_K64: hipLaunchKernelGGL((gemm_big_kernel<T, 4, 2, 2, 2, 3>), grid, block, 0, s, d, gm); break;
    case F_BIG_256x256: hipLaunchKernelGGL((gemm_big_kernel<T, 2, 4, 4, 2, 2>), grid, block, 0, s, d, gm); break;
    case F_BIG_256x128_SPLIT: hipLaunchKernelGGL((gemm_big_kernel<T, 4, 2, 2, 2, 3, 0, false, true>), grid, block, 0, s, d, gm); break;
    case F_BIG_256x64_SPLIT: hipLaunchKernelGGL((gemm_big_kernel<T, 8, 1, 1, 2, 3, 0, false, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_PH8: hipLaunchKernelGGL((gemm_big_kernel<T, 2, 4, 4, 2, 2, 0, true, false, 64, 1, true, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_256x128: hipLaunchKernelGGL((gemm_big_kernel<T, 4, 2, 2, 2, 3, 0, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_256x64: hipLaunchKernelGGL((gemm_big_kernel<T, 8, 1, 1, 2, 3, 0, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_PH8_SPLIT: hipLaunchKernelGGL((gemm_big_kernel<T, 2, 4, 4, 2, 2, 0, true, true, 64, 1, true, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_512x64_SPLIT: hipLaunchKernelGGL((gemm_big_kernel<T, 8, 1, 2, 2, 2, 0, true, true, 64, 1>), grid, block, 0, s, d, gm); break;
    case F_CONV_512x64_SPLIT_M16: hipLaunchKernelGGL((gemm_big_kernel<T, 8, 1, 2, 2, 2, 0, true, true, 64, 1, false, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_256x128_SPLIT: hipLaunchKernelGGL((gemm_big_kernel<T, 4, 2, 2, 2, 3, 0, true, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_256x128_SPLIT_M16: hipLaunchKernelGGL((gemm_big_kernel<T, 4, 2, 2, 2, 3, 0, true, true, 64, 2, false, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_256x128_SPLIT_BK32: hipLaunchKernelGGL((gemm_big_kernel<T, 4, 2, 2, 2, 3, 0, true, true, 32, 4>), grid, block, 0, s, d, gm); break;
    case F_CONV_256x64_SPLIT: hipLaunchKernelGGL((gemm_big_kernel<T, 8, 1, 1, 2, 3, 0, true, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_PH8_MX: hipLaunchKernelGGL((gemm_big_kernel<T, 2, 4, 4, 2, 2, 0, true, true, 64, 1, true, true, 0, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_512x64_MX: hipLaunchKernelGGL((gemm_big_kernel<T, 8, 1, 2, 2, 2, 0, true, true, 64, 1, false, true, 0, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_256x128_MX: hipLaunchKernelGGL((gemm_big_kernel<T, 4, 2, 2, 2, 3, 0, true, true, 64, 1, false, true, 0, true>), grid, block, 0, s, d, gm); break;
    case F_CONV_256x64_MX: hipLaunchKernelGGL((gemm_big_kernel<T, 8, 1, 1, 2, 3, 0, true, true, 64, 1, false, true, 0, true>), grid, block, 0, s, d, gm); break;
    case F_GENERIC: hipLaunchKernelGGL((gemm_kernel<T, false>), grid, block, 0, s, d); break;
    case F_GENERIC_CONV: hipLaunchKernelGGL((gemm_kernel<T, true>), grid, block, 0, s, d); break;
  }
}

// The argument checks and the plan of both entry points; *out = the descriptor as the kernels take it (batch >= 1).
int gemm_prepare(const asis_gemm_desc* dp, asis_gemm_desc* out, GemmPlan* p) {
  ASIS_REQUIRE(dp != nullptr, "asis_gemm: null descriptor");
  asis_gemm_desc& d = *out;
  d = *dp;
  ASIS_REQUIRE(d.A && d.B && d.C, "asis_gemm: null operand pointer");
  ASIS_REQUIRE(d.M > 0 && d.N > 0 && d.K > 0, "asis_gemm: M,N,K must be positive (got %d,%d,%d)", d.M, d.N, d.K);
  ASIS_DT_OK(d.dtype, "asis_gemm");
  ASIS_REQUIRE(d.K % 8 == 0, "asis_gemm: K=%d must be a multiple of 8", d.K);
  ASIS_REQUIRE(d.ldb % 8 == 0 && d.ldb >= d.K, "asis_gemm: ldb=%ld must be a multiple of 8 and >= K", (long)d.ldb);
  ASIS_REQUIRE(asis_aligned16(d.A) && asis_aligned16(d.B), "asis_gemm: A and B must be 16-byte aligned");
  ASIS_REQUIRE(d.strideA % 8 == 0 && d.strideB % 8 == 0, "asis_gemm: batch strides must be multiples of 8");
  ASIS_REQUIRE(d.ldc >= (d.act == ASIS_ACT_SILU_MUL ? d.N / 2 : d.N), "asis_gemm: ldc=%ld < N=%d", (long)d.ldc, d.N);
  ASIS_REQUIRE(d.act >= 0 && d.act <= ASIS_ACT_GELU_GRAD, "asis_gemm: bad act %d", d.act);
  if (d.batch <= 0) d.batch = 1;
  ASIS_REQUIRE(d.batch <= 65535, "asis_gemm: batch %d too large", d.batch);
  if (d.res) ASIS_REQUIRE(d.ldr >= d.N, "asis_gemm: ldr=%ld < N", (long)d.ldr);
  if (d.conv) {
    ASIS_REQUIRE(d.batch == 1, "asis_gemm: conv mode needs batch == 1 (batch is folded into M)");
    ASIS_REQUIRE(d.Cin % 8 == 0 && d.Cin > 0, "asis_gemm: conv Cin=%d must be a multiple of 8", d.Cin);
    ASIS_REQUIRE(d.KH > 0 && d.KW > 0 && d.stride > 0 && d.pad >= 0, "asis_gemm: bad conv geometry");
    ASIS_REQUIRE(d.K == d.KH * d.KW * d.Cin, "asis_gemm: conv K=%d != KH*KW*Cin=%d", d.K, d.KH * d.KW * d.Cin);
    ASIS_REQUIRE(d.OH == (d.H + 2 * d.pad - d.KH) / d.stride + 1 && d.OW == (d.W + 2 * d.pad - d.KW) / d.stride + 1,
                 "asis_gemm: conv output size mismatch");
    ASIS_REQUIRE((int64_t)d.B_ * d.OH * d.OW == d.M, "asis_gemm: conv M=%d != B*OH*OW", d.M);
  } else {
    ASIS_REQUIRE(d.lda % 8 == 0 && d.lda >= d.K, "asis_gemm: lda=%ld must be a multiple of 8 and >= K", (long)d.lda);
  }
  if (d.stats) ASIS_REQUIRE(d.batch == 1, "asis_gemm: stats need batch == 1");
  if (d.res16) ASIS_REQUIRE(d.res16_lo && !d.res && d.ldr16 % 4 == 0 && d.ldr16 >= d.N && (reinterpret_cast<uintptr_t>(d.res16) & 7) == 0 &&
                            (reinterpret_cast<uintptr_t>(d.res16_lo) & 7) == 0, "asis_gemm: res16 needs res16_lo, no fp32 res, ldr16 %% 4 == 0, 8-byte aligned planes");
  if (d.C_lo) ASIS_REQUIRE(!d.out_f32 && (reinterpret_cast<uintptr_t>(d.C_lo) & 7) == 0, "asis_gemm: C_lo is the second plane of a 16-bit output");
  if (d.ln_mr) ASIS_REQUIRE(d.ln_cs && (reinterpret_cast<uintptr_t>(d.ln_mr) & 7) == 0 && asis_aligned16(d.ln_cs), "asis_gemm: ln_mr needs ln_cs (16-byte aligned)");
  if (d.rowstats) ASIS_REQUIRE(d.batch == 1 && (reinterpret_cast<uintptr_t>(d.rowstats) & 7) == 0, "asis_gemm: rowstats need batch == 1");
  // the row statistics are per 64-column group ([M, N / 64, 2]): a ragged last group would need its own count in the finalizer
  if (d.rowstats) ASIS_REQUIRE(d.N % 64 == 0, "asis_gemm: rowstats need N %% 64 == 0 (N = %d)", (int)d.N);
  const int64_t tiles = (int64_t)asis_cdiv(d.M, BM) * asis_cdiv(d.N, BN);
  ASIS_REQUIRE(tiles < (1ll << 31), "asis_gemm: too many tiles");
  ASIS_REQUIRE(!d.conv || (d.A_lo == nullptr) == (d.B_lo == nullptr), "asis_gemm: a split convolution needs both A_lo and B_lo");
  ASIS_REQUIRE((!d.A_lo || asis_aligned16(d.A_lo)) && (!d.B_lo || asis_aligned16(d.B_lo)), "asis_gemm: split halves must be 16-byte aligned");
  p->why = nullptr;
  const int rc = gemm_plan(d, gemm_opts(), p);  // nonzero = no kernel form takes this descriptor
  if (rc != 0 && p->why)
    ASIS_FAIL(ASIS_EINVAL, "asis_gemm: stats / ASIS_ACT_GELU_GRAD / ksplit run in the vector epilogue of the large-tile kernels only: %s "
                           "(include/asis_hip.h)", p->why);
  if (rc != 0 && d.act == ASIS_ACT_SILU_MUL)
    ASIS_FAIL(ASIS_EINVAL, "asis_gemm: ASIS_ACT_SILU_MUL needs a dense 16-bit-output launch on the 8-phase form (include/asis_hip.h: K %% 64 == 0, "
                           "M >= 256, N >= 256, N %% 32 == 0, ldc %% 8 == 0, plain or MX split operands, bias only)");
  if (rc != 0) ASIS_FAIL(ASIS_EINVAL, "asis_gemm: split-precision operands / ASIS_ACT_GELU_GRAD / ksplit need the large-tile path (K %% 64 "
                                        "== 0 (GELU_GRAD: 32), M >= 256, N >= 32 (128), N and ldc multiples of 4, fp32 output for "
                                        "split; conv: Cin %% 64 == 0)");
  return ASIS_OK;
}

}  // namespace

extern "C" int asis_gemm_tiles_m(int M) { return (M + BM - 1) / BM; }

extern "C" int asis_gemm_set_option(const char* name, int value) {
  ASIS_REQUIRE(name != nullptr, "asis_gemm_set_option: null name");
  if (strcmp(name, "p8") == 0) { gemm_opts().p8 = value; return ASIS_OK; }
  ASIS_FAIL(ASIS_EINVAL, "asis_gemm_set_option: unknown option '%s'", name);
}

extern "C" int asis_gemm_plan(const asis_gemm_desc* dp, int* form, int* grid_x, int* grid_y, int* block) {
  asis_gemm_desc d;
  GemmPlan p;
  if (int bad = gemm_prepare(dp, &d, &p)) return bad;
  if (form) *form = p.form;
  if (grid_x) *grid_x = p.grid_x;
  if (grid_y) *grid_y = p.grid_y;
  if (block) *block = p.block;
  return ASIS_OK;
}

extern "C" const char* asis_gemm_form_name(int form) { return form >= 0 && form < F_COUNT ? kFormNames[form] : "?"; }

extern "C" int asis_gemm(void* stream, const asis_gemm_desc* dp) {
  asis_gemm_desc d;
  GemmPlan p;
  if (int bad = gemm_prepare(dp, &d, &p)) return bad;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int bad = asis_dispatch16(d.dtype, "asis_gemm", [&](auto t) { launch<decltype(t)>(s, d, p); })) return bad;
  ASIS_CHECK_LAUNCH("asis_gemm");
  return ASIS_OK;
}
