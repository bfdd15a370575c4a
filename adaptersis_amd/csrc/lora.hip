// Rank-r (LoRA) side of the attention q / v projections: the two skinny products the dense GEMM forms serve badly.
//
//   asis_lora_down   U[R, 0:64]      = round16(X_seg[R, Kt] Wd^T)             Wd 16-bit [64, Kt]
//   asis_lora_wgrad  slab[b][64, Nt] = sum over the rows of block b of U[row, :]^T X_seg[row, :]
//
// X_seg = one or two column segments (col0, len), len % 64 == 0, of a row-strided 16-bit matrix (the LayerNorm output inside
// [xn | u], or the dQ and dV thirds of [dQ | dK | dV | du]); the columns between the segments are never read.  Both kernels are
// bound by their one read of X (87 MB at 42 348 x 1024), so they are laid out for the stream: no X tile is read twice, the 64
// outputs per row (down) and the 64 x Nt sums (wgrad) stay in registers, and the MFMA shape is the small 16x16x32 one.
#include "asis_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// down: one wave owns 32 rows (two 16-row MFMA tiles) and all 64 output columns.  The operand maps of the 16x16x32 MFMA put 8
// consecutive k of ONE row on a lane, so both fragments are plain 16-byte global loads, no LDS: in a 64-wide K step lane group
// g = lane >> 4 takes k = 16 g + 8 s + j for MFMA s = 0, 1 (the sum over k has no order, and both operands use the same
// assignment), i.e. 32 contiguous bytes of its row, the four groups 128 contiguous bytes.  Wd (128 KB at Kt = 1024) is read by
// every wave at the same addresses and stays in L1 / L2.  The product is computed as D[n][row] = Wd X^T: a lane then holds 4
// consecutive output columns of one row, one 8-byte store.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int DOWN_WAVES = 2, DOWN_ROWS = 32;  // rows per wave

template <typename T>
__global__ __launch_bounds__(64 * DOWN_WAVES) void lora_down_kernel(const T* __restrict__ X, int64_t ldx, int c0a, int lena, int c0b,
                                                                    int lenb, const T* __restrict__ Wd, int Kt, T* __restrict__ U,
                                                                    int64_t ldu, int64_t R) {
  typedef typename T16<T>::v8 v8;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int li = lane & 15, g = lane >> 4;
  const int64_t row0 = ((int64_t)blockIdx.x * DOWN_WAVES + wid) * DOWN_ROWS;
  if (row0 >= R) return;  // wave-uniform
  const T* xr[2];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t row = row0 + 16 * rt + li;
    xr[rt] = X + (row < R ? row : R - 1) * ldx + 16 * g;  // rows past the end re-read the last row and store nothing
  }
  const T* wr = Wd + (int64_t)li * Kt + 16 * g;
  f32x4 acc[2][4];
#pragma unroll
  for (int rt = 0; rt < 2; ++rt)
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) acc[rt][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  // K runs in 64-wide chunks over the segments, two register sets in turn: chunk c + 1 is in flight while the MFMAs of chunk c
  // run (the kernel is bound by load latency, not by the MFMAs: 8 KB of X per wave in flight instead of 4)
  const int nca = lena >> 6, nc = Kt >> 6;
  v8 xa[2][2], wb[4][2], xn[2][2], wn[4][2];
  auto load = [&](int c, v8 (&x)[2][2], v8 (&w)[4][2]) {
    const int col = c < nca ? c0a + 64 * c : c0b + 64 * (c - nca);
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
      for (int s = 0; s < 2; ++s) x[rt][s] = *reinterpret_cast<const v8*>(xr[rt] + col + 8 * s);
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
      for (int s = 0; s < 2; ++s) w[nb][s] = *reinterpret_cast<const v8*>(wr + (int64_t)16 * nb * Kt + 64 * c + 8 * s);
  };
  auto mma = [&](const v8 (&x)[2][2], const v8 (&w)[4][2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) acc[rt][nb] = T16<T>::mfma16(w[nb][s], x[rt][s], acc[rt][nb]);
  };
  load(0, xa, wb);
  for (int c = 0; c < nc; c += 2) {
    if (c + 1 < nc) load(c + 1, xn, wn);
    mma(xa, wb);
    if (c + 1 < nc) {
      if (c + 2 < nc) load(c + 2, xa, wb);
      mma(xn, wn);
    }
  }
  // D[n][row]: lane = row li of the tile, registers = output columns 16 nb + 4 g + (0..3)
#pragma unroll
  for (int rt = 0; rt < 2; ++rt) {
    const int64_t row = row0 + 16 * rt + li;
    if (row >= R) continue;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
      u32x2 w;
      w[0] = pack2<T>(acc[rt][nb][0], acc[rt][nb][1]);
      w[1] = pack2<T>(acc[rt][nb][2], acc[rt][nb][3]);
      *reinterpret_cast<u32x2*>(U + row * ldu + 16 * nb + 4 * g) = w;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// wgrad: slab[64, Nt] = U^T X over a block of rows.  The reduction index (rows) is the slow axis of both operands, so the
// tiles are staged [k][column] in LDS (coalesced 16-byte chunks, XOR-swizzled with (k & 3) << 2 as in wgrad.hip) and the
// fragments come from transposing reads.  Workgroup = 64 (all of U's columns) x 128 columns of X_seg, four waves of 64 x 32;
// a 64-column group of X_seg lies inside one segment (len % 64 == 0).  Rows past the block's end are loaded from its last
// row and masked to zero bits on the way to LDS (U AND X: a NaN behind the end of an oversized buffer must not meet a zero).
// ---------------------------------------------------------------------------------------------------------------------
constexpr int WG_BK = 64, WG_BN = 128, WG_LD = 128, WG_THREADS = 256;

template <typename T>
__global__ __launch_bounds__(WG_THREADS, 2) void lora_wgrad_kernel(const T* __restrict__ U, int64_t ldu, const T* __restrict__ X,
                                                                   int64_t ldx, int c0a, int lena, int c0b, int Nt,
                                                                   float* __restrict__ slabs, int64_t R, int64_t rows_per) {
  typedef typename T16<T>::v8 v8;
  typedef s16x4 __attribute__((address_space(3))) * lds_tr_ptr;
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  __shared__ __attribute__((aligned(16))) T lds[2 * 2 * WG_BK * WG_LD];  // [buf][U | X][64 k][128] = 64 KiB

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int n0 = blockIdx.x * WG_BN;
  const int64_t k_begin = (int64_t)blockIdx.y * rows_per;
  int64_t k_end = k_begin + rows_per;
  if (k_end > R) k_end = R;
  const int nt = k_end > k_begin ? (int)((k_end - k_begin + WG_BK - 1) / WG_BK) : 0;

  // loader: thread -> k rows (tid >> 4) + 16 i, 16-byte chunk (tid & 15)
  const int lk = tid >> 4, lch = tid & 15;
  const bool a_ok = lch < 8;
  const int bn = n0 + lch * 8;
  const bool b_ok = bn < Nt;
  const int acol = a_ok ? lch * 8 : 0;
  const int bcol = b_ok ? (bn < lena ? c0a + bn : c0b + (bn - lena)) : c0a;
  uint4 ra[4], rb[4];
  uint32_t okm = 0;
  auto load_tile = [&](int t) {
    okm = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int64_t row = k_begin + (int64_t)t * WG_BK + lk + 16 * i;
      const bool in = row < k_end;
      const int64_t rc = in ? row : k_end - 1;
      okm |= in ? (1u << i) : 0u;
      ra[i] = *reinterpret_cast<const uint4*>(U + rc * ldu + acol);
      rb[i] = *reinterpret_cast<const uint4*>(X + rc * ldx + bcol);
    }
  };
  auto store_tile = [&](int buf) {
    T* As = lds + buf * (2 * WG_BK * WG_LD);
    T* Bs = As + WG_BK * WG_LD;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int k = lk + 16 * i;
      const int sw = (lch ^ ((k & 3) << 2)) << 3;
      const bool row_ok = (okm >> i) & 1u;
      const uint32_t ma = (row_ok && a_ok) ? 0xFFFFFFFFu : 0u, mb = (row_ok && b_ok) ? 0xFFFFFFFFu : 0u;
      *reinterpret_cast<uint4*>(As + k * WG_LD + sw) = make_uint4(ra[i].x & ma, ra[i].y & ma, ra[i].z & ma, ra[i].w & ma);
      *reinterpret_cast<uint4*>(Bs + k * WG_LD + sw) = make_uint4(rb[i].x & mb, rb[i].y & mb, rb[i].z & mb, rb[i].w & mb);
    }
  };

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (nt > 0) {
    load_tile(0);
    store_tile(0);
  }
  __syncthreads();

  // transposed-read geometry of the 16x16x32 operand: lane l holds [column l & 15][k = 8 (l >> 4) + j]; 16-lane group g reads
  // two 4 (k) x 16 (column) blocks, lane 4 q + pc of the group supplying row q, columns 4 pc .. 4 pc + 3
  const int g = lane >> 4, li = lane & 15;
  const int q = li >> 2, pc = li & 3;
  const int n_off = wid * 32;
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) load_tile(t + 1);
    const T* As = lds + buf * (2 * WG_BK * WG_LD);
    const T* Bs = As + WG_BK * WG_LD;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      auto frag = [&](const T* S, int c0) -> v8 {
        s16x4 h[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
          const int k = ks * 32 + 8 * g + 4 * half + q;
          const int swz = (k & 3) << 2;
          h[half] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_tr_ptr)(S + k * WG_LD + ((((c0 >> 3) ^ swz) << 3) | (c0 & 7))));
        }
        return __builtin_bit_cast(v8, (s16x8)__builtin_shufflevector(h[0], h[1], 0, 1, 2, 3, 4, 5, 6, 7));
      };
      v8 af[4], bf[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag(As, 16 * i + 4 * pc);
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = frag(Bs, n_off + 16 * j + 4 * pc);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = T16<T>::mfma16(af[i], bf[j], acc[i][j]);
    }
    if (t + 1 < nt) store_tile(buf ^ 1);
    __syncthreads();
  }

  // D[p][n]: lane = column n, registers = rows 16 i + 4 g + (0..3)
  float* slab = slabs + (int64_t)blockIdx.y * 64 * Nt;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = n0 + n_off + 16 * j + li;
    if (n >= Nt) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) slab[(int64_t)(16 * i + 4 * g + r) * Nt + n] = acc[i][j][r];
  }
}

// rows per block (a multiple of the K tile) and the number of blocks: about two workgroups per CU over all column tiles, at
// least four K tiles per block; every block is non-empty
static inline int64_t lora_wgrad_rows_per(int64_t R, int Nt, int* nblk) {
  const int64_t tiles = asis_cdiv(Nt, WG_BN);
  int64_t want = 512 / tiles;
  const int64_t by_k = asis_cdiv(R, 4 * WG_BK);
  if (want > by_k) want = by_k;
  if (want < 1) want = 1;
  const int64_t rows_per = asis_cdiv(asis_cdiv(R, want), WG_BK) * WG_BK;
  *nblk = (int)asis_cdiv(R, rows_per);
  return rows_per;
}

// the checks both entry points share: the segments of X and the strided [R, 64] matrix U
static int lora_check(const char* entry, const void* x, int64_t ldx, int c0a, int lena, int c0b, int lenb, const void* u, int64_t ldu,
                      int64_t R) {
  ASIS_REQUIRE(x && u, "%s: null pointer", entry);
  ASIS_REQUIRE(R >= 1 && R < (1LL << 31), "%s: R=%ld must be in [1, 2^31)", entry, (long)R);
  ASIS_REQUIRE(asis_aligned16(x) && asis_aligned16(u), "%s: operands must be 16-byte aligned", entry);
  ASIS_REQUIRE(lena >= 64 && lena % 64 == 0 && lenb >= 0 && lenb % 64 == 0, "%s: segment lengths (%d, %d) must be multiples of 64", entry,
               lena, lenb);
  ASIS_REQUIRE(c0a >= 0 && c0a % 8 == 0 && c0b % 8 == 0 && (lenb == 0 || c0b >= c0a + lena),
               "%s: segment columns (%d, %d) must be multiples of 8, in order, not overlapping", entry, c0a, c0b);
  const int64_t extent = lenb ? (int64_t)c0b + lenb : (int64_t)c0a + lena;
  ASIS_REQUIRE(ldx >= extent && ldx % 8 == 0, "%s: ldx=%ld must be a multiple of 8 and cover the segments (%ld columns)", entry, (long)ldx,
               (long)extent);
  ASIS_REQUIRE(ldu >= 64 && ldu % 8 == 0, "%s: ldu=%ld must be a multiple of 8 and at least 64", entry, (long)ldu);
  return ASIS_OK;
}

}  // namespace

extern "C" int asis_lora_down(void* stream, int dtype, const void* x, int64_t ldx, int col0a, int lena, int col0b, int lenb,
                              const void* wd, void* u, int64_t ldu, int64_t R) {
  ASIS_DT_OK(dtype, "asis_lora_down");
  if (int rc = lora_check("asis_lora_down", x, ldx, col0a, lena, col0b, lenb, u, ldu, R)) return rc;
  ASIS_REQUIRE(wd != nullptr && asis_aligned16(wd), "asis_lora_down: wd must be a 16-byte aligned [64, Kt] matrix");
  const int Kt = lena + lenb;
  const dim3 grid((unsigned)asis_cdiv(R, DOWN_WAVES * DOWN_ROWS)), block(64 * DOWN_WAVES);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = asis_dispatch16(dtype, "asis_lora_down", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((lora_down_kernel<T>), grid, block, 0, s, static_cast<const T*>(x), ldx, col0a, lena, col0b, lenb,
                           static_cast<const T*>(wd), Kt, static_cast<T*>(u), ldu, R);
      })) return rc;
  ASIS_CHECK_LAUNCH("asis_lora_down");
  return ASIS_OK;
}

extern "C" int asis_lora_wgrad_nblk(int64_t R, int Nt) {
  if (R < 1 || Nt < 64) return 0;
  int nblk = 0;
  lora_wgrad_rows_per(R, Nt, &nblk);
  return nblk;
}

extern "C" int asis_lora_wgrad(void* stream, int dtype, const void* u, int64_t ldu, const void* x, int64_t ldx, int col0a, int lena,
                               int col0b, int lenb, float* slabs, int nblk, int64_t R) {
  ASIS_DT_OK(dtype, "asis_lora_wgrad");
  if (int rc = lora_check("asis_lora_wgrad", x, ldx, col0a, lena, col0b, lenb, u, ldu, R)) return rc;
  ASIS_REQUIRE(slabs != nullptr && asis_aligned16(slabs), "asis_lora_wgrad: slabs must be a 16-byte aligned fp32 buffer");
  const int Nt = lena + lenb;
  int want = 0;
  const int64_t rows_per = lora_wgrad_rows_per(R, Nt, &want);
  ASIS_REQUIRE(nblk == want, "asis_lora_wgrad: nblk=%d, asis_lora_wgrad_nblk(R, Nt) says %d", nblk, want);
  const dim3 grid((unsigned)asis_cdiv(Nt, WG_BN), (unsigned)nblk), block(WG_THREADS);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (int rc = asis_dispatch16(dtype, "asis_lora_wgrad", [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((lora_wgrad_kernel<T>), grid, block, 0, s, static_cast<const T*>(u), ldu, static_cast<const T*>(x), ldx, col0a,
                           lena, col0b, Nt, slabs, R, rows_per);
      })) return rc;
  ASIS_CHECK_LAUNCH("asis_lora_wgrad");
  return ASIS_OK;
}
