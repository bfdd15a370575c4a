// Lovasz-Softmax loss (segloss/lovasz_loss.py:39-60), fused with the bilinear resize of the logits like the losses of loss.hip.
//
//     q      = softmax^n_softmax(resize(logits))          n_softmax in {0, 1}, at the target's H x W
//     e_c[i] = |t_c[i] - q_c[i]|                           t_c[i] = (target[i] == c), i the flat pixel index of the whole batch
//     loss_c = sum_k e_c(k) g_k                            e_c sorted descending, g = lovasz_grad(t_c in that order)
// over all C classes (absent ones included), no per_image, no ignore index.
//
// Order: descending by the fp32 bit pattern of e (monotone: e >= 0), ties by ascending pixel index: a stable sort from index
// order, so the gradient is reproducible where values tie (torch.sort is not stable).
//
// g in closed form from integer counts (the fp32 difference of two Jaccard values near 1 has no correct digit at 4 M pixels):
// with G = #class pixels, f_k / b_k = #class / #other pixels among sorted positions 0..k, I = G - f_k, U = G + b_k:
//     class pixel: g_k = 1 / U        other: g_k = I / (U (U - 1))        G == 0: g_0 = 1, g_k = 0 otherwise
// evaluated in double.  d loss_c / d q_c[i] = s g_rank(i), s = -1 (class pixel), +1 (other), 0 where e == 0 (abs'(0) = 0 in torch).
//
// Stages (every launch ordered by the stream; NO workgroup waits on another: no look-back, no grid barrier, no flag):
//   keys     one pass over the pixels: taps -> softmax -> per class the key bits and the payload (pixel index | class flag << 31),
//            layout [C][N]
//   sort     LSD radix sort of the C segments at once (class = grid.y), 4 passes of 8 bits over the full 32-bit key, each pass
//            histogram -> row scan -> stable scatter as three launches.  The digit is taken from ~key, ascending = descending e.
//   scan     class-pixel count per tile -> exclusive scan of the tile totals (one workgroup per class, any number of tiles)
//            -> per element f_k, g_k, s g_k stored at [pixel][C] (each element written exactly once, no float atomics) and the
//            tile's partial of sum e g in double, in a fixed order
//   finalize per class the partials summed in double in a fixed order -> per_class, loss
//   dz       one pass over the pixels: q again, reduction factor, softmax transpose (n_softmax = 1), grad_scale; stored or added
//
// Radix width and tile.  8 bits: 256 digits = one digit per thread of a 256-thread workgroup for the histogram / offset steps,
// 4 passes, and 4 KiB of per-wave counters (4 waves x 256) — LDS never limits occupancy.  A wave ranks 64 keys of one round
// with match_digit (radix_routines.h, which also holds the scans, the reductions and the tile constants RX_*): popcounts of
// that 64-bit mask below my lane give the stable rank, and the first lane of each digit bumps the wave's counter: no LDS
// atomics on the scatter path and no same-address serialisation when the digit is nearly constant (the top byte of
// probabilities).  11 bits would save one pass of four but needs 2048 counters per wave and 11 ballots per round, and its
// histogram rows (one per digit and tile) would be 8 times as large as the tile's keys are worth.  Tile: 256 threads x 8 keys
// = 2048 keys, wave-striped (wave w owns keys w*512 .. w*512+511 of the tile, round j the 64 consecutive ones from j*64:
// coalesced 256-byte loads, and the order of the keys is wave, round, lane).  8 keys per thread keep 24 live registers of keys /
// payloads / ranks: 8 workgroups per CU stay resident.
#include "asis_common.h"
#include "bilinear_tap.h"  // MAXC, sample_logits_at, softmax_c, softmax_bwd_c
#include "radix_routines.h"

namespace {

// position of (wave, round, lane) in the tile that starts at `base`
__device__ __forceinline__ int64_t tile_pos(int64_t base, int wv, int j, int lane) { return base + wv * (RX_ITEMS * 64) + j * 64 + lane; }

__global__ __launch_bounds__(RX_THREADS) void lovasz_keys_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                 int h, int w, int H, int W, int C, int n_softmax, int64_t N,
                                                                 uint32_t* __restrict__ key, uint32_t* __restrict__ pay,
                                                                 float* __restrict__ dbg_keys) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    float z[MAXC];
    sample_logits_at(logits, h, w, H, W, C, i, z);
    if (n_softmax) softmax_c(z, C);
    const int64_t t = target[i];
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < C) {
        const bool f = (t == (int64_t)c);
        const float e = fabsf((f ? 1.f : 0.f) - z[c]);
        key[(int64_t)c * N + i] = __builtin_bit_cast(uint32_t, e);
        pay[(int64_t)c * N + i] = (uint32_t)i | (f ? 0x80000000u : 0u);
        if (dbg_keys) dbg_keys[(int64_t)c * N + i] = e;
      }
  }
}

// hist[(c * 256 + digit) * nblk + tile] = number of keys of the tile with that digit
__global__ __launch_bounds__(RX_THREADS) void lovasz_hist_kernel(const uint32_t* __restrict__ key, int64_t N, int nblk, int shift,
                                                                 int* __restrict__ hist) {
  __shared__ int hs[RX_RADIX];
  const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  hs[tid] = 0;
  __syncthreads();
  const uint32_t* k = key + (int64_t)c * N;
  const int64_t base = (int64_t)blk * RX_TILE;
#pragma unroll
  for (int j = 0; j < RX_ITEMS; ++j) {
    const int64_t p = tile_pos(base, wv, j, lane);
    const bool valid = p < N;
    count_digit(hs, valid ? (int)((~k[p] >> shift) & 255u) : 0, valid, lane);
  }
  __syncthreads();
  hist[((int64_t)c * RX_RADIX + tid) * nblk + blk] = hs[tid];
}

// rows of n ints, one workgroup per row: exclusive scan in place, the row's sum to totals[row].  Any n.
__global__ __launch_bounds__(RX_THREADS) void lovasz_rowscan_kernel(int* __restrict__ data, int n, int* __restrict__ totals) {
  __shared__ int ws[RX_WAVES];
  const int total = block_rowscan(data + (int64_t)blockIdx.x * n, n, ws);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// stable scatter of one tile by the digit at `shift`: hist holds the row-scanned counts (exclusive over the tiles of one
// digit), dtot the 256 digit totals of the class
__global__ __launch_bounds__(RX_THREADS) void lovasz_scatter_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ pin,
                                                                    uint32_t* __restrict__ kout, uint32_t* __restrict__ pout,
                                                                    int64_t N, int nblk, int shift, const int* __restrict__ hist,
                                                                    const int* __restrict__ dtot) {
  __shared__ int cnt[RX_WAVES][RX_RADIX];
  __shared__ int ws[RX_WAVES];
  const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // first output position of digit `tid` for this tile = keys of smaller digits + same digit in earlier tiles
  const int tot = dtot[c * RX_RADIX + tid];
#pragma unroll
  for (int q = 0; q < RX_WAVES; ++q) cnt[q][tid] = 0;
  const int dbase = block_incl_scan(tot, ws) - tot + hist[((int64_t)c * RX_RADIX + tid) * nblk + blk];  // its barrier: cnt too

  const uint32_t* ki = kin + (int64_t)c * N;
  const uint32_t* pi = pin + (int64_t)c * N;
  const int64_t base = (int64_t)blk * RX_TILE;
  uint32_t kk[RX_ITEMS], pp[RX_ITEMS];
  int loc[RX_ITEMS];
  // rank inside the wave's 512 keys: the counters cnt[wv][*] are this wave's alone (LDS operations of one wave complete in
  // program order; the fences keep the compiler from moving them across the rounds)
#pragma unroll
  for (int j = 0; j < RX_ITEMS; ++j) {
    const int64_t p = tile_pos(base, wv, j, lane);
    const bool valid = p < N;
    kk[j] = valid ? ki[p] : 0u;
    pp[j] = valid ? pi[p] : 0u;
    const int d = (int)((~kk[j] >> shift) & 255u);
    const uint64_t m = match_digit(d, valid);
    const int prev = cnt[wv][d];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (valid && (m & lanes_below(lane)) == 0) cnt[wv][d] = prev + __popcll(m);
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    loc[j] = prev + __popcll(m & lanes_below(lane));
  }
  __syncthreads();
  {  // cnt[wv][digit]: count -> first output position of the wave's keys of that digit
    int run = dbase;
#pragma unroll
    for (int q = 0; q < RX_WAVES; ++q) {
      const int t = cnt[q][tid];
      cnt[q][tid] = run;
      run += t;
    }
  }
  __syncthreads();
  uint32_t* ko = kout + (int64_t)c * N;
  uint32_t* po = pout + (int64_t)c * N;
#pragma unroll
  for (int j = 0; j < RX_ITEMS; ++j) {
    const int64_t p = tile_pos(base, wv, j, lane);
    if (p < N) {
      const int d = (int)((~kk[j] >> shift) & 255u);
      const int64_t dst = (int64_t)cnt[wv][d] + loc[j];
      ko[dst] = kk[j];
      po[dst] = pp[j];
    }
  }
}

// ftot[c * nblk + tile] = class pixels among the tile's sorted positions
__global__ __launch_bounds__(RX_THREADS) void lovasz_flagtot_kernel(const uint32_t* __restrict__ pay, int64_t N, int nblk,
                                                                    int* __restrict__ ftot) {
  __shared__ int ws[RX_WAVES];
  const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t* pi = pay + (int64_t)c * N;
  const int64_t base = (int64_t)blk * RX_TILE;
  bool f[RX_ITEMS];
#pragma unroll
  for (int j = 0; j < RX_ITEMS; ++j) {
    const int64_t p = tile_pos(base, wv, j, lane);
    f[j] = p < N && (pi[p] >> 31);
  }
  const int n = block_count(f, ws);
  if (tid == 0) ftot[(int64_t)c * nblk + blk] = n;
}

// per sorted position: f_k, g_k; grad[pixel * C + c] = s g_k; part[c * nblk + tile] = sum of e g over the tile (double)
__global__ __launch_bounds__(RX_THREADS) void lovasz_grad_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ pay,
                                                                 int64_t N, int nblk, int C, const int* __restrict__ ftot,
                                                                 const int* __restrict__ gtot, float* __restrict__ grad,
                                                                 double* __restrict__ part, int32_t* __restrict__ dbg_order) {
  __shared__ int ws[RX_WAVES];
  __shared__ double wd[RX_WAVES];
  const int c = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const uint32_t* ki = key + (int64_t)c * N;
  const uint32_t* pi = pay + (int64_t)c * N;
  const int64_t base = (int64_t)blk * RX_TILE;
  uint32_t kk[RX_ITEMS], pp[RX_ITEMS];
  uint64_t fm[RX_ITEMS];
  int wt = 0;
#pragma unroll
  for (int j = 0; j < RX_ITEMS; ++j) {
    const int64_t p = tile_pos(base, wv, j, lane);
    const bool valid = p < N;
    kk[j] = valid ? ki[p] : 0u;
    pp[j] = valid ? pi[p] : 0u;
    fm[j] = __ballot(valid && (pp[j] >> 31));
    wt += __popcll(fm[j]);
  }
  if (lane == 0) ws[wv] = wt;
  __syncthreads();
  int64_t run = ftot[(int64_t)c * nblk + blk];  // class pixels before this wave's first key
#pragma unroll
  for (int q = 0; q < RX_WAVES; ++q)
    if (q < wv) run += ws[q];
  const int64_t G = gtot[c];
  const uint64_t upto = lanes_below(lane) | (1ull << lane);
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < RX_ITEMS; ++j) {
    const int64_t k = tile_pos(base, wv, j, lane);
    if (k < N) {
      const bool f = pp[j] >> 31;
      const int64_t fk = run + __popcll(fm[j] & upto);
      const int64_t I = G - fk, U = G + (k + 1 - fk);
      double g;
      if (G == 0) g = (k == 0) ? 1.0 : 0.0;
      else if (f) g = 1.0 / (double)U;
      else g = (double)I / ((double)U * (double)(U - 1));
      acc += (double)__builtin_bit_cast(float, kk[j]) * g;
      const double s = kk[j] == 0u ? 0.0 : (f ? -1.0 : 1.0);
      const uint32_t pix = pp[j] & 0x7FFFFFFFu;
      grad[(int64_t)pix * C + c] = (float)(s * g);
      if (dbg_order) dbg_order[(int64_t)c * N + k] = (int32_t)pix;
    }
    run += __popcll(fm[j]);
  }
  const double sum = block_sum(acc, wd);
  if (tid == 0) part[(int64_t)c * nblk + blk] = sum;
}

// per_class[c] = sum of the class's tile partials (double, fixed order); loss = mean (reduction 0) or sum (1, 2) of them
__global__ __launch_bounds__(RX_THREADS) void lovasz_finalize_kernel(const double* __restrict__ part, int nblk, int C, int reduction,
                                                                     float* __restrict__ per_class, float* __restrict__ loss) {
  __shared__ double red[RX_THREADS];
  __shared__ double cls[MAXC];
  const int tid = threadIdx.x;
  for (int c = 0; c < C; ++c) {
    double s = 0.0;
    for (int i = tid; i < nblk; i += RX_THREADS) s += part[(int64_t)c * nblk + i];
    const double sum = tree_sum256(s, red);
    if (tid == 0) cls[c] = sum;
    __syncthreads();
  }
  if (tid == 0) {
    double t = 0.0;
    for (int c = 0; c < C; ++c) {
      per_class[c] = (float)cls[c];
      t += cls[c];
    }
    *loss = (float)(reduction == 0 ? t / (double)C : t);
  }
}

// dz[b, y, x, c] (=, or += with `accumulate`) grad_scale * d loss / d (resized logits)
__global__ __launch_bounds__(RX_THREADS) void lovasz_dz_kernel(const float* __restrict__ logits, const float* __restrict__ grad, int h,
                                                               int w, int H, int W, int C, int n_softmax, int64_t N, float rfac,
                                                               float grad_scale, int accumulate, float* __restrict__ dz) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (int64_t)gridDim.x * blockDim.x) {
    float g[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) g[c] = c < C ? grad[i * C + c] * rfac : 0.f;
    if (n_softmax) {
      float q[MAXC];
      sample_logits_at(logits, h, w, H, W, C, i, q);
      softmax_c(q, C);
      softmax_bwd_c(g, q, C);
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < C) {
        const float v = g[c] * grad_scale;
        dz[i * C + c] = accumulate ? dz[i * C + c] + v : v;
      }
  }
}

struct LvScratch {
  int64_t key[2], pay[2], hist, dtot, ftot, gtot, part, grad, bytes;
};
inline LvScratch lv_layout(int64_t N, int C) {
  const int64_t nblk = rx_nblk(N);
  LvScratch s;
  ScratchLayout l;
  s.key[0] = l.take(4 * N * C);
  s.key[1] = l.take(4 * N * C);
  s.pay[0] = l.take(4 * N * C);
  s.pay[1] = l.take(4 * N * C);
  s.hist = l.take(4 * (int64_t)C * RX_RADIX * nblk);
  s.dtot = l.take(4 * (int64_t)C * RX_RADIX);
  s.ftot = l.take(4 * (int64_t)C * nblk);
  s.gtot = l.take(4 * (int64_t)C);
  s.part = l.take(8 * (int64_t)C * nblk);
  s.grad = l.take(4 * N * C);
  s.bytes = l.bytes;
  return s;
}

}  // namespace

extern "C" int asis_lovasz_tile(void) { return RX_TILE; }

extern "C" int64_t asis_lovasz_scratch_bytes(int64_t N, int C) {
  if (N < 1 || N >= ((int64_t)1 << 31) || C < 1 || C > MAXC) {
    asis_set_error_("asis_lovasz_scratch_bytes: need 1 <= N < 2^31 and 1 <= C <= %d", MAXC);
    return ASIS_EINVAL;
  }
  return lv_layout(N, C).bytes;
}

extern "C" int asis_lovasz_softmax(void* stream, const float* logits, const int64_t* target, int B, int h, int w, int H, int W,
                                   int C, int n_softmax, int reduction, float grad_scale, int accumulate, void* scratch,
                                   float* loss, float* per_class, float* dz, float* keys, int32_t* order) {
  ASIS_REQUIRE(logits && target && scratch && loss && per_class && dz, "asis_lovasz_softmax: null pointer");
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "asis_lovasz_softmax: C=%d must be in 1..%d", C, MAXC);
  ASIS_REQUIRE(n_softmax == 0 || n_softmax == 1, "asis_lovasz_softmax: n_softmax must be 0 or 1");
  ASIS_REQUIRE(reduction >= 0 && reduction <= 2, "asis_lovasz_softmax: reduction must be 0 (mean), 1 (sum) or 2 (none)");
  ASIS_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "asis_lovasz_softmax: empty tensor");
  const int64_t N = (int64_t)B * H * W;
  ASIS_REQUIRE(N < ((int64_t)1 << 31), "asis_lovasz_softmax: B*H*W=%lld must be < 2^31 (the payload keeps the pixel index in 31 bits)",
               (long long)N);
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "asis_lovasz_softmax: scratch must be 8-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const LvScratch L = lv_layout(N, C);
  char* base = static_cast<char*>(scratch);
  uint32_t* key[2] = {reinterpret_cast<uint32_t*>(base + L.key[0]), reinterpret_cast<uint32_t*>(base + L.key[1])};
  uint32_t* pay[2] = {reinterpret_cast<uint32_t*>(base + L.pay[0]), reinterpret_cast<uint32_t*>(base + L.pay[1])};
  int* hist = reinterpret_cast<int*>(base + L.hist);
  int* dtot = reinterpret_cast<int*>(base + L.dtot);
  int* ftot = reinterpret_cast<int*>(base + L.ftot);
  int* gtot = reinterpret_cast<int*>(base + L.gtot);
  double* part = reinterpret_cast<double*>(base + L.part);
  float* grad = reinterpret_cast<float*>(base + L.grad);
  const int nblk = (int)rx_nblk(N);
  const dim3 tiles(nblk, C), blk(RX_THREADS);
  const int pgrid = asis_grid(N, RX_THREADS, 8192);

  hipLaunchKernelGGL(lovasz_keys_kernel, dim3(pgrid), blk, 0, s, logits, target, h, w, H, W, C, n_softmax, N, key[0], pay[0], keys);
  for (int pass = 0; pass < 4; ++pass) {  // four passes: the sorted order ends in buffer 0
    const int in = pass & 1, out = in ^ 1, shift = 8 * pass;
    hipLaunchKernelGGL(lovasz_hist_kernel, tiles, blk, 0, s, key[in], N, nblk, shift, hist);
    hipLaunchKernelGGL(lovasz_rowscan_kernel, dim3(C * RX_RADIX), blk, 0, s, hist, nblk, dtot);
    hipLaunchKernelGGL(lovasz_scatter_kernel, tiles, blk, 0, s, key[in], pay[in], key[out], pay[out], N, nblk, shift, hist, dtot);
  }
  hipLaunchKernelGGL(lovasz_flagtot_kernel, tiles, blk, 0, s, pay[0], N, nblk, ftot);
  hipLaunchKernelGGL(lovasz_rowscan_kernel, dim3(C), blk, 0, s, ftot, nblk, gtot);
  hipLaunchKernelGGL(lovasz_grad_kernel, tiles, blk, 0, s, key[0], pay[0], N, nblk, C, ftot, gtot, grad, part, order);
  hipLaunchKernelGGL(lovasz_finalize_kernel, dim3(1), blk, 0, s, part, nblk, C, reduction, per_class, loss);
  hipLaunchKernelGGL(lovasz_dz_kernel, dim3(pgrid), blk, 0, s, logits, grad, h, w, H, W, C, n_softmax, N,
                     reduction == 0 ? 1.f / (float)C : 1.f, grad_scale, accumulate, dz);
  ASIS_CHECK_LAUNCH("asis_lovasz_softmax");
  return ASIS_OK;
}
