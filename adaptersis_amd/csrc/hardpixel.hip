// Hard-pixel losses: the top-k cross entropy (segloss/ND_Crossentropy.py:34-47 TopKLoss) and the focal loss
// (segloss/focal_loss.py:7-91), fused with the bilinear resize of the logits like the losses of loss.hip and lovasz.hip.
//
//     z   = resize(logits) at the target's H x W, t = target[i], i = (b*H + y)*W + x the flat pixel index, N = B*H*W
//     kind 0 (cross entropy, n_softmax = 0):   v_i = w[t] (logsumexp(z) - z_t)                      w = class_weight or 1
//     kind 1 (focal): q = z (n_softmax 0) or softmax(z) (1); o = onehot(t), clamped to [smooth/(C-1), 1-smooth] if smooth > 0;
//                     pt = sum_c o_c q_c + smooth;  v_i = -w[t] max(1 - pt, 0)^gamma log(pt)          w = alpha
//     a label outside 0..C-1: v_i = 0 and no gradient; the pixel still counts in N
//     loss = (sum of the K largest v_i) / K        (size_average = 0: the plain sum)
//
// Order of the selection: by value, through an order-preserving map of the fp32 bits to uint32 (-0 taken as +0; a NaN is
// ordered by its bits), ties by ascending pixel index.  K = N: everything is selected and the select stages are not launched.
//
// Nothing is sorted and nothing is scattered: an MSB radix SELECT over one float per pixel.
// Stages (every launch ordered by the stream; NO workgroup waits on another; nothing is read back by the host):
//   values   one pass over the pixels: taps -> v_i, stored once (4 B per pixel), and the histogram of the top byte of the keys
//   pick     one workgroup: the digit bucket that holds the K-th largest key -> prefix, remaining count (device memory)
//   hist     x 3: histogram of the next byte over the keys that match the prefix so far, each followed by a pick.
//            Afterwards T = the key of the K-th largest value and r = K - #(key > T), 1 <= r <= #(key == T)
//   ties     #(key == T) per tile -> exclusive scan over the tiles (one workgroup, any number of tiles)
//   apply    per tile: rank of every key == T by ballots (pixel order), selected = key > T or (key == T and rank < r);
//            the tile's sum of the selected values in double in a fixed order; dz from the logits again (the softmax is
//            recomputed as in lovasz_dz_kernel: no [N][C] buffer), exactly 0 on unselected pixels (untouched with accumulate)
//   finalize the tile sums in double in a fixed order -> loss
//
// Histograms: per workgroup in LDS, 256 counters, one digit per thread when they are flushed, filled by count_digit of
// radix_routines.h (which also holds the scans, the reductions and the tile constants RX_*): cross-entropy values crowd into
// a few top bytes, and it keeps the LDS atomics off one address.  The workgroup's counters are then added to the 256
// global ones with integer atomics: integer sums do not depend on the order, so the result is bit-identical between calls.
// Every floating-point sum has a fixed order (thread: items in order; wave: xor tree; workgroup: 4 waves; tiles: finalize).
// Tile: 256 threads x 8 values = 2048, position = tile*2048 + item*256 + thread (coalesced, and ascending in (item, wave, lane)).
#include "asis_common.h"
#include "bilinear_tap.h"  // MAXC, sample_logits_at, softmax_c, softmax_bwd_c
#include "radix_routines.h"

namespace {

constexpr int HP_HIST_BLOCKS = 1024;  // workgroups of a histogram pass (each loops over tiles): bounds the global atomics

struct HpCfg {
  int h, w, H, W, C, kind, n_softmax;
  float gamma, smooth, o_hit, o_miss;  // the (clamped) one-hot row: o_hit at the label, o_miss elsewhere
};

// order-preserving map fp32 -> uint32 (larger value = larger key), -0 == +0
__device__ __forceinline__ uint32_t hp_key(float v) {
  uint32_t b = __builtin_bit_cast(uint32_t, v);
  if (b == 0x80000000u) b = 0u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// v_i of pixel i; with `g` also d v_i / d z (through the clamped one-hot and, n_softmax = 1, the softmax transpose)
__device__ __forceinline__ float hp_pixel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                          const float* __restrict__ cw, const HpCfg& k, int64_t i, float* g) {
  const int64_t t = target[i];
  if (t < 0 || t >= k.C) {
    if (g) {
#pragma unroll
      for (int c = 0; c < MAXC; ++c) g[c] = 0.f;
    }
    return 0.f;
  }
  float z[MAXC];
  sample_logits_at(logits, k.h, k.w, k.H, k.W, k.C, i, z);
  const float wt = cw ? cw[t] : 1.f;
  if (k.kind == 0) {
    float m = -INFINITY, zt = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < k.C) {
        m = fmaxf(m, z[c]);
        if (c == (int)t) zt = z[c];
      }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < k.C) se += expf(z[c] - m);
    if (g) {  // w (softmax(z) - onehot), the softmax as everywhere else in the loss kernels
      softmax_c(z, k.C);
#pragma unroll
      for (int c = 0; c < MAXC; ++c) g[c] = c < k.C ? wt * (z[c] - (c == (int)t ? 1.f : 0.f)) : 0.f;
    }
    return wt * (logf(se) - (zt - m));
  }
  if (k.n_softmax) softmax_c(z, k.C);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < k.C) s += (c == (int)t ? k.o_hit : k.o_miss) * z[c];
  const float pt = s + k.smooth;
  const float base = fmaxf(1.f - pt, 0.f);
  const float pw = k.gamma == 0.f ? 1.f : powf(base, k.gamma);
  const float lg = logf(pt);
  if (g) {
    // d/d pt of -w f(1 - pt) log(pt), f(b) = b^gamma; f' = 0 where gamma = 0 or the clamp at 0 holds
    const float dpw = (k.gamma == 0.f || base <= 0.f) ? 0.f : k.gamma * powf(base, k.gamma - 1.f);
    const float dpt = wt * (dpw * lg - pw / pt);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) g[c] = c < k.C ? dpt * (c == (int)t ? k.o_hit : k.o_miss) : 0.f;
    if (k.n_softmax) softmax_bwd_c(g, z, k.C);
  }
  return (-wt * pw) * lg;
}

// vals[i] = v_i (and `values`, optional); with `hist` the histogram of the top byte of the keys (pass 0 of the select)
__global__ __launch_bounds__(RX_THREADS) void hardpixel_values_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                      const float* __restrict__ cw, HpCfg k, int64_t N, int nblk,
                                                                      float* __restrict__ vals, float* __restrict__ values,
                                                                      int* __restrict__ hist) {
  __shared__ int hs[RX_RADIX];
  const int tid = threadIdx.x, lane = tid & 63;
  hs[tid] = 0;
  __syncthreads();
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t base = (int64_t)blk * RX_TILE;
#pragma unroll 1
    for (int j = 0; j < RX_ITEMS; ++j) {
      const int64_t i = base + j * RX_THREADS + tid;
      const bool valid = i < N;
      float v = 0.f;
      if (valid) {
        v = hp_pixel(logits, target, cw, k, i, nullptr);
        vals[i] = v;
        if (values) values[i] = v;
      }
      if (hist) count_digit(hs, (int)(hp_key(v) >> 24), valid, lane);
    }
  }
  if (hist) {
    __syncthreads();
    if (hs[tid]) atomicAdd(&hist[tid], hs[tid]);
  }
}

// pass 1..3: histogram of byte (3 - pass) over the keys whose bytes above it equal the prefix in state[0]
__global__ __launch_bounds__(RX_THREADS) void hardpixel_hist_kernel(const float* __restrict__ vals, int64_t N, int nblk, int pass,
                                                                    const uint32_t* __restrict__ state, int* __restrict__ hist) {
  __shared__ int hs[RX_RADIX];
  const int tid = threadIdx.x, lane = tid & 63;
  hs[tid] = 0;
  __syncthreads();
  const int up = 32 - 8 * pass, shift = 24 - 8 * pass;
  const uint32_t prefix = state[0] >> up;
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t base = (int64_t)blk * RX_TILE;
#pragma unroll
    for (int j = 0; j < RX_ITEMS; ++j) {
      const int64_t i = base + j * RX_THREADS + tid;
      const uint32_t key = i < N ? hp_key(vals[i]) : 0u;
      const bool valid = i < N && (key >> up) == prefix;
      count_digit(hs, (int)((key >> shift) & 255u), valid, lane);
    }
  }
  __syncthreads();
  if (hs[tid]) atomicAdd(&hist[pass * RX_RADIX + tid], hs[tid]);
}

// one workgroup: among the keys counted in hist[pass] the rem-th largest lies in digit d: state[0] |= d << shift, state[1] = rem
// minus the keys in larger digits.  rem is K before pass 0.  Thread i looks at digit 255 - i: the scan runs from the top.
__global__ __launch_bounds__(RX_THREADS) void hardpixel_pick_kernel(const int* __restrict__ hist, int pass, uint32_t K,
                                                                    uint32_t* __restrict__ state) {
  __shared__ int ws[RX_WAVES];
  const int d = RX_RADIX - 1 - threadIdx.x;
  const int cnt = hist[pass * RX_RADIX + d];
  const uint32_t rem = pass == 0 ? K : state[1], prefix = pass == 0 ? 0u : state[0];
  const int incl = block_incl_scan(cnt, ws);
  if (bin_holds_rank(incl, cnt, rem - 1)) {  // exactly one thread: the counts sum to >= rem
    state[0] = prefix | ((uint32_t)d << (24 - 8 * pass));
    state[1] = rem - (uint32_t)(incl - cnt);  // minus the keys in larger digits
  }
}

// bcnt[tile] = #(key == T) in the tile
__global__ __launch_bounds__(RX_THREADS) void hardpixel_ties_kernel(const float* __restrict__ vals, int64_t N,
                                                                    const uint32_t* __restrict__ state, int* __restrict__ bcnt) {
  __shared__ int ws[RX_WAVES];
  const int blk = blockIdx.x, tid = threadIdx.x;
  const uint32_t T = state[0];
  const int64_t base = (int64_t)blk * RX_TILE;
  bool tie[RX_ITEMS];
#pragma unroll
  for (int j = 0; j < RX_ITEMS; ++j) {
    const int64_t i = base + j * RX_THREADS + tid;
    tie[j] = i < N && hp_key(vals[i]) == T;
  }
  const int n = block_count(tie, ws);
  if (tid == 0) bcnt[blk] = n;
}

// n ints, one workgroup: exclusive scan in place.  Any n.
__global__ __launch_bounds__(RX_THREADS) void hardpixel_scan_kernel(int* __restrict__ row, int n) {
  __shared__ int ws[RX_WAVES];
  block_rowscan(row, n, ws);
}

// the selection, the tile's sum of the selected values, dz.  `state` == nullptr: every pixel is selected (K = N).
__global__ __launch_bounds__(RX_THREADS) void hardpixel_apply_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                                     const float* __restrict__ cw, HpCfg k, int64_t N,
                                                                     const float* __restrict__ vals, const uint32_t* __restrict__ state,
                                                                     const int* __restrict__ bcnt, float inv_k, float grad_scale,
                                                                     int accumulate, double* __restrict__ part, float* __restrict__ dz,
                                                                     uint8_t* __restrict__ selected) {
  __shared__ int wc[RX_ITEMS][RX_WAVES];
  __shared__ double wd[RX_WAVES];
  const int blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t base = (int64_t)blk * RX_TILE;
  const bool all = state == nullptr;
  const uint32_t T = all ? 0u : state[0], r = all ? 0u : state[1];
#pragma unroll
  for (int j = 0; j < RX_ITEMS; ++j) {
    const int64_t i = base + j * RX_THREADS + tid;
    const uint64_t em = __ballot(!all && i < N && hp_key(vals[i]) == T);
    if (lane == 0) wc[j][wv] = __popcll(em);
  }
  __syncthreads();
  uint32_t run = all ? 0u : (uint32_t)bcnt[blk];  // keys == T before this tile, then before round j
  double acc = 0.0;
  // one round at a time (the pixel function is large: not unrolled); the values come from the cache the second time
#pragma unroll 1
  for (int j = 0; j < RX_ITEMS; ++j) {
    const int64_t i = base + j * RX_THREADS + tid;
    const float v = i < N ? vals[i] : 0.f;
    const uint32_t key = hp_key(v);
    const uint64_t em = __ballot(!all && i < N && key == T);
    uint32_t rank = run + (uint32_t)__popcll(em & lanes_below(lane));
#pragma unroll
    for (int q = 0; q < RX_WAVES; ++q) {
      if (q < wv) rank += (uint32_t)wc[j][q];
      run += (uint32_t)wc[j][q];
    }
    if (i < N) {
      const bool sel = all || key > T || (key == T && rank < r);
      if (selected) selected[i] = sel ? 1 : 0;
      if (sel) {
        acc += (double)v;
        float g[MAXC];
        hp_pixel(logits, target, cw, k, i, g);
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < k.C) {
            const float d = __fmul_rn(__fmul_rn(g[c], inv_k), grad_scale);  // no contraction: grad_scale 2^n scales the bits
            dz[i * k.C + c] = accumulate ? __fadd_rn(dz[i * k.C + c], d) : d;
          }
      } else if (!accumulate) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < k.C) dz[i * k.C + c] = 0.f;
      }
    }
  }
  const double sum = block_sum(acc, wd);
  if (tid == 0) part[blk] = sum;
}

// loss = sum of the tile partials (double, fixed order) * scale
__global__ __launch_bounds__(RX_THREADS) void hardpixel_finalize_kernel(const double* __restrict__ part, int nblk, double scale,
                                                                        float* __restrict__ loss) {
  __shared__ double red[RX_THREADS];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int i = tid; i < nblk; i += RX_THREADS) s += part[i];
  const double sum = tree_sum256(s, red);
  if (tid == 0) *loss = (float)(sum * scale);
}

struct HpScratch {
  int64_t vals, hist, state, bcnt, part, bytes;
};
inline HpScratch hp_layout(int64_t N) {
  const int64_t nblk = rx_nblk(N);
  HpScratch s;
  ScratchLayout l;
  s.vals = l.take(4 * N);
  s.hist = l.take(4 * 4 * RX_RADIX);  // hist and state are zeroed by one memset: keep them adjacent
  s.state = l.take(16);
  s.bcnt = l.take(4 * nblk);
  s.part = l.take(8 * nblk);
  s.bytes = l.bytes;
  return s;
}

}  // namespace

extern "C" int asis_hardpixel_tile(void) { return RX_TILE; }

extern "C" int64_t asis_hardpixel_scratch_bytes(int64_t N) {
  if (N < 1 || N >= ((int64_t)1 << 31)) {
    asis_set_error_("asis_hardpixel_scratch_bytes: need 1 <= N < 2^31");
    return ASIS_EINVAL;
  }
  return hp_layout(N).bytes;
}

extern "C" int asis_hardpixel_loss(void* stream, const float* logits, const int64_t* target, const float* class_weight, int B, int h,
                                   int w, int H, int W, int C, int kind, int n_softmax, float gamma, float smooth, int64_t K,
                                   int size_average, float grad_scale, int accumulate, void* scratch, float* loss, float* dz,
                                   float* values, uint8_t* selected) {
  ASIS_REQUIRE(logits && target && scratch && loss && dz, "asis_hardpixel_loss: null pointer");
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "asis_hardpixel_loss: C=%d must be in 1..%d", C, MAXC);
  ASIS_REQUIRE(kind == 0 || kind == 1, "asis_hardpixel_loss: kind must be 0 (cross entropy) or 1 (focal)");
  ASIS_REQUIRE(n_softmax == 0 || (n_softmax == 1 && kind == 1),
               "asis_hardpixel_loss: n_softmax must be 0, or 1 with kind 1 (the cross entropy takes logits without a nonlinearity)");
  ASIS_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "asis_hardpixel_loss: empty tensor");
  const int64_t N = (int64_t)B * H * W;
  ASIS_REQUIRE(N < ((int64_t)1 << 31), "asis_hardpixel_loss: B*H*W=%lld must be < 2^31", (long long)N);
  ASIS_REQUIRE(K >= 1 && K <= N, "asis_hardpixel_loss: K=%lld must be in 1..B*H*W=%lld", (long long)K, (long long)N);
  if (kind == 1) {
    ASIS_REQUIRE(smooth >= 0.f && smooth <= 1.f, "asis_hardpixel_loss: smooth value should be in [0,1]");
    ASIS_REQUIRE(smooth == 0.f || C >= 2, "asis_hardpixel_loss: smooth > 0 needs C >= 2 (the one-hot row is clamped at smooth/(C-1))");
    ASIS_REQUIRE(gamma >= 0.f, "asis_hardpixel_loss: gamma must be >= 0");
  }
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(scratch) & 7) == 0, "asis_hardpixel_loss: scratch must be 8-byte aligned");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const HpScratch L = hp_layout(N);
  char* base = static_cast<char*>(scratch);
  float* vals = reinterpret_cast<float*>(base + L.vals);
  int* hist = reinterpret_cast<int*>(base + L.hist);
  uint32_t* state = reinterpret_cast<uint32_t*>(base + L.state);
  int* bcnt = reinterpret_cast<int*>(base + L.bcnt);
  double* part = reinterpret_cast<double*>(base + L.part);
  const int nblk = (int)rx_nblk(N);
  const dim3 blk(RX_THREADS), hgrid(nblk < HP_HIST_BLOCKS ? nblk : HP_HIST_BLOCKS);

  HpCfg k;
  k.h = h, k.w = w, k.H = H, k.W = W, k.C = C, k.kind = kind, k.n_softmax = n_softmax;
  k.gamma = gamma, k.smooth = kind == 1 ? smooth : 0.f;
  k.o_hit = 1.f, k.o_miss = 0.f;
  if (kind == 1 && smooth > 0.f) {  // torch.clamp(onehot, lo, hi) = min(max(x, lo), hi)
    const float lo = smooth / (float)(C - 1), hi = 1.f - smooth;
    k.o_hit = fminf(fmaxf(1.f, lo), hi);
    k.o_miss = fminf(fmaxf(0.f, lo), hi);
  }
  const bool all = K == N;
  if (!all) {
    const hipError_t e = hipMemsetAsync(base + L.hist, 0, (size_t)(L.bcnt - L.hist), s);
    if (e != hipSuccess) ASIS_FAIL(ASIS_ELAUNCH, "asis_hardpixel_loss: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(hardpixel_values_kernel, all ? dim3(asis_grid(nblk, 1, 8192)) : hgrid, blk, 0, s, logits, target, class_weight, k,
                     N, nblk, vals, values, all ? nullptr : hist);
  if (!all) {
    hipLaunchKernelGGL(hardpixel_pick_kernel, dim3(1), blk, 0, s, hist, 0, (uint32_t)K, state);
    for (int pass = 1; pass < 4; ++pass) {
      hipLaunchKernelGGL(hardpixel_hist_kernel, hgrid, blk, 0, s, vals, N, nblk, pass, state, hist);
      hipLaunchKernelGGL(hardpixel_pick_kernel, dim3(1), blk, 0, s, hist, pass, (uint32_t)K, state);
    }
    hipLaunchKernelGGL(hardpixel_ties_kernel, dim3(nblk), blk, 0, s, vals, N, state, bcnt);
    hipLaunchKernelGGL(hardpixel_scan_kernel, dim3(1), blk, 0, s, bcnt, nblk);
  }
  const float inv_k = size_average ? (float)(1.0 / (double)K) : 1.f;
  hipLaunchKernelGGL(hardpixel_apply_kernel, dim3(nblk), blk, 0, s, logits, target, class_weight, k, N, vals,
                     all ? nullptr : state, bcnt, inv_k, grad_scale, accumulate, part, dz, selected);
  hipLaunchKernelGGL(hardpixel_finalize_kernel, dim3(1), blk, 0, s, part, nblk, size_average ? 1.0 / (double)K : 1.0, loss);
  ASIS_CHECK_LAUNCH("asis_hardpixel_loss");
  return ASIS_OK;
}
