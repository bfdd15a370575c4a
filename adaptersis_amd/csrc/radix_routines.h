// Wave and workgroup routines of the radix kernels: the LSD sort of lovasz.hip, the MSB select of hardpixel.hip and the pick
// step of surface.hip's segmented select (pct_*).  One definition of each, so the three files rank, scan and reduce alike.
// A workgroup is RX_THREADS = 256 threads = RX_WAVES wave64s, a digit has 8 bits (RX_RADIX = one digit per thread) and a tile
// is RX_ITEMS keys per thread.  Where a key of a tile sits is the caller's business (lovasz.hip is wave-striped, hardpixel.hip
// thread-striped), and so is the direction of a scan over the digits.  Every routine that takes `ws` / `wd` / `red` wants that
// many entries of LDS, must be called by all 256 threads, and holds the barrier(s) its comment names.
#pragma once
#include "asis_common.h"

namespace {

constexpr int RX_THREADS = 256, RX_WAVES = 4, RX_ITEMS = 8, RX_TILE = RX_THREADS * RX_ITEMS, RX_RADIX = 256;

__device__ __forceinline__ uint64_t lanes_below(int lane) { return (1ull << lane) - 1ull; }
// the valid lanes of the wave that hold digit d (all 64 lanes call it): 8 wave64 ballots, one per digit bit
__device__ __forceinline__ uint64_t match_digit(int d, bool valid) {
  uint64_t m = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (d >> b) & 1;
    const uint64_t bm = __ballot(bit);
    m &= bit ? bm : ~bm;
  }
  return m;
}
// add the digits of up to 64 keys of one wave round into the workgroup's LDS histogram hs[RX_RADIX]: the first lane of each
// digit adds the popcount, so keys that crowd into a few digits do not serialise the LDS atomics on one address
__device__ __forceinline__ void count_digit(int* hs, int d, bool valid, int lane) {
  const uint64_t m = match_digit(d, valid);
  if (valid && (m & lanes_below(lane)) == 0) atomicAdd(&hs[d], __popcll(m));  // integer: order-independent
}
__device__ __forceinline__ int wave_incl_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// inclusive scan of one counter per thread in thread order; ws[RX_WAVES] keeps the four wave totals.  One barrier, between the
// caller's code before and after the call; a second call with the same ws needs a barrier of the caller's in between.
__device__ __forceinline__ int block_incl_scan(int v, int* ws) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int incl = wave_incl_scan(v, lane);
  if (lane == 63) ws[wv] = incl;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < RX_WAVES; ++q)
    if (q < wv) incl += ws[q];
  return incl;
}
// after block_incl_scan over bins: does this thread's bin (cnt keys, incl up to and including it) hold the key of 0-based
// `rank` in scan order?  True in exactly one thread when rank < the sum of all bins.
__device__ __forceinline__ bool bin_holds_rank(uint32_t incl, uint32_t cnt, uint32_t rank) {
  return incl - cnt <= rank && rank < incl;
}

// exclusive scan of row[0..n) in place by one workgroup, any n: RX_TILE entries a pass (8 consecutive ones per thread), the
// passes chained by a carry.  -> the row's sum, in every thread.
__device__ __forceinline__ int block_rowscan(int* __restrict__ row, int n, int* ws) {
  const int tid = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < n; base += RX_TILE) {
    const int i0 = base + tid * RX_ITEMS;
    int v[RX_ITEMS], s = 0;
#pragma unroll
    for (int j = 0; j < RX_ITEMS; ++j) {
      v[j] = (i0 + j < n) ? row[i0 + j] : 0;
      s += v[j];
    }
    int run = carry + block_incl_scan(s, ws) - s;
#pragma unroll
    for (int j = 0; j < RX_ITEMS; ++j) {
      if (i0 + j < n) row[i0 + j] = run;
      run += v[j];
    }
    carry += (ws[0] + ws[1]) + (ws[2] + ws[3]);
    __syncthreads();  // ws is written again by the next pass
  }
  return carry;
}

// number of set flags over the workgroup's tile, flag[j] this thread's of round j (any position rule).  One barrier.
__device__ __forceinline__ int block_count(const bool (&flag)[RX_ITEMS], int* ws) {
  int n = 0;
#pragma unroll
  for (int j = 0; j < RX_ITEMS; ++j) n += __popcll(__ballot(flag[j]));
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = n;
  __syncthreads();
  return (ws[0] + ws[1]) + (ws[2] + ws[3]);
}
// sum of one double per thread in a fixed order: xor tree over the wave, then (w0 + w1) + (w2 + w3).  One barrier.
__device__ __forceinline__ double block_sum(double acc, double* wd) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) wd[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (wd[0] + wd[1]) + (wd[2] + wd[3]);
}
// sum of one double per thread by a binary tree over red[RX_THREADS] (fixed order).  red[0] is read after the last barrier:
// a caller that sums again puts one of its own before the next call.
__device__ __forceinline__ double tree_sum256(double s, double* red) {
  const int tid = threadIdx.x;
  red[tid] = s;
  __syncthreads();
  for (int o = RX_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}

// ---- host side: the caller-owned scratch as consecutive buffers, each on a 256-byte boundary ----
struct ScratchLayout {
  int64_t bytes = 0;
  int64_t take(int64_t b) {
    const int64_t at = bytes;
    bytes += (b + 255) / 256 * 256;
    return at;
  }
};
inline int64_t rx_nblk(int64_t N) { return (N + RX_TILE - 1) / RX_TILE; }

}  // namespace
