// Boundary metrics of a prediction against its ground truth: the exact squared Euclidean distance transform of the class
// boundaries at native size, evaluated where the metrics need it, and the per (frame, class) statistics behind Dice, the
// normalised surface distance, Hausdorff and the mean surface distance (definitions: include/asis_hip.h).
//
//   P = (pred_lut[pred] == c), G = (lut[target] == c); a table value >= C belongs to no class.
//   E(M) = M and not erode(M, 4-neighbour cross, outside = background): the mask pixels on the image border or with a
//          4-neighbour outside the mask.  A pixel has one class, so the edge pixels of ALL classes of a side are one uint8 map
//          (class of the edge pixel, 255 elsewhere).
//   d2_G(y, x) = min over E(G) of (y - y')^2 + (x - x')^2, an exact integer: the transform separates into
//          g(y, x') = |y - nearest edge pixel of column x'| and d2 = min over x' of (x - x')^2 + g(y, x')^2.
//
//   surface_edges_kernel   one thread per pixel, both sides: the two edge maps and inter / n_pred / n_lab / e_pred / e_lab
//                          (LDS atomics per wave, one 64-bit atomic add per non-zero entry per block, as predict_mask_kernel).
//   surface_column_kernel  one thread per column of one (frame, side, class): a downward and an upward sweep write g as uint16
//                          (65535 = no edge pixel in the column; a distance is at most 16383).  A (frame, side, class) without
//                          edge pixels is skipped: its g is never read.
//   surface_row_kernel     one block per (row, frame, side).  The metrics need d2 only at the OTHER side's edge pixels, a few
//                          thousand of two million, and there the minimum is usually a few pixels: the search walks outwards
//                          from x' = x and stops once (x - x')^2 reaches the best value so far, which is exact (every x' left
//                          out has (x - x')^2 >= the minimum found).  Hits and maxima: LDS atomics, then one 64-bit atomic per
//                          non-zero entry per block: integers, independent of the order.  Distances: sqrt of the exact integer
//                          in float64 (correctly rounded; this file is built without fast-math), summed in a FIXED order: per
//                          chunk of 256 pixels thread c adds the values of class c in x order, one partial per (frame, side,
//                          class, row), then surface_sum_kernel adds the rows (strided, then a fixed tree).  No float atomics.
//   surface_field_kernel   testing: the whole field of one side, int32 [B, C, H, W], by the same search from every pixel.
//   pct_*_kernel           asis_surface_quantiles: the order statistics behind the percentile Hausdorff distance, a segmented
//                          radix select over the distances at the edge pixels (described above the kernels); its workspace is
//                          dq int32 [B][2][H][W] (16.6 MB per 1080 x 1920 frame) beside the three buffers below.
//
// Intermediate storage (the caller's workspace; ops.surface_stats chunks over frames and classes to bound it):
//   edges   uint8  [B][2][H][W]            at 1080 x 1920:          4.1 MB per frame
//   g       uint16 [B][2][nc][H][W]        at 1080 x 1920, nc = 8: 66.4 MB per frame (8.3 MB per class)
//   partial double [B][2][nc][H]                                    0.14 MB per frame
// = 70.6 MB per frame at 1080 x 1920, C = 8 (847 MB for a batch of 12, 1.6 GiB at C = 16: hence the chunking, which keeps g
// under 512 MiB whenever one class of one frame fits).
#include "asis_common.h"
#include "radix_routines.h"  // block_incl_scan, bin_holds_rank (pct_pick)

namespace {

constexpr int MAXC = 16;          // classes (predict.hip's bound)
constexpr int NOCLS = 255;       // edge-map value of a pixel that is no edge pixel
constexpr int GINF = 65535;       // g of a column without an edge pixel of the class
constexpr int MAXT = 8;           // tolerances
constexpr int MAXHW = 16384;
// g <= MAXHW - 1 fits 16 bits below GINF; d2 <= 2 (MAXHW - 1)^2 = 5.4e8 fits int32, and so does every candidate of the search
static_assert(MAXHW - 1 < GINF, "vertical distances must fit uint16 below the sentinel");
static_assert(2ll * (MAXHW - 1) * (MAXHW - 1) < 2147483647ll, "squared distances must fit int32");
static_assert(MAXC <= 16, "one LDS row of statistics per class");

struct Thr { int t[MAXT]; };

__device__ __forceinline__ int cls_of(const uint8_t* s_lut, uint8_t raw, int C) {
  const int v = s_lut[raw];
  return v < C ? v : NOCLS;
}

// pred, target uint8 [B,H,W] -> edges uint8 [B][2][H][W]; ints[b][c][0..4] += inter, n_pred, n_lab, e_pred, e_lab
__global__ __launch_bounds__(256) void surface_edges_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ target,
                                                            const uint8_t* __restrict__ plut, const uint8_t* __restrict__ glut,
                                                            int H, int W, int C, int ncol, uint8_t* __restrict__ edges,
                                                            unsigned long long* __restrict__ ints) {
  __shared__ uint8_t s_lut[2][256];
  __shared__ int s_cnt[4][MAXC * 5];
  const int tid = threadIdx.x;
  s_lut[0][tid] = plut[tid];
  s_lut[1][tid] = glut[tid];
  for (int i = tid; i < 4 * MAXC * 5; i += 256) (&s_cnt[0][0])[i] = 0;
  __syncthreads();
  const int b = blockIdx.y;
  const int64_t hw = (int64_t)H * W;
  const int64_t t = (int64_t)blockIdx.x * 256 + tid;
  if (t < hw) {
    const int y = (int)(t / W), x = (int)(t - (int64_t)y * W);
    const bool border = y == 0 || x == 0 || y == H - 1 || x == W - 1;
    int* cnt = s_cnt[tid >> 6];
    int cls[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const uint8_t* m = (s == 0 ? pred : target) + (int64_t)b * hw + t;
      const uint8_t* l = s_lut[s];
      const int c = cls_of(l, m[0], C);
      cls[s] = c;
      int e = NOCLS;
      if (c != NOCLS) {
        // every neighbour inside the image (no border) must be of the class for the pixel to survive the erosion
        const bool edge = border || cls_of(l, m[-W], C) != c || cls_of(l, m[W], C) != c || cls_of(l, m[-1], C) != c ||
                          cls_of(l, m[1], C) != c;
        if (edge) e = c;
        atomicAdd(&cnt[c * 5 + 1 + s], 1);
        if (edge) atomicAdd(&cnt[c * 5 + 3 + s], 1);
      }
      edges[((int64_t)b * 2 + s) * hw + t] = (uint8_t)e;
    }
    if (cls[0] != NOCLS && cls[0] == cls[1]) atomicAdd(&cnt[cls[0] * 5], 1);
  }
  __syncthreads();
  if (tid < C * 5) {
    const int n = (s_cnt[0][tid] + s_cnt[1][tid]) + (s_cnt[2][tid] + s_cnt[3][tid]);
    if (n) atomicAdd(&ints[((int64_t)b * C + tid / 5) * ncol + tid % 5], (unsigned long long)n);
  }
}

// edges -> g uint16 [B][2][nc][H][W] for the classes c0 .. c0 + nc - 1; grid (ceil(W / 256), nc, B * 2)
__global__ __launch_bounds__(256) void surface_column_kernel(const uint8_t* __restrict__ edges, int H, int W, int C, int c0, int nc,
                                                             int ncol, const unsigned long long* __restrict__ ints,
                                                             uint16_t* __restrict__ g) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int c = c0 + blockIdx.y, bs = blockIdx.z, b = bs >> 1, s = bs & 1;
  if (ints[((int64_t)b * C + c) * ncol + 3 + s] == 0) return;   // no edge pixel of the class on this side: g is never read
  if (x >= W) return;
  const int64_t hw = (int64_t)H * W;
  const uint8_t* e = edges + (int64_t)bs * hw + x;
  uint16_t* gc = g + ((int64_t)bs * nc + blockIdx.y) * hw + x;
  int last = -1;
#pragma unroll 8
  for (int y = 0; y < H; ++y) {
    if (e[(int64_t)y * W] == c) last = y;
    gc[(int64_t)y * W] = (uint16_t)(last < 0 ? GINF : y - last);
  }
  last = -1;
#pragma unroll 8
  for (int y = H - 1; y >= 0; --y) {
    if (e[(int64_t)y * W] == c) last = y;
    if (last >= 0 && last - y < (int)gc[(int64_t)y * W]) gc[(int64_t)y * W] = (uint16_t)(last - y);
  }
}

// min over x' of (x - x')^2 + g[x']^2 along one row of g, walking outwards from x.  The row holds at least one finite entry
// whenever the class has an edge pixel on that side, so the result is finite; INT_MAX otherwise.
__device__ __forceinline__ int row_min(const uint16_t* __restrict__ g, int x, int W) {
  int best = 2147483647;
  const int v = g[x];
  if (v != GINF) best = v * v;
  for (int d = 1; d < MAXHW; d += 4) {
    if (d * d >= best) break;                   // every x' from here on has (x - x')^2 >= best
    if (x - d < 0 && x + d >= W) break;         // the row is exhausted on both sides
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int dd = d + u, l = x - dd, r = x + dd;
      const int vl = l >= 0 ? (int)g[l] : GINF, vr = r < W ? (int)g[r] : GINF;
      const int m = min(vl, vr);
      if (m != GINF) best = min(best, dd * dd + m * m);
    }
  }
  return best;
}

// statistics at the edge pixels of side s against the field of the other side; grid (H, B, 2), 256 threads
__global__ __launch_bounds__(256) void surface_row_kernel(const uint8_t* __restrict__ edges, const uint16_t* __restrict__ g, int H,
                                                          int W, int C, int c0, int nc, int ncol, int T, Thr thr,
                                                          unsigned long long* __restrict__ ints, double* __restrict__ partial) {
  __shared__ int s_hit[MAXC * MAXT], s_max[MAXC];
  __shared__ double s_val[256];
  __shared__ uint8_t s_cls[256];
  const int tid = threadIdx.x, y = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
  const int64_t hw = (int64_t)H * W;
  if (tid < MAXC * MAXT) s_hit[tid] = 0;
  if (tid < MAXC) s_max[tid] = 0;
  __syncthreads();
  const uint8_t* q = edges + ((int64_t)b * 2 + s) * hw + (int64_t)y * W;            // query pixels: this side's edge map
  const uint16_t* gf = g + ((int64_t)b * 2 + (1 - s)) * nc * hw + (int64_t)y * W;   // field: the other side, class k at + k hw
  const unsigned long long* fi = ints + (int64_t)b * C * ncol;
  double acc = 0.0;                                                                 // thread c0 + tid < c0 + nc: this row's sum
  for (int x0 = 0; x0 < W; x0 += 256) {
    const int x = x0 + tid;
    int c = NOCLS;
    if (x < W) {
      c = q[x];
      // the class must be in this call's range and have edge pixels on the other side (its field is undefined otherwise)
      if (c != NOCLS && (c < c0 || c >= c0 + nc || fi[(int64_t)c * ncol + 3 + (1 - s)] == 0)) c = NOCLS;
    }
    if (!__syncthreads_or(c != NOCLS)) continue;
    double val = 0.0;
    if (c != NOCLS) {
      const int d2 = row_min(gf + (int64_t)(c - c0) * hw, x, W);
      for (int j = 0; j < T; ++j)
        if (d2 <= thr.t[j]) atomicAdd(&s_hit[c * MAXT + j], 1);
      atomicMax(&s_max[c], d2);
      val = sqrt((double)d2);
    }
    s_val[tid] = val;
    s_cls[tid] = (uint8_t)c;
    __syncthreads();
    if (tid < nc) {
      const int mine = c0 + tid;
      for (int i = 0; i < 256; ++i)
        if (s_cls[i] == mine) acc += s_val[i];
    }
    __syncthreads();
  }
  if (tid < nc) partial[(((int64_t)b * 2 + s) * nc + tid) * H + y] = acc;
  __syncthreads();
  if (tid < C * MAXT) {
    const int c = tid / MAXT, j = tid % MAXT;
    if (j < T && s_hit[tid]) atomicAdd(&ints[((int64_t)b * C + c) * ncol + 7 + s * T + j], (unsigned long long)s_hit[tid]);
  }
  if (tid < C && s_max[tid]) atomicMax(&ints[((int64_t)b * C + tid) * ncol + 5 + s], (unsigned long long)s_max[tid]);
}

// partial [B][2][nc][H] -> sums [B][C][2], fixed order; grid (nc, B, 2), 256 threads
__global__ __launch_bounds__(256) void surface_sum_kernel(const double* __restrict__ partial, int H, int C, int c0, int nc,
                                                          double* __restrict__ sums) {
  __shared__ double s_acc[256];
  const int tid = threadIdx.x, k = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
  const double* p = partial + (((int64_t)b * 2 + s) * nc + k) * H;
  double a = 0.0;
  for (int y = tid; y < H; y += 256) a += p[y];
  s_acc[tid] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_acc[tid] += s_acc[tid + o];
    __syncthreads();
  }
  if (tid == 0) sums[((int64_t)b * C + c0 + k) * 2 + s] = s_acc[0];
}

// the whole field of side ``side``: d2 int32 [B][C][H][W], classes c0 .. c0 + nc - 1; grid (H, nc, B), 256 threads
__global__ __launch_bounds__(256) void surface_field_kernel(const uint16_t* __restrict__ g, int H, int W, int C, int c0, int nc,
                                                            int ncol, int side, const unsigned long long* __restrict__ ints,
                                                            int32_t* __restrict__ d2) {
  const int y = blockIdx.x, k = blockIdx.y, b = blockIdx.z;
  if (ints[((int64_t)b * C + c0 + k) * ncol + 3 + side] == 0) return;   // no edge pixels: the field is undefined (left as it is)
  const int64_t hw = (int64_t)H * W;
  const uint16_t* gr = g + (((int64_t)b * 2 + side) * nc + k) * hw + (int64_t)y * W;
  int32_t* o = d2 + ((int64_t)b * C + c0 + k) * hw + (int64_t)y * W;
  for (int x = threadIdx.x; x < W; x += 256) o[x] = row_min(gr, x, W);
}

// ---- percentile Hausdorff: order statistics of the distance multisets (definitions: include/asis_hip.h) -------------------------
// A SEGMENTED MSB radix select over the exact integer keys d2 < 2^30, four 8-bit digits.  A slot is one (frame, class of the
// call, percentile, set); set 0 = d2_G over E(P), 1 = d2_P over E(G), 2 = the two pooled.  Every launch is ordered by the stream,
// nothing is read back by the host and no workgroup waits on another; every count is an integer atomic and every minimum an
// integer atomicMin, so ord does not depend on the order of the blocks.
//   pct_fill    surface_row_kernel's geometry: row_min once per query edge pixel -> dq (written at those pixels only: nothing
//               else of dq is ever read) and the histogram of the top byte per (frame, class, side).  That histogram has no
//               prefix yet, so the percentiles share it and the pooled set is the sum of the two sides.
//   pct_pick    one workgroup per slot, one thread per bin.  After pass 0 it forms n from ints and lo = (n - 1) q / 10000,
//               dhi = ((n - 1) q % 10000 != 0) on the device; after every pass it finds the bin that holds rank k among the keys
//               that match the prefix, appends the digit and takes the keys below it off k.  After the last pass the prefix is
//               v[lo] and the bin's count is #(key == v[lo]): v[hi] = v[lo] if k + dhi is still inside it, else the smallest
//               key above v[lo] (NEED).  It zeroes the slot's bins for the next pass.
//   pct_hist    passes 1..3 over tiles of 4096 pixels of one (frame, side, percentile): the next byte of the keys that match
//               the slot's prefix, for the side's own set and for the pooled one (they have different prefixes); LDS atomics,
//               then one global atomic per non-zero bin per block.  A block whose classes are all unmatched, or whose tile
//               holds no matching key, ends early.
//   pct_min     the same tiles: min over the keys > v[lo] for the slots that NEED it (none, usually: the blocks end at once).
//   pct_write   ord[b][c][p][set] = (v[lo], v[hi]) for the matched classes; the others keep the caller's -1.
constexpr int MAXP = 4;                      // percentiles per call
constexpr int PCT_TILE = 4096;               // pixels of a tile of pct_hist / pct_min: 16 per thread
constexpr uint32_t PCT_VALID = 1u, PCT_DHI = 2u, PCT_NEED = 4u;
constexpr uint32_t PCT_NONE = 0xFFFFFFFFu;
static_assert(2ll * (MAXHW - 1) * (MAXHW - 1) < (1ll << 30), "the keys must stay below 2^30");

struct PctQ { int q[MAXP]; };
struct PctState { uint32_t prefix, k, flags, above; };   // above: min over the keys > v[lo] (pct_min)

__device__ __forceinline__ int64_t pct_slot(int b, int k, int p, int set, int nc, int P) {
  return (((int64_t)b * nc + k) * P + p) * 3 + set;
}

// grid (H, B, 2), 256 threads; hist0 uint32 [B][nc][2][256]
__global__ __launch_bounds__(256) void pct_fill_kernel(const uint8_t* __restrict__ edges, const uint16_t* __restrict__ g, int H, int W,
                                                       int C, int c0, int nc, int ncol, const unsigned long long* __restrict__ ints,
                                                       int32_t* __restrict__ dq, uint32_t* __restrict__ hist0) {
  __shared__ uint32_t s_h[MAXC * 256];
  __shared__ int s_ok[MAXC];
  const int tid = threadIdx.x, y = blockIdx.x, b = blockIdx.y, s = blockIdx.z;
  const int64_t hw = (int64_t)H * W;
  if (tid < nc) {
    const unsigned long long* fi = ints + ((int64_t)b * C + c0 + tid) * ncol;
    s_ok[tid] = fi[3] != 0 && fi[4] != 0;                  // matched: edge pixels on both sides
  }
  for (int i = tid; i < nc * 256; i += 256) s_h[i] = 0;
  __syncthreads();
  const int64_t row = ((int64_t)b * 2 + s) * hw + (int64_t)y * W;
  const uint8_t* q = edges + row;
  const uint16_t* gf = g + ((int64_t)b * 2 + (1 - s)) * nc * hw + (int64_t)y * W;
  int found = 0;
  for (int x = tid; x < W; x += 256) {
    const int k = (int)q[x] - c0;                           // NOCLS - c0 >= nc: MAXC <= 16
    if (k < 0 || k >= nc || !s_ok[k]) continue;
    const int d2 = row_min(gf + (int64_t)k * hw, x, W);
    dq[row + x] = d2;
    atomicAdd(&s_h[k * 256 + (d2 >> 24)], 1u);
    found = 1;
  }
  if (!__syncthreads_or(found)) return;
  for (int i = tid; i < nc * 256; i += 256) {
    const uint32_t v = s_h[i];
    if (v) atomicAdd(&hist0[(((int64_t)b * nc + (i >> 8)) * 2 + s) * 256 + (i & 255)], v);
  }
}

// grid (3 P, nc, B), 256 threads: thread d looks at bin d
__global__ __launch_bounds__(256) void pct_pick_kernel(const unsigned long long* __restrict__ ints, int C, int c0, int nc, int ncol,
                                                       int P, PctQ pq, int pass, const uint32_t* __restrict__ hist0,
                                                       uint32_t* __restrict__ hist, PctState* __restrict__ state) {
  __shared__ int ws[RX_WAVES];
  const int tid = threadIdx.x;
  const int p = blockIdx.x / 3, set = blockIdx.x % 3, k = blockIdx.y, b = blockIdx.z;
  const int64_t slot = pct_slot(b, k, p, set, nc, P);
  uint32_t prefix = 0, rank, flags, cnt;
  if (pass == 0) {
    const unsigned long long* fi = ints + ((int64_t)b * C + c0 + k) * ncol;
    const int64_t ep = (int64_t)fi[3], el = (int64_t)fi[4];
    if (ep == 0 || el == 0) {                               // unmatched: no value; the later passes skip the slot
      if (tid == 0) state[slot] = PctState{0u, 0u, 0u, PCT_NONE};
      return;
    }
    const int64_t n = set == 0 ? ep : (set == 1 ? el : ep + el);
    const int64_t r = (n - 1) * (int64_t)pq.q[p];
    rank = (uint32_t)(r / 10000);
    flags = PCT_VALID | (r % 10000 != 0 ? PCT_DHI : 0u);
    const uint32_t* h = hist0 + ((int64_t)b * nc + k) * 2 * 256;
    cnt = set == 0 ? h[tid] : (set == 1 ? h[256 + tid] : h[tid] + h[256 + tid]);
  } else {
    const PctState st = state[slot];
    if (!(st.flags & PCT_VALID)) return;
    prefix = st.prefix, rank = st.k, flags = st.flags;
    cnt = hist[slot * 256 + tid];
    hist[slot * 256 + tid] = 0;                             // for the next pass (only this block reads these bins)
  }
  // a slot holds fewer than 2^30 keys: int.  Its barrier also puts every read of state[slot] before the one write below
  const uint32_t incl = (uint32_t)block_incl_scan((int)cnt, ws);
  if (bin_holds_rank(incl, cnt, rank)) {                    // exactly one thread: the bins hold more than `rank` keys
    PctState st;
    st.prefix = prefix | ((uint32_t)tid << (24 - 8 * pass));
    st.k = rank - (incl - cnt);
    st.flags = flags;
    if (pass == 3 && st.k + ((flags & PCT_DHI) ? 1u : 0u) >= cnt) st.flags |= PCT_NEED;   // v[hi] lies above the ties of v[lo]
    st.above = PCT_NONE;
    state[slot] = st;
  }
}

// what a block of pct_hist / pct_min needs of the slots of its (frame, side, percentile): [class][0 = own set, 1 = pooled]
__device__ __forceinline__ bool pct_load_slots(const PctState* __restrict__ state, int b, int s, int p, int nc, int P, uint32_t want,
                                               uint32_t (*s_prefix)[2], int (*s_on)[2]) {
  const int tid = threadIdx.x;
  int on = 0;
  if (tid < nc * 2) {
    const PctState st = state[pct_slot(b, tid >> 1, p, (tid & 1) ? 2 : s, nc, P)];
    on = (st.flags & want) != 0;
    s_prefix[tid >> 1][tid & 1] = st.prefix;
    s_on[tid >> 1][tid & 1] = on;
  }
  return __syncthreads_or(on) != 0;
}

// grid (ceil(H W / PCT_TILE), B, 2 P), 256 threads; pass 1..3
__global__ __launch_bounds__(256) void pct_hist_kernel(const uint8_t* __restrict__ edges, const int32_t* __restrict__ dq, int64_t hw,
                                                       int c0, int nc, int P, int pass, const PctState* __restrict__ state,
                                                       uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_h[MAXC * 2 * 256];
  __shared__ uint32_t s_prefix[MAXC][2];
  __shared__ int s_on[MAXC][2];
  const int tid = threadIdx.x, b = blockIdx.y, s = blockIdx.z & 1, p = blockIdx.z >> 1;
  if (!pct_load_slots(state, b, s, p, nc, P, PCT_VALID, s_prefix, s_on)) return;
  for (int i = tid; i < nc * 512; i += 256) s_h[i] = 0;
  __syncthreads();
  const int up = 32 - 8 * pass, shift = 24 - 8 * pass;
  const int64_t plane = ((int64_t)b * 2 + s) * hw, base = (int64_t)blockIdx.x * PCT_TILE;
  int found = 0;
#pragma unroll 4
  for (int it = 0; it < PCT_TILE / 256; ++it) {
    const int64_t i = base + it * 256 + tid;
    if (i >= hw) break;
    const int k = (int)edges[plane + i] - c0;
    if (k < 0 || k >= nc || !s_on[k][0]) continue;          // own and pooled slot are valid together (the class is matched)
    const uint32_t key = (uint32_t)dq[plane + i];
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if ((key >> up) == (s_prefix[k][j] >> up)) {
        atomicAdd(&s_h[(k * 2 + j) * 256 + ((key >> shift) & 255u)], 1u);
        found = 1;
      }
  }
  if (!__syncthreads_or(found)) return;
  for (int i = tid; i < nc * 512; i += 256) {
    const uint32_t v = s_h[i];
    if (v) atomicAdd(&hist[pct_slot(b, i >> 9, p, ((i >> 8) & 1) ? 2 : s, nc, P) * 256 + (i & 255)], v);
  }
}

// grid as pct_hist_kernel
__global__ __launch_bounds__(256) void pct_min_kernel(const uint8_t* __restrict__ edges, const int32_t* __restrict__ dq, int64_t hw,
                                                      int c0, int nc, int P, PctState* __restrict__ state) {
  __shared__ uint32_t s_min[MAXC][2];
  __shared__ uint32_t s_prefix[MAXC][2];
  __shared__ int s_on[MAXC][2];
  const int tid = threadIdx.x, b = blockIdx.y, s = blockIdx.z & 1, p = blockIdx.z >> 1;
  if (tid < MAXC * 2) s_min[tid >> 1][tid & 1] = PCT_NONE;
  if (!pct_load_slots(state, b, s, p, nc, P, PCT_NEED, s_prefix, s_on)) return;   // its barrier orders s_min as well
  const int64_t plane = ((int64_t)b * 2 + s) * hw, base = (int64_t)blockIdx.x * PCT_TILE;
#pragma unroll 4
  for (int it = 0; it < PCT_TILE / 256; ++it) {
    const int64_t i = base + it * 256 + tid;
    if (i >= hw) break;
    const int k = (int)edges[plane + i] - c0;
    if (k < 0 || k >= nc || !(s_on[k][0] | s_on[k][1])) continue;
    const uint32_t key = (uint32_t)dq[plane + i];
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (s_on[k][j] && key > s_prefix[k][j]) atomicMin(&s_min[k][j], key);
  }
  __syncthreads();
  if (tid < nc * 2 && s_min[tid >> 1][tid & 1] != PCT_NONE)
    atomicMin(&state[pct_slot(b, tid >> 1, p, (tid & 1) ? 2 : s, nc, P)].above, s_min[tid >> 1][tid & 1]);
}

// one thread per slot; ord int64 [B][C][P][3][2]
__global__ __launch_bounds__(256) void pct_write_kernel(const PctState* __restrict__ state, int64_t nslot, int C, int c0, int nc, int P,
                                                        int64_t* __restrict__ ord) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nslot) return;
  const PctState st = state[i];
  if (!(st.flags & PCT_VALID)) return;
  const int64_t bk = i / (3 * P), ps = i - bk * (3 * P);
  const int64_t b = bk / nc, k = bk - b * nc;
  int64_t* o = ord + (((b * C + c0 + k) * P) * 3 + ps) * 2;
  o[0] = (int64_t)st.prefix;
  o[1] = (int64_t)((st.flags & PCT_NEED) ? st.above : st.prefix);
}

struct PctScratch { int64_t hist0, hist, state, bytes; };
inline PctScratch pct_layout(int64_t B, int64_t nc, int64_t P) {
  PctScratch s;
  s.hist0 = 0;
  s.hist = s.hist0 + B * nc * 2 * 256 * 4;
  s.state = s.hist + B * nc * P * 3 * 256 * 4;
  s.bytes = s.state + B * nc * P * 3 * (int64_t)sizeof(PctState);
  return s;
}

}  // namespace

extern "C" int64_t asis_surface_quantile_scratch_bytes(int B, int nc, int P) {
  if (B < 1 || B > 32767 || nc < 1 || nc > MAXC || P < 1 || P > MAXP) {
    asis_set_error_("asis_surface_quantile_scratch_bytes: need 1 <= B <= 32767, 1 <= nc <= %d, 1 <= P <= %d", MAXC, MAXP);
    return ASIS_EINVAL;
  }
  return pct_layout(B, nc, P).bytes;
}

extern "C" int asis_surface_quantiles(void* stream, const uint8_t* edges, const uint16_t* g, const int64_t* ints, int B, int H, int W,
                                      int C, int c0, int nc, int T, const int32_t* q, int P, int32_t* dq, void* scratch,
                                      int64_t* ord) {
  ASIS_REQUIRE(edges && g && ints && q && dq && scratch && ord,
               "asis_surface_quantiles: null pointer (edges, g, ints, q, dq, scratch and ord are required)");
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "asis_surface_quantiles: C=%d must be in 1..%d", C, MAXC);
  ASIS_REQUIRE(c0 >= 0 && nc >= 1 && c0 + nc <= C, "asis_surface_quantiles: class range c0=%d nc=%d outside 0..C=%d", c0, nc, C);
  ASIS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "asis_surface_quantiles: non-positive size B=%d H=%d W=%d", B, H, W);
  ASIS_REQUIRE(B <= 32767 && H <= MAXHW && W <= MAXHW,
               "asis_surface_quantiles: B=%d H=%d W=%d: sizes above %d (batch above 32767) are not supported", B, H, W, MAXHW);
  ASIS_REQUIRE(T >= 0 && T <= MAXT, "asis_surface_quantiles: T=%d tolerances (the row length of ints), supported 0..%d", T, MAXT);
  ASIS_REQUIRE(P >= 1 && P <= MAXP, "asis_surface_quantiles: P=%d percentiles, supported 1..%d", P, MAXP);
  PctQ pq;
  for (int p = 0; p < MAXP; ++p) {
    pq.q[p] = p < P ? q[p] : 0;
    ASIS_REQUIRE(pq.q[p] >= 0 && pq.q[p] <= 10000, "asis_surface_quantiles: q=%d must be in 0..10000 (hundredths of a percent)",
                 pq.q[p]);
  }
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(ints) & 7) == 0 && (reinterpret_cast<uintptr_t>(ord) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(scratch) & 15) == 0 && (reinterpret_cast<uintptr_t>(dq) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(g) & 1) == 0,
               "asis_surface_quantiles: misaligned buffer (scratch: 16 bytes; ints, ord: 8; dq: 4; g: 2)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ncol = 7 + 2 * T;
  const int64_t hw = (int64_t)H * W;
  const PctScratch L = pct_layout(B, nc, P);
  char* base = static_cast<char*>(scratch);
  uint32_t* hist0 = reinterpret_cast<uint32_t*>(base + L.hist0);
  uint32_t* hist = reinterpret_cast<uint32_t*>(base + L.hist);
  PctState* state = reinterpret_cast<PctState*>(base + L.state);
  const unsigned long long* ip = reinterpret_cast<const unsigned long long*>(ints);
  const hipError_t e = hipMemsetAsync(scratch, 0, (size_t)L.bytes, s);
  if (e != hipSuccess) ASIS_FAIL(ASIS_ELAUNCH, "asis_surface_quantiles: %s", hipGetErrorString(e));
  const dim3 blk(256), pick((unsigned)(3 * P), (unsigned)nc, (unsigned)B);
  const dim3 tiles((unsigned)((hw + PCT_TILE - 1) / PCT_TILE), (unsigned)B, (unsigned)(2 * P));
  hipLaunchKernelGGL(pct_fill_kernel, dim3((unsigned)H, (unsigned)B, 2), blk, 0, s, edges, g, H, W, C, c0, nc, ncol, ip, dq, hist0);
  ASIS_CHECK_LAUNCH("asis_surface_quantiles (fill)");
  hipLaunchKernelGGL(pct_pick_kernel, pick, blk, 0, s, ip, C, c0, nc, ncol, P, pq, 0, hist0, hist, state);
  for (int pass = 1; pass < 4; ++pass) {
    hipLaunchKernelGGL(pct_hist_kernel, tiles, blk, 0, s, edges, dq, hw, c0, nc, P, pass, state, hist);
    hipLaunchKernelGGL(pct_pick_kernel, pick, blk, 0, s, ip, C, c0, nc, ncol, P, pq, pass, hist0, hist, state);
  }
  ASIS_CHECK_LAUNCH("asis_surface_quantiles (select)");
  hipLaunchKernelGGL(pct_min_kernel, tiles, blk, 0, s, edges, dq, hw, c0, nc, P, state);
  const int64_t nslot = (int64_t)B * nc * P * 3;
  hipLaunchKernelGGL(pct_write_kernel, dim3((unsigned)((nslot + 255) / 256)), blk, 0, s, state, nslot, C, c0, nc, P, ord);
  ASIS_CHECK_LAUNCH("asis_surface_quantiles (write)");
  return ASIS_OK;
}

extern "C" int asis_surface_stats(void* stream, const uint8_t* pred, const uint8_t* target, const uint8_t* pred_lut,
                                  const uint8_t* lut, int B, int H, int W, int C, int c0, int nc, const int32_t* thr, int T,
                                  uint8_t* edges, uint16_t* g, double* partial, int64_t* ints, double* sums, int32_t* d2,
                                  int d2_side) {
  ASIS_REQUIRE(pred && target && pred_lut && lut && edges && g && partial && ints && sums,
               "asis_surface_stats: null pointer (pred, target, both tables, the workspace and both outputs are required)");
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "asis_surface_stats: C=%d must be in 1..%d", C, MAXC);
  ASIS_REQUIRE(c0 >= 0 && nc >= 1 && c0 + nc <= C, "asis_surface_stats: class range c0=%d nc=%d outside 0..C=%d", c0, nc, C);
  ASIS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "asis_surface_stats: non-positive size B=%d H=%d W=%d", B, H, W);
  ASIS_REQUIRE(B <= 32767 && H <= MAXHW && W <= MAXHW,
               "asis_surface_stats: B=%d H=%d W=%d: sizes above %d (batch above 32767) are not supported: squared distances must "
               "fit int32", B, H, W, MAXHW);
  ASIS_REQUIRE(T >= 0 && T <= MAXT && (T == 0 || thr), "asis_surface_stats: T=%d tolerances, supported 0..%d", T, MAXT);
  ASIS_REQUIRE(!d2 || d2_side == 0 || d2_side == 1, "asis_surface_stats: d2_side=%d must be 0 (pred) or 1 (target)", d2_side);
  ASIS_REQUIRE((reinterpret_cast<uintptr_t>(ints) & 7) == 0 && (reinterpret_cast<uintptr_t>(sums) & 7) == 0 &&
                   (reinterpret_cast<uintptr_t>(partial) & 7) == 0 && (reinterpret_cast<uintptr_t>(g) & 1) == 0 &&
                   (reinterpret_cast<uintptr_t>(d2) & 3) == 0,
               "asis_surface_stats: misaligned buffer (ints, sums, partial: 8 bytes; d2: 4; g: 2)");
  Thr t;
  for (int j = 0; j < MAXT; ++j) {
    t.t[j] = j < T ? thr[j] : 0;
    ASIS_REQUIRE(t.t[j] >= 0, "asis_surface_stats: squared tolerance %d is negative", t.t[j]);
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ncol = 7 + 2 * T;
  unsigned long long* ip = reinterpret_cast<unsigned long long*>(ints);
  const int64_t hw = (int64_t)H * W;
  if (c0 == 0) {
    hipLaunchKernelGGL(surface_edges_kernel, dim3((unsigned)((hw + 255) / 256), (unsigned)B), dim3(256), 0, s, pred, target,
                       pred_lut, lut, H, W, C, ncol, edges, ip);
    ASIS_CHECK_LAUNCH("asis_surface_stats (edges)");
  }
  hipLaunchKernelGGL(surface_column_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)nc, (unsigned)(B * 2)), dim3(256), 0, s,
                     edges, H, W, C, c0, nc, ncol, ip, g);
  ASIS_CHECK_LAUNCH("asis_surface_stats (columns)");
  hipLaunchKernelGGL(surface_row_kernel, dim3((unsigned)H, (unsigned)B, 2), dim3(256), 0, s, edges, g, H, W, C, c0, nc, ncol, T, t,
                     ip, partial);
  ASIS_CHECK_LAUNCH("asis_surface_stats (rows)");
  hipLaunchKernelGGL(surface_sum_kernel, dim3((unsigned)nc, (unsigned)B, 2), dim3(256), 0, s, partial, H, C, c0, nc, sums);
  ASIS_CHECK_LAUNCH("asis_surface_stats (sums)");
  if (d2) {
    hipLaunchKernelGGL(surface_field_kernel, dim3((unsigned)H, (unsigned)nc, (unsigned)B), dim3(256), 0, s, g, H, W, C, c0, nc,
                       ncol, d2_side, ip, d2);
    ASIS_CHECK_LAUNCH("asis_surface_stats (field)");
  }
  return ASIS_OK;
}
