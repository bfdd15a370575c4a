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
//
// Intermediate storage (the caller's workspace; ops.surface_stats chunks over frames and classes to bound it):
//   edges   uint8  [B][2][H][W]            at 1080 x 1920:          4.1 MB per frame
//   g       uint16 [B][2][nc][H][W]        at 1080 x 1920, nc = 8: 66.4 MB per frame (8.3 MB per class)
//   partial double [B][2][nc][H]                                    0.14 MB per frame
// = 70.6 MB per frame at 1080 x 1920, C = 8 (847 MB for a batch of 12, 1.6 GiB at C = 16: hence the chunking, which keeps g
// under 512 MiB whenever one class of one frame fits).
#include "asis_common.h"

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

}  // namespace

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
