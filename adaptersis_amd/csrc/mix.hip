// CutMix / ClassMix over the samples of one batch, and the consistency loss of consist.hip over such a batch.  Built into
// libasis_mix.so (build.py SIDE_LIBS; ABI and semantics in include/asis_mix.h), beside libasis_hip.so, whose error plumbing it uses.
//
// Three small kernels and one instantiation:
//   mix_presence_kernel  target -> one class bit set per sample.  A thread ORs the bits of its labels, a wave ORs its lanes through
//                        shuffles, lane 0 takes one atomicOr per wave and sample (an integer atomic: the result has no order).
//   mix_select_kernel    one thread per sample: the classes a ClassMix sample pastes, out of its donor's set.
//   mix_apply_kernel     the streaming pass: sel, the mixed image and labels, the pasted count.  A tile is MX_TILE pixels of ONE
//                        sample (so kind, box, donor and set are uniform over a workgroup); a workgroup walks the tiles blockIdx.x,
//                        blockIdx.x + gridDim.x, ...; the count is summed per thread, then over the workgroup, and added with one
//                        integer atomic per workgroup and sample.  VEC: a thread holds 4 consecutive pixels of a row (16-byte
//                        accesses of the image, 2 x 16 of the labels, 4 bytes of sel); otherwise consecutive threads hold
//                        consecutive pixels.  Image and labels move as integers: copies of bits.
//   st_kernel<.., MixGate>  soft_target.h's kernel with the gate of consist.hip and the teacher's sample chosen per pixel.
#include "../../include/asis_mix.h"
#include "soft_target.h"

namespace {

constexpr int MX_ITEMS = 4, MX_TILE = RX_THREADS * MX_ITEMS;
constexpr int MX_MAX_BLOCKS = 2048;  // cap of the grid (8 workgroups a CU)
constexpr int MX_PLANES = 3;

typedef int64_t i64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int donor_of(const int* __restrict__ donor, int b, int B) {
  const int d = donor[b];
  return (unsigned)d < (unsigned)B ? d : b;  // never an address outside the batch
}

// tiles of one sample: tps a sample, ntile = B * tps in all
__global__ __launch_bounds__(RX_THREADS) void mix_presence_kernel(const int64_t* __restrict__ target, int hw, int tps, int ntile, int C,
                                                                  uint32_t* __restrict__ present) {
  const int tid = threadIdx.x;
  uint32_t m = 0;
  int cur = -1;
  auto flush = [&]() {  // `cur` is uniform over the workgroup
    if (cur < 0) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m |= __shfl_xor(m, o, 64);
    if ((tid & 63) == 0 && m) atomicOr(present + cur, m);
  };
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int b = tile / tps;
    if (b != cur) {
      flush();
      m = 0;
      cur = b;
    }
    const int r0 = (tile - b * tps) * MX_TILE;
    const int64_t* t = target + (int64_t)b * hw;
#pragma unroll
    for (int j = 0; j < MX_ITEMS; ++j) {
      const int r = r0 + j * RX_THREADS + tid;
      if (r < hw) {
        const uint64_t v = (uint64_t)t[r];
        if (v < (uint64_t)C) m |= 1u << (int)v;
      }
    }
  }
  flush();
}

__global__ __launch_bounds__(RX_THREADS) void mix_select_kernel(const uint32_t* __restrict__ present, const int* __restrict__ donor,
                                                                const int* __restrict__ kind, const uint8_t* __restrict__ order, int B,
                                                                int C, int background, uint32_t* __restrict__ pset) {
  const int b = blockIdx.x * RX_THREADS + threadIdx.x;
  if (b >= B) return;
  uint32_t set = 0;
  if (kind[b] == 2) {
    uint32_t P = present[donor_of(donor, b, B)] & ((1u << C) - 1u);
    if (!background) P &= ~1u;
    const int take = (__popc(P) + 1) / 2;
    int taken = 0;
    for (int k = 0; k < MAXC; ++k) {
      const int c = order[b * MAXC + k];
      if (c < C && ((P >> c) & 1u) && !((set >> c) & 1u) && taken < take) {
        set |= 1u << c;
        ++taken;
      }
    }
  }
  pset[b] = set;
}

__device__ __forceinline__ bool in_set(uint32_t set, int64_t label) { return (uint64_t)label < 32u && ((set >> (int)label) & 1u); }

template <bool VEC>
__global__ __launch_bounds__(RX_THREADS) void mix_apply_kernel(const uint32_t* __restrict__ inp, const int64_t* __restrict__ target,
                                                               const int* __restrict__ donor, const int* __restrict__ kind,
                                                               const int* __restrict__ box, const uint32_t* __restrict__ pset, int B,
                                                               int H, int W, int tps, int ntile, uint32_t* __restrict__ inp_out,
                                                               int64_t* __restrict__ target_out, uint8_t* __restrict__ sel,
                                                               int* __restrict__ pasted) {
  __shared__ int wc[RX_WAVES];
  const int tid = threadIdx.x;
  const int hw = H * W;
  int cnt = 0, cur = -1;
  auto flush = [&]() {  // `cur` is uniform over the workgroup: every thread takes the barriers
    if (cur < 0) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) wc[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
      const int total = (wc[0] + wc[1]) + (wc[2] + wc[3]);
      if (total) atomicAdd(pasted + cur, total);
    }
    __syncthreads();
  };
  for (int tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int b = tile / tps;
    if (b != cur) {
      flush();
      cnt = 0;
      cur = b;
    }
    const int d = donor_of(donor, b, B);
    const uint32_t set = pset ? pset[b] : 0u;
    int k = kind[b];
    if (k == 2 && set == 0u) k = 0;  // nothing to paste: the donor is not read
    const int y0 = box[4 * b], x0 = box[4 * b + 1], y1 = box[4 * b + 2], x1 = box[4 * b + 3];
    const int r0 = (tile - b * tps) * MX_TILE;
    const int64_t* to = target + (int64_t)b * hw;
    const int64_t* td = target + (int64_t)d * hw;
    if constexpr (VEC) {
      const int r = r0 + tid * MX_ITEMS;  // W % 4 == 0: the 4 pixels lie in one row, and r + 3 < hw where r < hw
      if (r >= hw) continue;
      bool s[4] = {false, false, false, false};
      i64x2 dn[2] = {{0, 0}, {0, 0}}, own[2] = {{0, 0}, {0, 0}};
      if (k == 1) {
        const int y = r / W, x = r - y * W;
        const bool row = y >= y0 && y < y1;
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = row && x + e >= x0 && x + e < x1;
      } else if (k == 2) {
        dn[0] = *reinterpret_cast<const i64x2*>(td + r);
        dn[1] = *reinterpret_cast<const i64x2*>(td + r + 2);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = in_set(set, dn[e >> 1][e & 1]);
      }
      const bool any = s[0] | s[1] | s[2] | s[3], all = s[0] & s[1] & s[2] & s[3];
      if (k == 1 && any) {
        dn[0] = *reinterpret_cast<const i64x2*>(td + r);
        dn[1] = *reinterpret_cast<const i64x2*>(td + r + 2);
      }
      if (!all) {
        own[0] = *reinterpret_cast<const i64x2*>(to + r);
        own[1] = *reinterpret_cast<const i64x2*>(to + r + 2);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) own[e >> 1][e & 1] = s[e] ? dn[e >> 1][e & 1] : own[e >> 1][e & 1];
      int64_t* t_out = target_out + (int64_t)b * hw + r;
      *reinterpret_cast<i64x2*>(t_out) = own[0];
      *reinterpret_cast<i64x2*>(t_out + 2) = own[1];
#pragma unroll
      for (int c = 0; c < MX_PLANES; ++c) {
        const int64_t ob = ((int64_t)b * MX_PLANES + c) * hw + r, od = ((int64_t)d * MX_PLANES + c) * hw + r;
        u32x4 vo = {0u, 0u, 0u, 0u}, vd = {0u, 0u, 0u, 0u};
        if (!all) vo = *reinterpret_cast<const u32x4*>(inp + ob);
        if (any) vd = *reinterpret_cast<const u32x4*>(inp + od);
#pragma unroll
        for (int e = 0; e < 4; ++e) vo[e] = s[e] ? vd[e] : vo[e];
        *reinterpret_cast<u32x4*>(inp_out + ob) = vo;
      }
      *reinterpret_cast<uint32_t*>(sel + (int64_t)b * hw + r) =
          (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
      cnt += (int)s[0] + (int)s[1] + (int)s[2] + (int)s[3];
    } else {
#pragma unroll
      for (int j = 0; j < MX_ITEMS; ++j) {
        const int r = r0 + j * RX_THREADS + tid;
        if (r >= hw) continue;
        bool s = false;
        int64_t dn = 0;
        if (k == 1) {
          const int y = r / W, x = r - y * W;
          s = y >= y0 && y < y1 && x >= x0 && x < x1;
          if (s) dn = td[r];
        } else if (k == 2) {
          dn = td[r];
          s = in_set(set, dn);
        }
        target_out[(int64_t)b * hw + r] = s ? dn : to[r];
        const int src = s ? d : b;
#pragma unroll
        for (int c = 0; c < MX_PLANES; ++c)
          inp_out[((int64_t)b * MX_PLANES + c) * hw + r] = inp[((int64_t)src * MX_PLANES + c) * hw + r];
        sel[(int64_t)b * hw + r] = (uint8_t)s;
        cnt += (int)s;
      }
    }
  }
  flush();
}

// the sizes every entry shares -> tiles a sample (0 with the error set)
int mix_tps(const char* op, int B, int64_t HW, int* ntile) {
  if (B < 1 || HW < 1 || HW >= ((int64_t)1 << 31) || (int64_t)B * HW >= ((int64_t)1 << 31)) {
    asis_set_error_("%s: need B >= 1, H*W >= 1 and B*H*W < 2^31 (B=%d, H*W=%lld)", op, B, (long long)HW);
    return 0;
  }
  const int tps = (int)((HW + MX_TILE - 1) / MX_TILE);
  *ntile = B * tps;  // <= B*H*W
  return tps;
}

}  // namespace

extern "C" int asis_mix_tile(void) { return MX_TILE; }

extern "C" int asis_mix_nblk(int B, int64_t HW) {
  int ntile = 0;
  if (!mix_tps("asis_mix_nblk", B, HW, &ntile)) return ASIS_EINVAL;
  return asis_grid(ntile, 1, MX_MAX_BLOCKS);
}

extern "C" int asis_mix_class_sets(void* stream, const int64_t* target, const int* donor, const int* kind, const uint8_t* order, int B,
                                   int H, int W, int C, int background, uint32_t* sets) {
  const char* op = "asis_mix_class_sets";
  ASIS_REQUIRE(target && donor && kind && order && sets, "%s: null pointer", op);
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "%s: C=%d must be in 1..%d", op, C, MAXC);
  ASIS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive size B=%d H=%d W=%d", op, B, H, W);
  int ntile = 0;
  const int tps = mix_tps(op, B, (int64_t)H * W, &ntile);
  if (!tps) return ASIS_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(sets, 0, sizeof(uint32_t) * (size_t)B, s) != hipSuccess) ASIS_FAIL(ASIS_ELAUNCH, "%s: memset failed", op);
  hipLaunchKernelGGL(mix_presence_kernel, dim3(asis_grid(ntile, 1, MX_MAX_BLOCKS)), dim3(RX_THREADS), 0, s, target, H * W, tps, ntile, C,
                     sets);
  hipLaunchKernelGGL(mix_select_kernel, dim3((unsigned)asis_cdiv(B, RX_THREADS)), dim3(RX_THREADS), 0, s, sets, donor,
                     kind, order, B, C, background != 0, sets + B);
  ASIS_CHECK_LAUNCH(op);
  return ASIS_OK;
}

extern "C" int asis_mix_apply(void* stream, const float* inp, const int64_t* target, const int* donor, const int* kind, const int* box,
                              const uint32_t* pasted_sets, int B, int H, int W, float* inp_out, int64_t* target_out, uint8_t* sel,
                              int* pasted) {
  const char* op = "asis_mix_apply";
  ASIS_REQUIRE(inp && target && donor && kind && box && inp_out && target_out && sel && pasted, "%s: null pointer", op);
  ASIS_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive size B=%d H=%d W=%d", op, B, H, W);
  ASIS_REQUIRE(inp != inp_out && target != target_out, "%s: an output aliases its input", op);
  int ntile = 0;
  const int tps = mix_tps(op, B, (int64_t)H * W, &ntile);
  if (!tps) return ASIS_EINVAL;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(pasted, 0, sizeof(int) * (size_t)B, s) != hipSuccess) ASIS_FAIL(ASIS_ELAUNCH, "%s: memset failed", op);
  const bool vec = W % 4 == 0 && asis_aligned16(inp) && asis_aligned16(target) && asis_aligned16(inp_out) && asis_aligned16(target_out) &&
                   asis_aligned16(sel);
  const dim3 grid(asis_grid(ntile, 1, MX_MAX_BLOCKS));
  auto go = [&](auto v) {
    hipLaunchKernelGGL(mix_apply_kernel<decltype(v)::value>, grid, dim3(RX_THREADS), 0, s, reinterpret_cast<const uint32_t*>(inp), target,
                       donor, kind, box, pasted_sets, B, H, W, tps, ntile, reinterpret_cast<uint32_t*>(inp_out), target_out, sel, pasted);
  };
  if (vec) go(std::true_type{});
  else go(std::false_type{});
  ASIS_CHECK_LAUNCH(op);
  return ASIS_OK;
}

extern "C" int asis_mix_consist_tile(void) { return ST_TILE; }

extern "C" int asis_mix_consist_nblk(int64_t N) { return st_nblk("asis_mix_consist_nblk", N); }

extern "C" int asis_mix_consist_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers, const int* hs,
                                     const int* ws, const int* flips, int V, int H, int W, int C, float temperature, float threshold,
                                     const float* sample_weight, const uint8_t* sel, const int* donor, float grad_scale, int accumulate,
                                     double* partial, float* loss, int* kept, float* dz) {
  return st_loss("asis_mix_consist_loss", MixGate{threshold, sample_weight, sel, donor, B}, stream, logits, B, h, w, teachers, hs, ws,
                 flips, V, H, W, C, temperature, grad_scale, accumulate, partial, loss, kept, dz);
}
