// Per-pixel segmentation losses, fused with the final bilinear resize of the logits.
//
// Training loss of train.py:422-428:
//     out  = F.interpolate(logits, size=(H, W), mode="bilinear")      (align_corners=False)
//     prob = softmax_C(out)                                           train.py:424
//     loss = DC(C)(prob, target)  with  p = softmax_C(prob)  (second softmax, segloss/dice.py:23)
//            dice[b,c] = 2 sum(p t) / (sum p + sum t + 1e-19) ;  loss = 1 - mean_{b,c} dice
// One pass reads the NHWC logits (4 taps) and the int64 target once and keeps the C running
// sums per thread; wave64 shuffles + one LDS step reduce them per block; the per-block partials
// are summed in double by the finalize kernel (deterministic, no atomics).
// The backward recomputes the two softmaxes instead of storing probabilities:
//     dL/dp[b,c,pix] = a[b,c] * t + g[b,c]   with  a = -2/(BC S), g = 2 I/(BC S^2), S = sum p + sum t + eps
// then softmax^T twice, written at (H, W); asis_resize_bilinear_bwd gathers it back to the
// decoder's (h, w) grid as the 16-bit operand of the dgrad / wgrad GEMMs.
#include "asis_common.h"
#include "bilinear_tap.h"  // MAXC, Tap, tap_ac_false, sample_logits, softmax_c, softmax_bwd_c
#include "seg_loss_body.h"  // the fused loss: seg_loss_{fwd,finalize,bwd}_kernel and their launches; AllValid here, IgnoreLabel in semi.hip

namespace {

// Transpose of the bilinear resize (align_corners=False), gather form (deterministic):
// dsrc[b, sy, sx, c] = sum over output pixels whose taps touch (sy, sx).  Writes a 16-bit NHWC
// tensor with CP (>= C, multiple of 8) channels (pad channels zero) and per-block column sums
// (conv bias gradient): partial[blk][C].
template <typename T>
__global__ __launch_bounds__(256) void resize_bwd_kernel(const float* __restrict__ dz, int B, int H, int W, int h, int w,
                                                         int C, int CP, T* __restrict__ out, T* __restrict__ out_lo,
                                                         float* __restrict__ partial) {
  __shared__ float red[4][MAXC];
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  const float ish = (float)H / (float)h, isw = (float)W / (float)w;
  const int64_t total = (int64_t)B * h * w;
  float csum[MAXC];
#pragma unroll
  for (int c = 0; c < MAXC; ++c) csum[c] = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int sx = (int)(i % w);
    const int sy = (int)((i / w) % h);
    const int b = (int)(i / ((int64_t)w * h));
    float acc[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) acc[c] = 0.f;
    int y_lo = (int)floorf(((float)sy - 1.f + 0.5f) * ish - 0.5f) - 1, y_hi = (int)ceilf(((float)sy + 1.f + 0.5f) * ish - 0.5f) + 1;
    int x_lo = (int)floorf(((float)sx - 1.f + 0.5f) * isw - 0.5f) - 1, x_hi = (int)ceilf(((float)sx + 1.f + 0.5f) * isw - 0.5f) + 1;
    if (y_lo < 0) y_lo = 0;
    if (x_lo < 0) x_lo = 0;
    if (y_hi > H - 1) y_hi = H - 1;
    if (x_hi > W - 1) x_hi = W - 1;
    for (int y = y_lo; y <= y_hi; ++y) {
      const Tap ty = tap_ac_false(y, sh, h);
      const float wy = ((ty.i0 == sy) ? ty.l0 : 0.f) + ((ty.i1 == sy) ? ty.l1 : 0.f);
      if (wy == 0.f) continue;
      for (int x = x_lo; x <= x_hi; ++x) {
        const Tap tx = tap_ac_false(x, sw, w);
        const float wx = ((tx.i0 == sx) ? tx.l0 : 0.f) + ((tx.i1 == sx) ? tx.l1 : 0.f);
        if (wx == 0.f) continue;
        const float* src = dz + (((int64_t)b * H + y) * W + x) * C;
        const float wt = wy * wx;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) acc[c] += wt * src[c];
      }
    }
    T* o = out + i * CP;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < CP) {
        const float v = c < C ? acc[c] : 0.f;
        o[c] = to_t16<T>(v);
        if (out_lo) out_lo[i * CP + c] = to_t16<T>(lo_part<T>(v));
      }
#pragma unroll
    for (int c = 0; c < MAXC; ++c) csum[c] += acc[c];
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < MAXC; ++c)
    if (c < C) {
      const float v = wave_sum(csum[c]);
      if (lane == 0) red[wid][c] = v;
    }
  __syncthreads();
  if (threadIdx.x < C)
    partial[(int64_t)blockIdx.x * C + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// out[k] = scale * sum_n partial[n][k]   (double accumulate).  32 row groups x 8 columns per block (K / 8 blocks: 256 for the
// 2048 columns of a LayerNorm-backward partial, one per CU), four independent loads per thread in flight, one LDS pass over the
// row groups at the end.  The partials were just written: the 32-byte row segments come out of L2.
__global__ __launch_bounds__(256) void reduce_rows_kernel(const float* __restrict__ partial, int n, int K, float scale,
                                                          float* __restrict__ out) {
  constexpr int NG = 32, NCOL = 8;
  __shared__ double red[NG][NCOL + 1];
  const int c = threadIdx.x & (NCOL - 1), g = threadIdx.x / NCOL;
  const int k = blockIdx.x * NCOL + c;
  double s = 0.0;
  if (k < K) {
    const float* p = partial + k;
    int i = g;
    for (; i + 3 * NG < n; i += 4 * NG) {
      const float a0 = p[(int64_t)i * K], a1 = p[(int64_t)(i + NG) * K], a2 = p[(int64_t)(i + 2 * NG) * K],
                  a3 = p[(int64_t)(i + 3 * NG) * K];
      s += ((double)a0 + (double)a1) + ((double)a2 + (double)a3);
    }
    for (; i < n; i += NG) s += (double)p[(int64_t)i * K];
  }
  red[g][c] = s;
  __syncthreads();
  if (g == 0 && k < K) {
    double t = 0.0;
#pragma unroll
    for (int j = 0; j < NG; ++j) t += red[j][c];
    out[k] = (float)(t * (double)scale);
  }
}

// F.interpolate(x, size=(H, W), mode="bilinear") (align_corners=False) on NHWC fp32 (decoders.py:88, train.py:422)
__global__ __launch_bounds__(256) void resize_fwd_kernel(const float* __restrict__ x, int B, int h, int w, int H, int W, int C,
                                                         float* __restrict__ out) {
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  const int64_t total = (int64_t)B * H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int xx = (int)(i % W);
    const int yy = (int)((i / W) % H);
    const int b = (int)(i / ((int64_t)W * H));
    float z[MAXC];
    sample_logits(x + (int64_t)b * h * w * C, h, w, C, yy, xx, sh, sw, z);
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < C) out[i * C + c] = z[c];
  }
}

// Validation metrics of train.py:616-642 in one pass over the (resized) logits: class-weighted cross entropy
// numerator / denominator (nn.CrossEntropyLoss(weight) = sum w[t]*nll / sum w[t]) and the number of pixels
// whose argmax equals the target.  partial[blk][3] = {sum w*nll, sum w, correct}.
__global__ __launch_bounds__(256) void ce_acc_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                     const float* __restrict__ weight, int B, int h, int w, int H, int W,
                                                     int C, float* __restrict__ partial, int* __restrict__ counts) {
  __shared__ float red[4][3];
  __shared__ int cnt[MAXC * 3];  // per class: #(target == c), #(argmax == c), #(both)  (ch_iou / isi_iou inputs)
  if (counts) {
    if (threadIdx.x < MAXC * 3) cnt[threadIdx.x] = 0;
    __syncthreads();
  }
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  const int64_t total = (int64_t)B * H * W;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int x = (int)(i % W);
    const int y = (int)((i / W) % H);
    const int b = (int)(i / ((int64_t)W * H));
    float z[MAXC];
    sample_logits(logits + (int64_t)b * h * w * C, h, w, C, y, x, sh, sw, z);
    float m = -INFINITY;
    int am = 0;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < C && z[c] > m) { m = z[c]; am = c; }
    float se = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < C) se += __expf(z[c] - m);
    const int t = (int)target[i];
    float zt = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c == t) zt = z[c];
    const float wt = weight ? weight[t] : 1.f;
    a0 += wt * (m + __logf(se) - zt);
    a1 += wt;
    a2 += (am == t) ? 1.f : 0.f;
    if (counts) {
      if (t >= 0 && t < C) atomicAdd(&cnt[t * 3 + 0], 1);
      atomicAdd(&cnt[am * 3 + 1], 1);
      if (am == t) atomicAdd(&cnt[am * 3 + 2], 1);
    }
  }
  if (counts) {
    __syncthreads();
    if (threadIdx.x < C * 3 && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], cnt[threadIdx.x]);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
  if (lane == 0) { red[wid][0] = a0; red[wid][1] = a1; red[wid][2] = a2; }
  __syncthreads();
  if (threadIdx.x < 3)
    partial[(int64_t)blockIdx.x * 3 + threadIdx.x] =
        (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// few rows, many columns (split-K slabs of the weight gradients): one thread per column, coalesced rows
__global__ __launch_bounds__(256) void reduce_rows_wide_kernel(const float* __restrict__ partial, int n, int64_t K,
                                                               float scale, float* __restrict__ out) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)partial[(int64_t)i * K + k];
    out[k] = (float)(s * (double)scale);
  }
}

}  // namespace

extern "C" int asis_dice_nblk(int H, int W) {
  int n = (H * W + 256 * 8 - 1) / (256 * 8);
  if (n > 512) n = 512;
  if (n < 1) n = 1;
  return n;
}

extern "C" int asis_seg_loss_fwd(void* stream, const float* logits, const int64_t* target, const float* ce_weight, int B,
                                 int h, int w, int H, int W, int C, int n_region, int mode, float eps, int n_ce,
                                 float grad_scale, float* partial, float* sums, float* loss, float* coef) {
  return seg_loss_fwd_launch("asis_seg_loss_fwd", AllValid{}, stream, logits, target, ce_weight, B, h, w, H, W, C, n_region, mode, eps,
                             n_ce, grad_scale, partial, sums, loss, coef);
}

extern "C" int asis_seg_loss_bwd(void* stream, const float* logits, const int64_t* target, const float* coef,
                                 const float* ce_weight, int B, int h, int w, int H, int W, int C, int n_region, int mode,
                                 int n_ce, float* dz) {
  return seg_loss_bwd_launch("asis_seg_loss_bwd", AllValid{}, stream, logits, target, coef, ce_weight, B, h, w, H, W, C, n_region, mode,
                             n_ce, dz);
}

// the two-mode entry points of the train.py / train_mla.py losses (region term only)
extern "C" int asis_dice_fwd(void* stream, const float* logits, const int64_t* target, int B, int h, int w, int H, int W,
                             int C, int n_softmax, float eps, int mode, float grad_scale, float* partial, float* sums,
                             float* loss, float* coef) {
  ASIS_REQUIRE(mode == 0 || mode == 1, "asis_dice_fwd: mode must be 0 (Dice) or 1 (soft IoU)");
  return asis_seg_loss_fwd(stream, logits, target, nullptr, B, h, w, H, W, C, n_softmax, mode, eps, 0, grad_scale, partial,
                           sums, loss, coef);
}

extern "C" int asis_dice_bwd(void* stream, const float* logits, const int64_t* target, const float* coef, int B, int h,
                             int w, int H, int W, int C, int n_softmax, float* dz) {
  ASIS_REQUIRE(n_softmax >= 1 && n_softmax <= 2, "asis_dice_bwd: bad n_softmax");
  return asis_seg_loss_bwd(stream, logits, target, coef, nullptr, B, h, w, H, W, C, n_softmax, 0, 0, dz);
}

extern "C" int asis_resize_bilinear_fwd(void* stream, const float* x, int B, int h, int w, int H, int W, int C, float* out) {
  ASIS_REQUIRE(x && out && C >= 1 && C <= MAXC, "asis_resize_bilinear_fwd: bad arguments (C <= %d)", MAXC);
  hipLaunchKernelGGL(resize_fwd_kernel, dim3(asis_grid((int64_t)B * H * W, 256, 8192)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     x, B, h, w, H, W, C, out);
  ASIS_CHECK_LAUNCH("asis_resize_bilinear_fwd");
  return ASIS_OK;
}

extern "C" int asis_ce_acc_nblk(int64_t total_pixels) {
  return asis_grid(total_pixels, 256 * 8, 2048);
}

extern "C" int asis_ce_acc_counts(void* stream, const float* logits, const int64_t* target, const float* weight, int B,
                                  int h, int w, int H, int W, int C, float* partial, int32_t* counts) {
  ASIS_REQUIRE(logits && target && partial, "asis_ce_acc: null pointer");
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "asis_ce_acc: C=%d must be in 1..%d", C, MAXC);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (counts && hipMemsetAsync(counts, 0, sizeof(int32_t) * C * 3, s) != hipSuccess)
    ASIS_FAIL(ASIS_ELAUNCH, "asis_ce_acc_counts: hipMemsetAsync failed");
  hipLaunchKernelGGL(ce_acc_kernel, dim3(asis_ce_acc_nblk((int64_t)B * H * W)), dim3(256), 0, s, logits, target, weight, B,
                     h, w, H, W, C, partial, counts);
  ASIS_CHECK_LAUNCH("asis_ce_acc");
  return ASIS_OK;
}

extern "C" int asis_ce_acc(void* stream, const float* logits, const int64_t* target, const float* weight, int B, int h,
                           int w, int H, int W, int C, float* partial) {
  return asis_ce_acc_counts(stream, logits, target, weight, B, h, w, H, W, C, partial, nullptr);
}

extern "C" int asis_resize_bwd_nblk(int64_t total_pixels) {
  return asis_grid(total_pixels, 256, 4096);
}

extern "C" int asis_resize_bilinear_bwd(void* stream, int dtype, const float* dz, int B, int H, int W, int h, int w, int C,
                                        int CP, void* out, void* out_lo, float* partial) {
  ASIS_REQUIRE(dz && out && partial, "asis_resize_bilinear_bwd: null pointer");
  ASIS_REQUIRE(C >= 1 && C <= MAXC && CP >= C && CP <= MAXC, "asis_resize_bilinear_bwd: bad C=%d CP=%d", C, CP);
  if (dtype != ASIS_F32) ASIS_DT_OK(dtype, "asis_resize_bilinear_bwd");
  ASIS_REQUIRE(dtype == ASIS_F32 || CP % 8 == 0, "asis_resize_bilinear_bwd: 16-bit output needs CP %% 8 == 0");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nblk = asis_resize_bwd_nblk((int64_t)B * h * w);
  if (dtype == ASIS_F32)  // the float branch stays explicit (no second plane): the dispatcher knows the two 16-bit types only
    hipLaunchKernelGGL((resize_bwd_kernel<float>), dim3(nblk), dim3(256), 0, s, dz, B, H, W, h, w, C, CP,
                       static_cast<float*>(out), static_cast<float*>(nullptr), partial);
  else if (int rc = asis_dispatch16(dtype, "asis_resize_bilinear_bwd", [&](auto t) {
             using T = decltype(t);
             hipLaunchKernelGGL((resize_bwd_kernel<T>), dim3(nblk), dim3(256), 0, s, dz, B, H, W, h, w, C, CP,
                                static_cast<T*>(out), static_cast<T*>(out_lo), partial);
           })) return rc;
  ASIS_CHECK_LAUNCH("asis_resize_bilinear_bwd");
  return ASIS_OK;
}

extern "C" int asis_reduce_rows(void* stream, const float* partial, int n, int K, float scale, float* out) {
  ASIS_REQUIRE(partial && out && n > 0 && K > 0, "asis_reduce_rows: bad arguments");
  if (n <= 64 || K > 65535) {
    hipLaunchKernelGGL(reduce_rows_wide_kernel, dim3(asis_grid(K, 256, 8192)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       partial, n, (int64_t)K, scale, out);
  } else {
    hipLaunchKernelGGL(reduce_rows_kernel, dim3((K + 7) / 8), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), partial, n,
                       K, scale, out);
  }
  ASIS_CHECK_LAUNCH("asis_reduce_rows");
  return ASIS_OK;
}
