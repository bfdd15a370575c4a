// The fused segmentation loss that loss.hip and semi.hip export: the forward, finalize and backward kernel bodies, the argument
// checks and the launches in front of them, included by those two sources and by nothing else.  loss.hip documents the arithmetic;
// semi.hip what an ignore label adds.  Which pixels take part is a type (AllValid / IgnoreLabel), the way soft_target.h has its
// gate: everything the ignore label adds sits behind `if constexpr (V::on)`, so the AllValid kernels of libasis_hip.so carry none
// of it (same statements in the same order as before the bodies moved here).
//
// IgnoreLabel{g}: v_i = [t_i != g], n_b = sum_{i in b} v_i, sample b PRESENT when n_b > 0, P = number of present samples.
//   forward    an ignored pixel adds to no sum and its logits are not sampled (only its 8-byte label is read); one more partial
//              per (b, block): the block's count of valid pixels, an int in the float slot (bit pattern, exact).  The label
//              decides whether the taps are loaded at all, so its latency would stand in front of theirs: both passes load
//              the label of a thread's NEXT pixel one trip ahead (measured: 2 % of the op's time at 24 x 588^2 x 8)
//   finalize   n_b (`valid`, int32 [B]); the mean of the region term over the P*C pairs of the present samples (P*C replaces B*C
//              in the loss and in coef; coef of an absent sample is 0; P = 0: region term exactly 0); CE = sum v w nll / sum v w,
//              exactly 0 with a CE scale of 0 where the denominator is 0
//   backward   dz is all-bits-zero on an ignored pixel, whose logits are not sampled; a sample with n_b = 0 gets zeros and reads
//              neither its logits nor its labels
// Labels outside 0..C-1 other than g stay what they are to the AllValid kernels: no class (t = 0 in every region sum, counted in
// Sp), CE weight 1.
#pragma once
#include "asis_common.h"
#include "bilinear_tap.h"  // MAXC, Tap, tap_ac_false, sample_logits, softmax_c, softmax_bwd_c

namespace {

// every pixel of every sample takes part
struct AllValid {
  static constexpr bool on = false;
};
// a pixel takes part where its label is not g; `valid`: int32 [B], written by the finalize kernel and read by the backward
struct IgnoreLabel {
  static constexpr bool on = true;
  int g;
  int* valid;
};

template <typename V> constexpr int seg_loss_extra() { return V::on ? 1 : 0; }  // partials per (b, block) beside the C*3 + 2 sums

// One generalised pass for every loss of segloss/: with x0 = resized logits, x1 = softmax(x0), x2 = softmax(x1)
//   region term on q = x_{n_region}:  per (b, c) sums I = sum q t, Sp = sum q, St = sum t   (tp = I, fp = Sp - I, fn = St - I)
//   CE term (n_ce >= 1): nll = -log softmax(x_{n_ce-1})[t], weighted mean with optional class weights
// partial[(b * nblk + blk) * PS + {c*3 + {0,1,2}: I, Sp, St ; C*3: sum w nll ; C*3+1: sum w ; (IgnoreLabel) C*3+2: valid pixels}]
// PS = C*3 + 2 (+ 1 with IgnoreLabel)
template <typename V>
__global__ __launch_bounds__(256) void seg_loss_fwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                           const float* __restrict__ ce_w, int h, int w, int H, int W, int C,
                                                           int n_region, int n_ce, float* __restrict__ partial, const V pol) {
  __shared__ float red[4][MAXC * 3 + 2];
  __shared__ int redn[V::on ? 4 : 1];
  const int b = blockIdx.y, nblk = gridDim.x;
  const float* lg = logits + (int64_t)b * h * w * C;
  const int64_t* tg = target + (int64_t)b * H * W;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  float acc[MAXC * 3 + 2];
#pragma unroll
  for (int i = 0; i < MAXC * 3 + 2; ++i) acc[i] = 0.f;
  int nv = 0;
  const int npix = H * W;
  const int nmax = n_region > n_ce ? n_region : n_ce;
  [[maybe_unused]] int tnext = 0;  // IgnoreLabel: the label of the thread's next pixel, loaded one trip ahead
  if constexpr (V::on) {
    const int p0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (p0 < npix) tnext = (int)tg[p0];
  }
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += nblk * blockDim.x) {
    const int y = p / W, x = p - y * W;
    float z[MAXC];
    [[maybe_unused]] int tcur = 0;
    if constexpr (V::on) {  // the label first: an ignored pixel's logits are not read
      tcur = tnext;
      const int pn = p + nblk * blockDim.x;
      if (pn < npix) tnext = (int)tg[pn];
      if (tcur == pol.g) continue;
      ++nv;
    }
    sample_logits(lg, h, w, C, y, x, sh, sw, z);
    int t;
    if constexpr (V::on) t = tcur;
    else t = (int)tg[p];
    for (int k = 0; k <= nmax; ++k) {
      if (k == n_region) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) {
            const float tt = (t == c) ? 1.f : 0.f;
            acc[c * 3 + 0] += z[c] * tt;
            acc[c * 3 + 1] += z[c];
            acc[c * 3 + 2] += tt;
          }
      }
      if (k + 1 == n_ce) {  // log-sum-exp on the input of the CE's own softmax
        float m = -INFINITY, zt = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) {
            m = fmaxf(m, z[c]);
            if (c == t) zt = z[c];
          }
        float se = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) se += expf(z[c] - m);
        const float wt = (ce_w && t >= 0 && t < C) ? ce_w[t] : 1.f;
        acc[MAXC * 3 + 0] += wt * (logf(se) - (zt - m));
        acc[MAXC * 3 + 1] += wt;
      }
      if (k < nmax) softmax_c(z, C);
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < MAXC * 3 + 2; ++i)
    if (i < C * 3 || i >= MAXC * 3) {
      const float v = wave_sum(acc[i]);
      if (lane == 0) red[wid][i] = v;
    }
  if constexpr (V::on) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o, 64);
    if (lane == 0) redn[wid] = nv;
  }
  __syncthreads();
  const int tx = threadIdx.x;
  constexpr int X = seg_loss_extra<V>();
  if (tx < C * 3 + 2) {
    const int src = tx < C * 3 ? tx : MAXC * 3 + (tx - C * 3);
    partial[((int64_t)b * nblk + blockIdx.x) * (C * 3 + 2 + X) + tx] = (red[0][src] + red[1][src]) + (red[2][src] + red[3][src]);
  }
  if constexpr (V::on) {
    if (tx == C * 3 + 2)
      partial[((int64_t)b * nblk + blockIdx.x) * (C * 3 + 2 + X) + tx] = __int_as_float((redn[0] + redn[1]) + (redn[2] + redn[3]));
  }
}

// sums[b][c][3] (fp32, from double accumulation), loss, and the backward coefficients:
//   coef[(b*C + c)*2 + {0,1}] : d region / d q[b,c,pix] = coef0 * t + coef1     (times grad_scale)
//   coef[B*C*2]               : grad_scale / sum of CE weights (0 without a CE term)
// region modes (all derive from I, Sp, St):
//   0 Dice      segloss/dice.py:27-33            1 - mean 2I/(Sp+St+eps)
//   1 soft IoU  segloss/iou_multi.py:38-49       mean [1 - (I+eps)/(Sp+St-I+eps)]
//   2 SoftDice  segloss/dice_loss.py:255-291     -mean (2I+eps)/(Sp+St+eps)            (2tp+fp+fn = Sp+St)
//   3 Tversky   segloss/dice_loss.py:333-372     -mean (I+eps)/((1-a-b)I + a Sp + b St + eps),  a=.3, b=.7
//   4 none      (CE only, segloss/ND_Crossentropy.py:11-32)
// IgnoreLabel: the mean runs over the pairs of the present samples, see the head of this file.
template <typename V>
__global__ void seg_loss_finalize_kernel(const float* __restrict__ partial, int nblk, int B, int C, float eps, int mode,
                                         int n_ce, float grad_scale, float* __restrict__ sums, float* __restrict__ loss,
                                         float* __restrict__ coef, const V pol) {
  __shared__ double dsum[256];
  __shared__ double ce_tot[2];
  __shared__ int pres[V::on ? 256 : 1];
  const int i = threadIdx.x;  // one thread per (b, c)
  const int PS = C * 3 + 2 + seg_loss_extra<V>();
  [[maybe_unused]] double pairs = 0.0;  // IgnoreLabel: the pairs the mean is taken over, and whether this thread's sample is one
  [[maybe_unused]] bool present = true;
  if constexpr (V::on) {
    if (i < B) {  // B <= B*C <= 256: thread i counts sample i
      int n = 0;
      for (int k = 0; k < nblk; ++k) n += __float_as_int(partial[((int64_t)i * nblk + k) * PS + C * 3 + 2]);
      pol.valid[i] = n;
      pres[i] = n > 0 ? 1 : 0;
    }
    __syncthreads();
    int P = 0;
    for (int k = 0; k < B; ++k) P += pres[k];
    pairs = (double)P * C;
    present = i < B * C && pres[i / C] != 0;
  }
  double term = 0.0;
  if (i < B * C) {
    const int b = i / C, c = i - b * C;
    double s0 = 0, s1 = 0, s2 = 0;
    for (int k = 0; k < nblk; ++k) {
      const float* p = partial + ((int64_t)b * nblk + k) * PS + c * 3;
      s0 += p[0];
      s1 += p[1];
      s2 += p[2];
    }
    if (sums) {
      sums[i * 3 + 0] = (float)s0;
      sums[i * 3 + 1] = (float)s1;
      sums[i * 3 + 2] = (float)s2;
    }
    double bc = (double)B * C;
    if constexpr (V::on) bc = pairs;
    const double e = (double)eps;
    double c0 = 0.0, c1 = 0.0;
    if (V::on && !present) {
      // an absent sample: no term, no gradient
    } else if (mode == 0) {
      const double S = s1 + s2 + e;
      term = 2.0 * s0 / S;
      c0 = -2.0 / (bc * S);
      c1 = 2.0 * s0 / (bc * S * S);
    } else if (mode == 1) {
      const double In = s0 + e, U = s1 + s2 - s0 + e;
      term = In / U;  // d(-In/U)/dq = t * (-(U + In)/U^2) + In/U^2
      c0 = -(U + In) / (U * U) / bc;
      c1 = In / (U * U) / bc;
    } else if (mode == 2) {
      const double Nn = 2.0 * s0 + e, S = s1 + s2 + e;
      term = Nn / S;
      c0 = -2.0 / (bc * S);
      c1 = Nn / (bc * S * S);
    } else if (mode == 3) {
      const double al = 0.3, be = 0.7, g = 1.0 - al - be;
      const double Nn = s0 + e, Dn = g * s0 + al * s1 + be * s2 + e;
      term = Nn / Dn;  // d(-Nn/Dn)/dq = -(t Dn - Nn (g t + al)) / Dn^2
      c0 = -(Dn - Nn * g) / (Dn * Dn) / bc;
      c1 = Nn * al / (Dn * Dn) / bc;
    }
    coef[i * 2 + 0] = (float)(c0 * grad_scale);
    coef[i * 2 + 1] = (float)(c1 * grad_scale);
  }
  dsum[i] = term;
  if (i < 2) {
    double s = 0.0;
    if (n_ce > 0)
      for (int k = 0; k < B * nblk; ++k) s += partial[(int64_t)k * PS + C * 3 + i];
    ce_tot[i] = s;
  }
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (i < o) dsum[i] += dsum[i + o];
    __syncthreads();
  }
  if (i == 0) {
    if constexpr (V::on) {
      double l = 0.0;
      if (pairs > 0.0) {
        const double mean = dsum[0] / pairs;
        l = (mode == 0 || mode == 1) ? 1.0 - mean : (mode == 4 ? 0.0 : -mean);
      }
      const bool ce = n_ce > 0 && ce_tot[1] > 0.0;  // no valid pixel with a weight: no CE term, no CE gradient
      if (ce) l += ce_tot[0] / ce_tot[1];
      *loss = (float)l;
      coef[B * C * 2] = ce ? (float)((double)grad_scale / ce_tot[1]) : 0.f;
    } else {
      const double mean = dsum[0] / ((double)B * C);
      double l = (mode == 0 || mode == 1) ? 1.0 - mean : (mode == 4 ? 0.0 : -mean);
      if (n_ce > 0) l += ce_tot[0] / ce_tot[1];
      *loss = (float)l;
      coef[B * C * 2] = n_ce > 0 ? (float)((double)grad_scale / ce_tot[1]) : 0.f;
    }
  }
}

// dz[b, y, x, c] = d loss / d (resized logits), fp32 at (H, W)
template <typename V>
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const float* __restrict__ logits, const int64_t* __restrict__ target,
                                                           const float* __restrict__ coef, const float* __restrict__ ce_w,
                                                           int B, int h, int w, int H, int W, int C, int n_region, int n_ce,
                                                           int mode, float* __restrict__ dz, const V pol) {
  const int b = blockIdx.y;
  const float* lg = logits + (int64_t)b * h * w * C;
  const int64_t* tg = target + (int64_t)b * H * W;
  float* out = dz + (int64_t)b * H * W * C;
  const float sh = (float)h / (float)H, sw = (float)w / (float)W;
  const int npix = H * W;
  if constexpr (V::on) {
    if (pol.valid[b] == 0) {  // no label in this sample: zeros, and neither its logits nor its labels are read
      for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)npix * C; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = 0.f;
      return;
    }
  }
  const float ce_scale = coef[B * C * 2];
  const int nmax = n_region > n_ce ? n_region : n_ce;
  [[maybe_unused]] int tnext = 0;
  if constexpr (V::on) {
    const int p0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (p0 < npix) tnext = (int)tg[p0];
  }
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
    const int y = p / W, x = p - y * W;
    float p1[MAXC], p2[MAXC];
    [[maybe_unused]] int tcur = 0;
    if constexpr (V::on) {
      tcur = tnext;
      const int pn = p + gridDim.x * blockDim.x;
      if (pn < npix) tnext = (int)tg[pn];
      if (tcur == pol.g) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c)
          if (c < C) out[(int64_t)p * C + c] = 0.f;
        continue;
      }
    }
    sample_logits(lg, h, w, C, y, x, sh, sw, p1);
    if (nmax >= 1) softmax_c(p1, C);
#pragma unroll
    for (int c = 0; c < MAXC; ++c) p2[c] = p1[c];
    if (nmax >= 2) softmax_c(p2, C);
    int t;
    if constexpr (V::on) t = tcur;
    else t = (int)tg[p];
    float r[MAXC];  // region gradient wrt q
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      r[c] = (c < C && mode != 4) ? coef[(b * C + c) * 2 + 0] * ((t == c) ? 1.f : 0.f) + coef[(b * C + c) * 2 + 1] : 0.f;
    const float cw = n_ce > 0 ? ce_scale * ((ce_w && t >= 0 && t < C) ? ce_w[t] : 1.f) : 0.f;
    float g[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) g[c] = 0.f;
    if (nmax >= 2) {  // level x1: softmax2 backward of the region term + region at x1 + CE over softmax(x1)
      if (n_region == 2) {
#pragma unroll
        for (int c = 0; c < MAXC; ++c) g[c] = r[c];
        softmax_bwd_c(g, p2, C);
      }
#pragma unroll
      for (int c = 0; c < MAXC; ++c)
        if (c < C) {
          if (n_region == 1) g[c] += r[c];
          if (n_ce == 2) g[c] += cw * (p2[c] - ((t == c) ? 1.f : 0.f));
        }
      softmax_bwd_c(g, p1, C);
    } else if (nmax == 1 && n_region == 1) {
#pragma unroll
      for (int c = 0; c < MAXC; ++c) g[c] = r[c];
      softmax_bwd_c(g, p1, C);
    }
#pragma unroll
    for (int c = 0; c < MAXC; ++c)
      if (c < C) {
        if (n_region == 0) g[c] += r[c];
        if (n_ce == 1) g[c] += cw * (p1[c] - ((t == c) ? 1.f : 0.f));
        out[(int64_t)p * C + c] = g[c];
      }
  }
}

// The argument checks, under the name `op`, and the launches of asis_seg_loss_fwd (AllValid) and of the forward half of
// asis_semi_loss (IgnoreLabel).  partial: asis_dice_nblk(H, W) * B * (C*3 + 2 + seg_loss_extra<V>()) floats.
template <typename V>
int seg_loss_fwd_launch(const char* op, V pol, void* stream, const float* logits, const int64_t* target, const float* ce_weight,
                        int B, int h, int w, int H, int W, int C, int n_region, int mode, float eps, int n_ce, float grad_scale,
                        float* partial, float* sums, float* loss, float* coef) {
  ASIS_REQUIRE(logits && target && partial && loss && coef, "%s: null pointer", op);
  ASIS_REQUIRE(C >= 1 && C <= MAXC, "%s: C=%d must be in 1..%d", op, C, MAXC);
  ASIS_REQUIRE(B * C <= 256 && B <= 65535, "%s: B*C=%d must be <= 256", op, B * C);
  ASIS_REQUIRE(n_region >= 0 && n_region <= 2, "%s: n_region must be 0, 1 or 2", op);
  ASIS_REQUIRE(n_ce >= 0 && n_ce <= 2, "%s: n_ce must be 0 (no CE term), 1 or 2", op);
  ASIS_REQUIRE(mode >= 0 && mode <= 4, "%s: mode must be 0..4", op);
  ASIS_REQUIRE(mode != 4 || n_ce > 0, "%s: mode 4 (no region term) needs a CE term", op);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int nblk = asis_dice_nblk(H, W);
  hipLaunchKernelGGL(seg_loss_fwd_kernel<V>, dim3(nblk, B), dim3(256), 0, s, logits, target, ce_weight, h, w, H, W, C, n_region,
                     n_ce, partial, pol);
  hipLaunchKernelGGL(seg_loss_finalize_kernel<V>, dim3(1), dim3(256), 0, s, partial, nblk, B, C, eps, mode, n_ce, grad_scale,
                     sums, loss, coef, pol);
  ASIS_CHECK_LAUNCH(op);
  return ASIS_OK;
}

template <typename V>
int seg_loss_bwd_launch(const char* op, V pol, void* stream, const float* logits, const int64_t* target, const float* coef,
                        const float* ce_weight, int B, int h, int w, int H, int W, int C, int n_region, int mode, int n_ce,
                        float* dz) {
  ASIS_REQUIRE(logits && target && coef && dz, "%s: null pointer", op);
  ASIS_REQUIRE(C >= 1 && C <= MAXC && n_region >= 0 && n_region <= 2 && n_ce >= 0 && n_ce <= 2 && mode >= 0 && mode <= 4,
               "%s: bad C / n_region / n_ce / mode", op);
  hipLaunchKernelGGL(seg_loss_bwd_kernel<V>, dim3(asis_dice_nblk(H, W), B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     logits, target, coef, ce_weight, B, h, w, H, W, C, n_region, n_ce, mode, dz, pol);
  ASIS_CHECK_LAUNCH(op);
  return ASIS_OK;
}

}  // namespace
