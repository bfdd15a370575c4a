/* C ABI of libasis_semi.so (adaptersis_amd/csrc/semi.hip), a library beside libasis_hip.so: return codes, error text
 * (asis_last_error) and conventions are those of asis_hip.h; gfx950 only.
 *
 * The fused segmentation loss of asis_seg_loss_fwd / asis_seg_loss_bwd with an ignore label, for batches that hold unlabelled or
 * partly labelled frames.  logits, target, ce_weight, B, h, w, H, W, C, n_region, mode, eps, n_ce, grad_scale as there; the
 * kernels are the same bodies (csrc/seg_loss_body.h) instantiated with the policy IgnoreLabel.  With g = ignore_index:
 *   v_i = [target_i != g];  n_b = sum_{i in b} v_i;  sample b is PRESENT when n_b > 0;  P = the number of present samples.
 *   sums [B,C,3]: I = sum v q t, Sp = sum v q, St = sum v t per (b, c), q = softmax^{n_region}(resize(logits)).
 *   region term: the five mode formulas of asis_seg_loss_fwd with the mean taken over the P*C pairs of the present samples: P*C
 *     replaces B*C in the loss and in coef, the coef of an absent sample is 0, P = 0 gives a region term of exactly 0.
 *   CE term: sum v w_t nll / sum v w_t; exactly 0, with a CE scale (coef[B*C*2]) of 0, where the denominator is 0.  Nothing is NaN.
 *   valid int32 [B] = n_b, exact.
 *   dz fp32 [B,H,W,C] = d loss / d resized logits times grad_scale; all bits zero on every ignored pixel.
 *   The forward does not sample the logits of an ignored pixel (it reads its 8-byte label only); the backward of a sample with
 *     n_b = 0 writes zeros and reads neither its logits nor its labels.  Logits of such pixels may hold anything, NaN included.
 *   Labels outside 0..C-1 other than g are what they are to asis_seg_loss_fwd: valid pixels of no class (CE weight 1).
 *   partial: asis_dice_nblk(H, W) * B * asis_semi_partial_stride(C) floats owned by the caller; coef: B*C*2 + 1 floats.
 *   Forward, finalize and backward are launched by the one call, in that order on `stream`.
 *   ignore_index must lie outside 0..C-1.  C <= 16, B*C <= 256; deterministic (the order of sums of asis_seg_loss_fwd), no atomics,
 *   no host sync. */
#ifndef ASIS_SEMI_H
#define ASIS_SEMI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int asis_semi_partial_stride(int C);
int asis_semi_loss(void* stream, const float* logits, const int64_t* target, const float* ce_weight, int B, int h, int w, int H,
                   int W, int C, int ignore_index, int n_region, int mode, float eps, int n_ce, float grad_scale, float* partial,
                   float* sums, float* loss, float* coef, int32_t* valid, float* dz);
#ifdef __cplusplus
}
#endif
#endif
