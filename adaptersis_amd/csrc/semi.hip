// The hard loss of semi-supervised training: the fused segmentation loss of loss.hip with an ignore label.  Built into
// libasis_semi.so (build.py SIDE_LIBS; ABI in include/asis_semi.h), beside libasis_hip.so, whose error plumbing and
// asis_dice_nblk it uses.  The kernels are seg_loss_body.h's, the ones loss.hip launches, instantiated with IgnoreLabel; the
// arithmetic is documented in loss.hip, what the label changes at the head of seg_loss_body.h.  A frame without labels is a
// sample whose target is the ignore value throughout: its logits are read by neither pass, it is left out of the mean of the
// region term, and its dz is zeros.
#include "../../include/asis_semi.h"
#include "seg_loss_body.h"

extern "C" int asis_semi_partial_stride(int C) { return C * 3 + 2 + seg_loss_extra<IgnoreLabel>(); }

extern "C" int asis_semi_loss(void* stream, const float* logits, const int64_t* target, const float* ce_weight, int B, int h, int w,
                              int H, int W, int C, int ignore_index, int n_region, int mode, float eps, int n_ce, float grad_scale,
                              float* partial, float* sums, float* loss, float* coef, int32_t* valid, float* dz) {
  const char* op = "asis_semi_loss";
  ASIS_REQUIRE(valid && dz, "%s: null pointer", op);
  ASIS_REQUIRE(B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1, "%s: non-positive size B=%d h=%d w=%d H=%d W=%d", op, B, h, w, H, W);
  ASIS_REQUIRE(ignore_index < 0 || ignore_index >= C, "%s: ignore_index=%d must lie outside the classes 0..%d", op, ignore_index,
               C - 1);
  const IgnoreLabel pol{ignore_index, valid};
  if (int rc = seg_loss_fwd_launch(op, pol, stream, logits, target, ce_weight, B, h, w, H, W, C, n_region, mode, eps, n_ce,
                                   grad_scale, partial, sums, loss, coef))
    return rc;
  return seg_loss_bwd_launch(op, pol, stream, logits, target, coef, ce_weight, B, h, w, H, W, C, n_region, mode, n_ce, dz);
}
