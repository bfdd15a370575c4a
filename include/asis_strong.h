/* C ABI of libasis_strong.so (adaptersis_amd/csrc/strongaug.hip), a library beside libasis_hip.so: return codes, error text
 * (asis_last_error) and conventions are those of asis_hip.h; gfx950 only.
 *
 * The strong student view of semi-supervised training: colour jitter, greyscale and Gaussian blur on x fp32 [B,3,H,W] in [0,1]
 * (the output of asis_augment).  Per-sample tables on the device:
 *   ops   int32 [B,4]: operation codes in the order they run: 0 brightness, 1 contrast, 2 saturation, 3 hue; any other value
 *                      (-1) is no operation.  Contrast is expected at most once per sample (every occurrence uses the same mean).
 *   fac   fp32  [B,4]: the factor of each.  With grey(x) = 0.2989 r + 0.587 g + 0.114 b and every result clamped to [0,1]:
 *                        brightness x f;  contrast f x + (1 - f) m, m = the mean of grey over the sample as it stands when contrast
 *                        is reached;  saturation f x + (1 - f) grey(x);  hue RGB -> HSV (max / min form; a grey pixel stays
 *                        itself), h <- (h + f) mod 1, HSV -> RGB.
 *   flags int32 [B,2]: (grey, radius).  grey != 0: the three channels become grey(x) after the jitter.  radius r in 1..6: a
 *                      separable Gaussian blur with a reflect border (no edge repeat) runs last, its result clamped to [0,1];
 *                      a radius outside 0..6 or >= min(H, W) is read as 0 (callers check their host copy).
 *   gauss fp32  [B,13]: the taps, centred (index 6 is the middle), used at 6 - r .. 6 + r.
 *   apply int32 [B] or NULL: a sample with apply == 0 is copied through, like a sample without any operation: copies of bits.
 *
 * asis_strong_mean: for every sample with a contrast operation (and apply != 0), the sum of grey over the image under the operations
 *   in front of contrast, applied on the fly -> partial double [B, nblk], nblk = asis_strong_nblk(H * W): workgroup j of a sample
 *   sums the pixels [j, j + 1) * asis_strong_chunk() in double, in a fixed order (a thread's items, an xor tree over the wave, the
 *   4 waves in index order).  Rows of other samples are not written.  Needed only when some sample has a contrast operation.
 * asis_strong_view: x -> out (must not overlap x), one read and one write of the image.  partial: what asis_strong_mean wrote, or
 *   NULL when no sample has a contrast operation (contrast then runs with m = 0); a workgroup adds the nblk partials of its sample
 *   in index order.  A workgroup owns a 32 x 32 output tile of one sample; a sample with a blur is staged with its halo in LDS
 *   (max_radius: the largest radius of the batch, 0..6, sizes the LDS of the launch; a larger radius in the table is read as 0).
 *   16-byte accesses on the path without blur when W % 4 == 0 and both pointers are 16-byte aligned.
 * No host sync, no atomics: every result is bit-identical from call to call.  H, W >= 1, B * 3 * H * W < 2^31, B <= 65535. */
#ifndef ASIS_STRONG_H
#define ASIS_STRONG_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int asis_strong_chunk(void);
int asis_strong_nblk(int64_t HW);
int asis_strong_mean(void* stream, const float* x, const int* ops, const float* fac, const int* apply, int B, int H, int W,
                     double* partial);
int asis_strong_view(void* stream, const float* x, const int* ops, const float* fac, const int* flags, const float* gauss,
                     const int* apply, const double* partial, int max_radius, int B, int H, int W, float* out);
#ifdef __cplusplus
}
#endif
#endif
