/* C ABI of libasis_mix.so (adaptersis_amd/csrc/mix.hip), a library beside libasis_hip.so, libasis_distill.so and
 * libasis_consist.so: return codes, error text (asis_last_error) and conventions are those of asis_hip.h; gfx950 only.
 *
 * CutMix / ClassMix over the samples of one batch: sample b receives pixels of sample donor[b].  The tables live on the device:
 *   donor int32 [B]: the sample b takes pixels from.  A value outside 0..B-1 is read as b (it never becomes an address); callers
 *     check their host copy.
 *   kind  int32 [B]: 0 not mixed, 1 CutMix, 2 ClassMix; any other value is 0.
 *   box   int32 [B,4]: (y0, x0, y1, x1), half-open, of kind 1; clipped to the frame by the comparison itself.
 *   order uint8 [B,16]: a permutation of 0..15, the order in which kind 2 picks classes; entries >= C are passed over.
 *
 * asis_mix_class_sets: target int64 [B,H,W] -> sets uint32 [2,B].
 *   sets[0][d] bit c = some pixel of target[d] equals c, 0 <= c < C (labels outside 0..C-1 set nothing).
 *   sets[1][b] = the classes sample b pastes: for kind[b] == 2, with P = sets[0][donor[b]] without bit 0 unless `background`, the
 *     first ceil(|P| / 2) members of P in the order order[b]; 0 for every other kind and for an empty P.
 * asis_mix_apply: inp fp32 [B,3,H,W], target int64 [B,H,W] -> inp_out, target_out of the same shapes, sel uint8 [B,H,W],
 *   pasted int32 [B].  None of the outputs may alias an input.  Per pixel (y, x) of sample b with d = donor[b]:
 *     sel = 1 inside the box (kind 1), 1 where target[d](y, x) is a bit of pasted_sets[b] (kind 2), else 0;
 *     inp_out[b] = sel ? inp[d] : inp[b] for the three planes, target_out[b] likewise: copies of bits;
 *     pasted[b] = the number of pixels with sel = 1 (exact: integers).
 *   pasted_sets: sets[1] of asis_mix_class_sets, or NULL when no sample has kind 2 (kind 2 then pastes nothing).  The donor's image
 *   is read only where sel is set, and sample b's only where it is not (in units of 4 pixels of a row on the 16-byte path, taken
 *   when W % 4 == 0 and every pointer is 16-byte aligned).
 *   asis_mix_tile(): pixels of one sample a workgroup handles per pass; asis_mix_nblk(B, HW): the workgroups of the launch for B
 *   samples of HW pixels (callable without a GPU; -1 for B < 1, HW < 1 or B*HW >= 2^31).
 * asis_mix_consist_loss: asis_consist_loss of asis_consist.h over a mixed batch.  sel uint8 [B,H,W] and donor int32 [B] on the
 *   device: for pixel i of sample b the student is read from sample b, every teacher map from sample (sel[i] ? donor[b] : b) at the
 *   same (y, x) and through the same flips.  Everything else is that header's, to the letter: the gate on the confidence of the mixed
 *   q, sample_weight[b] of the destination (a sample of weight 0 reads neither its own maps nor its donor's, nor sel), kept, the
 *   normalisation by N, the accumulation into dz, the two doubles per workgroup.  asis_mix_consist_tile / asis_mix_consist_nblk are
 *   asis_consist_tile / asis_consist_nblk.
 * No host sync, no float atomics; every result is bit-identical from call to call.  C <= 16, B*H*W < 2^31. */
#ifndef ASIS_MIX_H
#define ASIS_MIX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int asis_mix_tile(void);
int asis_mix_nblk(int B, int64_t HW);
int asis_mix_class_sets(void* stream, const int64_t* target, const int* donor, const int* kind, const uint8_t* order, int B, int H,
                        int W, int C, int background, uint32_t* sets);
int asis_mix_apply(void* stream, const float* inp, const int64_t* target, const int* donor, const int* kind, const int* box,
                   const uint32_t* pasted_sets, int B, int H, int W, float* inp_out, int64_t* target_out, uint8_t* sel, int* pasted);
int asis_mix_consist_tile(void);
int asis_mix_consist_nblk(int64_t N);
int asis_mix_consist_loss(void* stream, const float* logits, int B, int h, int w, const float* const* teachers, const int* hs,
                          const int* ws, const int* flips, int V, int H, int W, int C, float temperature, float threshold,
                          const float* sample_weight, const uint8_t* sel, const int* donor, float grad_scale, int accumulate,
                          double* partial, float* loss, int* kept, float* dz);
#ifdef __cplusplus
}
#endif
#endif
