/* libmopoe_hip.so -- optimiser ABI beside mopoe_adam_step: the global gradient-norm clip of `--max_grad_norm`.
 *
 * torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2) in front of the Adam step, on the device and capturable:
 *   total_norm = sqrt(sum of g^2 over every element of every record that has a gradient)
 *   scale      = min(1, max_norm / (total_norm + 1e-6))
 *   the Adam update uses scale * g.
 * Two deliberate differences from torch: the gradients are NOT rewritten (the scale is applied where the Adam kernel loads
 * them; the norm reported is the one before clipping, as torch's return value is), and a total_norm that is not finite
 * SKIPS the update on the device instead of multiplying everything by NaN (below).
 * Compiled from csrc/adam.hip into the same library as include/mopoe_hip.h, whose mopoe_adam_seg records both calls take.
 *
 * Conventions: those of include/mopoe_hip.h.  The records are a HOST array and travel in the kernel arguments, 64 per
 * launch; every other pointer is a DEVICE pointer into caller-owned memory; the library never allocates, frees or retains
 * a pointer past return; work is enqueued on the caller's `stream` (a hipStream_t passed as void*), no host sync inside;
 * return 0 on success, a negative code on error (MOPOE_ERR_* of include/mopoe_hip.h; the last-error text says why);
 * nothing throws across the ABI.
 */
#ifndef MOPOE_HIP_OPTIM_H
#define MOPOE_HIP_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#include "mopoe_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The clip state: float[4] on the device, written by mopoe_grad_norm, read by mopoe_adam_step_clipped. */
#define MOPOE_CLIP_NORM 0          /* total_norm of this step, before clipping (may be inf / NaN) */
#define MOPOE_CLIP_SCALE 1         /* min(1, max_norm / (total_norm + 1e-6)); exactly 1 when nothing is clipped; 0 with skip */
#define MOPOE_CLIP_SKIP 2          /* 1 if total_norm is not finite: the clipped Adam step changes nothing; else 0 */
#define MOPOE_CLIP_SKIPPED_TOTAL 3 /* += skip on every call (the caller zeroes it once); exact up to 2^24 */
#define MOPOE_CLIP_STATE_LEN 4

/* ---- scratch size -------------------------------------------------------------------------------------------------
 * The number of doubles of scratch that suffices for mopoe_grad_norm over these records, whichever of them have a
 * gradient: one per 4096-element chunk of every record with n > 0 (the g pointers are not looked at, so the caller can
 * size the buffer once, before any gradient exists).  Host arithmetic only.  A negative code on bad arguments. */
int64_t mopoe_grad_norm_partials(const mopoe_adam_seg* segs, int32_t nseg);

/* ---- norm, scale and skip decision ----------------------------------------------------------------------------------
 * Reads only .g and .n of each record; a record with g == NULL or n == 0 contributes nothing; with no gradient at all the
 * norm is 0 and the scale 1.  Every element is converted to double BEFORE it is squared and all sums are carried in
 * double (a gradient of 1e20 gives a finite norm), rounded to float once for the state.
 * Deterministic: one block per 4096-element chunk sums its chunk in a fixed order and stores ONE double into
 * scratch[chunk number] (chunks numbered in record order); a last single-block launch adds the partials -- thread t takes
 * t, t + 256, ... in index order, then a fixed tree over the 256 threads -- and writes the four floats of `state`.  No
 * floating-point atomics, no inter-block hand-off inside a launch.  16-byte loads where g is 16-byte aligned, one float
 * per load otherwise.
 * skip = 1 when the float norm is not finite (an inf or NaN gradient, or a norm beyond the float range).
 * scratch: double[scratch_len], scratch_len >= the chunks of the records that HAVE a gradient (mopoe_grad_norm_partials
 * gives an upper bound); max_norm: finite, >= 0. */
int mopoe_grad_norm(const mopoe_adam_seg* segs, int32_t nseg, double max_norm, double* scratch, int64_t scratch_len,
                    float* state, void* stream);

/* ---- the Adam step of include/mopoe_hip.h under a clip state --------------------------------------------------------
 * mopoe_adam_step with one more argument.  state[MOPOE_CLIP_SKIP] != 0: the step counter, `coef`, and every p, m, v and
 * p16 stay exactly as they are (no store is issued).  Otherwise every gradient is multiplied by state[MOPOE_CLIP_SCALE]
 * in float where it is loaded; with a scale of exactly 1 the results equal mopoe_adam_step's bit for bit. */
int mopoe_adam_step_clipped(const mopoe_adam_seg* segs, int32_t nseg, float* step, const float* lr_dev, double lr,
                            double beta1, double beta2, double eps, float* coef, const float* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOPOE_HIP_OPTIM_H */
