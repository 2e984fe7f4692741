/* libmopoe_hip.so -- optimiser ABI beside mopoe_adam_step: the exponential moving average of the weights of `--ema_decay`.
 *
 * An average of every parameter tensor, kept on the device and updated once per optimiser step right behind the Adam
 * launch that wrote the tensor, and an in-place exchange of the averaged with the live weights for evaluation and for
 * the `<mm_vae_save>_ema` checkpoint.  The reference has no such option (an extension of this project, like
 * --max_grad_norm).  Compiled from csrc/ema.hip into the same library as include/mopoe_hip.h; the Adam kernels of
 * csrc/adam.hip are not involved.
 *
 * Conventions: those of include/mopoe_hip_optim.h.  The records are a HOST array and travel in the kernel arguments, 64
 * per launch; every other pointer is a DEVICE pointer into caller-owned memory; the library never allocates, frees or
 * retains a pointer past return; work is enqueued on the caller's `stream` (a hipStream_t passed as void*), no host sync
 * inside, no atomics; return 0 on success, a negative code on error (MOPOE_ERR_* of include/mopoe_hip.h; the last-error
 * text says why); every refusal comes before the first launch, so a refused call writes nothing; nothing throws across
 * the ABI.  One block owns one 4096-element chunk of one record; 16-byte loads and stores where every pointer of the
 * record is 16-byte aligned (p16: 8-byte), one element per access otherwise.
 */
#ifndef MOPOE_HIP_EMA_H
#define MOPOE_HIP_EMA_H

#include <stddef.h>
#include <stdint.h>

#include "mopoe_hip.h"
#include "mopoe_hip_optim.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One tensor: the live parameter, its average, and (swap only) the bf16 copy of the parameter a bf16-family layer reads. */
typedef struct {
  float* p;      /* [n] fp32 parameter */
  float* ema;    /* [n] fp32 average */
  uint16_t* p16; /* [n] bf16 copy of p, or NULL */
  int64_t n;     /* elements; a record with n == 0 takes no part */
} mopoe_ema_seg;

/* ---- update ---------------------------------------------------------------------------------------------------------
 * Reads p, reads and writes ema; p16 is ignored.  `step` is Adam's device step counter AFTER this step's increment
 * (mopoe_adam_step's `step`), read on the device, so the call is capturable.  The arithmetic is fixed:
 *   s = step[0]
 *   d = min(decay, (1 + s) / (10 + s))      in double: the usual warm-up, which keeps the initial weights from lingering
 *   w = (float)(1.0 - d)
 *   ema = fmaf(w, p - ema, ema)             in float
 * clip_state != NULL (the state of mopoe_grad_norm) and clip_state[MOPOE_CLIP_SKIP] != 0: no store is issued at all -- a
 * step that --max_grad_norm skipped does not move the average.
 * A non-finite element of p makes that one element of ema non-finite and touches nothing else.
 * MOPOE_ERR_ARG: decay not finite or outside [0, 1); step NULL; segs NULL with nseg > 0; nseg < 0; a record with a NULL
 * p or ema (and n > 0), or n < 0. */
int mopoe_ema_update(const mopoe_ema_seg* segs, int32_t nseg, double decay, const float* step,
                     const float* clip_state /* may be NULL */, void* stream);

/* ---- swap -----------------------------------------------------------------------------------------------------------
 * Per element, bits preserved: tmp = p, p = ema, ema = tmp; where p16 != NULL, p16 = bf16(new p) with the rounding of
 * mopoe_adam_step (round to nearest even).  Two calls are the identity, bit for bit, on p, ema and p16 (given that p16
 * held bf16(p) before the first).  In place, not by pointer: a captured train step has the parameter addresses in its
 * nodes.  MOPOE_ERR_ARG as above. */
int mopoe_ema_swap(const mopoe_ema_seg* segs, int32_t nseg, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOPOE_HIP_EMA_H */
