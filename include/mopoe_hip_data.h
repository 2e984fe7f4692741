/* libmopoe_hip.so -- input-pipeline ABI: the label-weighted training batches of `--weighted_sampler`.
 *
 * The reference draws training rows on the host (mimic/dataio/utils.py:126-133: WeightedRandomSampler over
 * calculateWeights, with replacement) and converts every sample with ToTensor in DataLoader workers.  Here a split lives
 * in HBM (mimic_amd/dataio/MimicDataset.py: DeviceResidentMimic), so the rows of an epoch are drawn on the device and a
 * batch is gathered and converted by one launch.  Compiled from csrc/batch.hip into the same library as include/mopoe_hip.h.
 *
 * Conventions: those of include/mopoe_hip.h.  Plain pointers and sizes only; every pointer is a DEVICE pointer into
 * caller-owned memory; the library never allocates, frees or retains a pointer past return; work is enqueued on the
 * caller's `stream` (a hipStream_t passed as void*), no host sync inside; return 0 on success, a negative code on error
 * (MOPOE_ERR_* of include/mopoe_hip.h; mopoe_last_error() gives the text); nothing throws across the ABI.
 */
#ifndef MOPOE_HIP_DATA_H
#define MOPOE_HIP_DATA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- weighted draws with replacement ------------------------------------------------------------------------------
 * out[i - first] for first <= i < first + count: the row that draw number i of (seed, epoch, rank) selects.  A draw is a
 * pure function of (seed, epoch, rank, i): it depends neither on the grid nor on `first` / `count`, so an epoch may be
 * drawn in one call or in pieces.
 *
 * Generator: Philox4x32-10 (Salmon et al., SC'11; multipliers 0xD2511F53, 0xCD9E8D57, key increments 0x9E3779B9,
 * 0xBB67AE85) with key = (seed & 0xffffffff, seed >> 32) and counter = (i & 0xffffffff, i >> 32, epoch, rank).  Of the
 * output words x0..x3:  u = ((x0 >> 5) * 2^26 + (x1 >> 6)) * 2^-53, a double in [0, 1).
 *
 * cdf: double[n], the INCLUSIVE prefix sum of the rows' weights in row order (non-decreasing, cdf[n-1] > 0 and finite),
 * summed by the caller: the kernel never sums.  With t = u * cdf[n-1] the draw is the first j with cdf[j] > t
 * (searchsorted(cdf, t, side='right')), clamped to n - 1: a row of weight zero is never drawn.
 * One thread per draw: a binary search over global memory with fp64 compares.
 * n >= 1, first >= 0, count >= 0 (count == 0: nothing is launched). */
int mopoe_batch_draw(const double* cdf, int64_t n, uint64_t seed, uint32_t epoch, uint32_t rank,
                     int64_t first, int64_t count, int64_t* out, void* stream);

/* ---- one training batch out of a resident split --------------------------------------------------------------------
 * pa, lat: uint8 [n, S, S] images; text: [n, L] class ids (text_kind 0: int32 token ids; 1: uint8 alphabet positions);
 * labels: float [n, n_labels]; sel: int64 [B] row numbers.  One launch writes, for b < B and r = sel[b]:
 *   out_pa, out_lat [B, 1, S, S]   (float)u8 / 255.0f, the division correctly rounded (torchvision's ToTensor; the value
 *                                  u8.float() / 255 has on the CPU -- not a multiplication by a rounded reciprocal)
 *   out_text  text_kind 0: [B, L] the ids as floats;  text_kind 1: [B, L, F] one-hot rows, EVERY element written
 *                                  (1.0f at the position, 0.0f elsewhere; a position >= F leaves its row all zero)
 *   out_labels [B, n_labels]
 * A sel value outside [0, n) is CLAMPED into range (negative -> row 0, >= n -> row n - 1): whatever sel holds, the
 * kernel reads inside the n rows of its inputs and writes inside its B output rows.
 * No alignment is required.  Image rows are moved as 16-byte loads and four 16-byte stores per load when S * S is a
 * multiple of 16 and pa, lat, out_pa, out_lat are 16-byte aligned; one element per work item otherwise.
 * n >= 1, S >= 1, L >= 1, n_labels >= 1, B >= 1, F >= 1 with text_kind 1 (ignored with 0); the number of output
 * elements, 2 * B * S * S + B * L * (F or 1) + B * n_labels, must stay below 2^31 (n * S * S may exceed it). */
int mopoe_batch_assemble(const uint8_t* pa, const uint8_t* lat, int64_t n, int32_t S,
                         const void* text, int32_t text_kind /*0: int32 token ids, 1: uint8 alphabet positions*/,
                         int32_t L, int32_t F /*one-hot width, text_kind 1 only*/,
                         const float* labels, int32_t n_labels, const int64_t* sel, int32_t B,
                         float* out_pa, float* out_lat, float* out_text, float* out_labels, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOPOE_HIP_DATA_H */
