// Input pipeline of --weighted_sampler (include/mopoe_hip_data.h): the rows of an epoch drawn on the device, and a training
// batch gathered out of the resident split and converted to floats by one launch.  Both are glue: no LDS, no tuned plan.
#include "common.hpp"
#include "batch_draw.hpp"
#include "../../include/mopoe_hip_data.h"

namespace mopoe {

// one thread per draw: Philox4x32-10 on (seed; i, epoch, rank), then a binary search of t = u * cdf[n-1] in the prefix sums
// (<= 18 dependent loads at MIMIC's row counts; the table of an epoch's threads is the same n doubles, L2 resident)
__global__ __launch_bounds__(256) void batch_draw_kernel(const double* __restrict__ cdf, long n, uint64_t seed, uint32_t epoch,
                                                         uint32_t rank, long first, long count, int64_t* __restrict__ out) {
  const double total = cdf[n - 1];
  for (long d = (long)blockIdx.x * 256 + threadIdx.x; d < count; d += (long)gridDim.x * 256) {
    const double u = draw_uniform(seed, epoch, rank, (uint64_t)(first + d));
    out[d] = first_above(cdf, n, u * total);
  }
}

__device__ __forceinline__ long clamp_row(long r, long n) { return r < 0 ? 0 : (r >= n ? n - 1 : r); }

// (float)u8 / 255.0f with the division correctly rounded: what ToTensor and a CPU u8.float() / 255 give
__device__ __forceinline__ float4 bytes_to_unit(unsigned w) {
  float4 f;
  f.x = (float)(w & 0xffu) / 255.0f;
  f.y = (float)((w >> 8) & 0xffu) / 255.0f;
  f.z = (float)((w >> 16) & 0xffu) / 255.0f;
  f.w = (float)(w >> 24) / 255.0f;
  return f;
}

// Work items of one grid, in this order: the PA image rows, the Lateral image rows (VEC: one 16-byte piece of a row each,
// else one pixel each), then one item per text output element, then one per label element; grid-stride over all of them.
template <bool VEC>
__global__ __launch_bounds__(256) void batch_assemble_kernel(const uint8_t* __restrict__ pa, const uint8_t* __restrict__ lat, long n,
                                                             unsigned SS, const void* __restrict__ text, int text_kind, unsigned L,
                                                             unsigned F, const float* __restrict__ labels, unsigned n_labels,
                                                             const int64_t* __restrict__ sel, unsigned B, float* __restrict__ out_pa,
                                                             float* __restrict__ out_lat, float* __restrict__ out_text,
                                                             float* __restrict__ out_labels) {
  const unsigned per_img = VEC ? SS / 16 : SS;      // items per image row
  const unsigned n_img = B * per_img;
  const unsigned text_row = text_kind == 0 ? L : L * F;
  const unsigned n_text = B * text_row;
  const unsigned total = 2 * n_img + n_text + B * n_labels;      // (< 2^31: checked by the launcher)
  for (unsigned w = blockIdx.x * 256u + threadIdx.x; w < total; w += gridDim.x * 256u) {
    if (w < 2 * n_img) {
      const bool second = w >= n_img;
      const unsigned i = second ? w - n_img : w;
      const unsigned b = i / per_img, c = i - b * per_img;
      const uint8_t* src = (second ? lat : pa) + clamp_row(sel[b], n) * (long)SS;
      float* dst = (second ? out_lat : out_pa) + (long)b * SS;
      if (VEC) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + 16u * c);
        float4* d = reinterpret_cast<float4*>(dst + 16u * c);
        d[0] = bytes_to_unit(v.x);
        d[1] = bytes_to_unit(v.y);
        d[2] = bytes_to_unit(v.z);
        d[3] = bytes_to_unit(v.w);
      } else {
        dst[c] = (float)src[c] / 255.0f;
      }
    } else if (w < 2 * n_img + n_text) {
      const unsigned i = w - 2 * n_img;
      const unsigned b = i / text_row, c = i - b * text_row;
      const long row = clamp_row(sel[b], n);
      if (text_kind == 0) {
        out_text[i] = (float)static_cast<const int32_t*>(text)[row * (long)L + c];
      } else {
        const unsigned l = c / F, f = c - l * F;
        out_text[i] = static_cast<const uint8_t*>(text)[row * (long)L + l] == f ? 1.0f : 0.0f;
      }
    } else {
      const unsigned i = w - 2 * n_img - n_text;
      const unsigned b = i / n_labels, c = i - b * n_labels;
      out_labels[i] = labels[clamp_row(sel[b], n) * (long)n_labels + c];
    }
  }
}

static unsigned glue_grid(long items) {   // memory-bound glue: at most 8 blocks of 256 per CU, the rest by stride
  const long blocks = (items + 255) / 256;
  return (unsigned)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks));
}

}  // namespace mopoe

using namespace mopoe;

extern "C" int mopoe_batch_draw(const double* cdf, int64_t n, uint64_t seed, uint32_t epoch, uint32_t rank, int64_t first,
                                int64_t count, int64_t* out, void* stream) {
  if (!cdf || (count > 0 && !out)) { set_error("batch_draw: null input / output"); return MOPOE_ERR_ARG; }
  if (n < 1 || first < 0 || count < 0 || first > INT64_MAX - count) {
    set_error("batch_draw: bad sizes n %ld first %ld count %ld", (long)n, (long)first, (long)count);
    return MOPOE_ERR_ARG;
  }
  if (count == 0) return MOPOE_OK;
  hipLaunchKernelGGL(batch_draw_kernel, dim3(glue_grid(count)), dim3(256), 0, (hipStream_t)stream, cdf, (long)n, seed, epoch, rank,
                     (long)first, (long)count, out);
  return check_launch("batch_draw");
}

extern "C" int mopoe_batch_assemble(const uint8_t* pa, const uint8_t* lat, int64_t n, int32_t S, const void* text, int32_t text_kind,
                                    int32_t L, int32_t F, const float* labels, int32_t n_labels, const int64_t* sel, int32_t B,
                                    float* out_pa, float* out_lat, float* out_text, float* out_labels, void* stream) {
  if (!pa || !lat || !text || !labels || !sel || !out_pa || !out_lat || !out_text || !out_labels) {
    set_error("batch_assemble: null input / output");
    return MOPOE_ERR_ARG;
  }
  if (n < 1 || S < 1 || L < 1 || n_labels < 1 || B < 1 || (text_kind != 0 && text_kind != 1) || (text_kind == 1 && F < 1)) {
    set_error("batch_assemble: bad sizes n %ld S %d L %d F %d n_labels %d B %d text_kind %d", (long)n, (int)S, (int)L, (int)F,
              (int)n_labels, (int)B, (int)text_kind);
    return MOPOE_ERR_ARG;
  }
  const long SS = (long)S * S;
  const long out_elems = 2L * B * SS + (long)B * L * (text_kind == 1 ? F : 1) + (long)B * n_labels;
  if (SS >= (1L << 31) || (long)L * (text_kind == 1 ? F : 1) >= (1L << 31) || out_elems >= (1L << 31)) {
    set_error("batch_assemble: %ld output elements (B %d, S %d, L %d, F %d): the batch must stay below 2^31 elements", out_elems,
              (int)B, (int)S, (int)L, (int)F);
    return MOPOE_ERR_ARG;
  }
  const bool vec = SS % 16 == 0 && (((uintptr_t)pa | (uintptr_t)lat | (uintptr_t)out_pa | (uintptr_t)out_lat) & 15) == 0;
  const long items = out_elems - (vec ? 2L * B * SS / 16 * 15 : 0);
  const unsigned F_ = text_kind == 1 ? (unsigned)F : 1u;
  if (vec)
    hipLaunchKernelGGL(batch_assemble_kernel<true>, dim3(glue_grid(items)), dim3(256), 0, (hipStream_t)stream, pa, lat, (long)n,
                       (unsigned)SS, text, (int)text_kind, (unsigned)L, F_, labels, (unsigned)n_labels, sel, (unsigned)B, out_pa,
                       out_lat, out_text, out_labels);
  else
    hipLaunchKernelGGL(batch_assemble_kernel<false>, dim3(glue_grid(items)), dim3(256), 0, (hipStream_t)stream, pa, lat, (long)n,
                       (unsigned)SS, text, (int)text_kind, (unsigned)L, F_, labels, (unsigned)n_labels, sel, (unsigned)B, out_pa,
                       out_lat, out_text, out_labels);
  return check_launch("batch_assemble");
}
