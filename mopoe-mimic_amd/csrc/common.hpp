// Shared device/host helpers for libmopoe_hip (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mopoe_hip.h"
#include "bn_ref_check.hpp"

#define MOPOE_WAVE 64

namespace mopoe {

void set_error(const char* fmt, ...);
int check_launch(const char* what);

// check_bn_ref (bn_ref_check.hpp) with its message handed to mopoe_last_error()
inline int bn_ref_ok(const mopoe_bn_ref* b, int C, bool allow_mode3, const char* who) {
  char msg[256];
  const int rc = check_bn_ref(b, C, allow_mode3, who, msg, sizeof msg);
  if (rc) set_error("%s", msg);
  return rc;
}

// ---- BatchNorm coefficients from a mopoe_bn_ref --------------------------------------------------
struct BnC {
  float mean, rstd, scale, shift;
};

__device__ __forceinline__ BnC bn_coef(const mopoe_bn_ref& b, int c) {
  BnC r;
#ifdef MOPOE_DBG_CONST_COEF   // timing experiment only (A/B library, wrong results): what the coefficient prologues cost
  r.mean = 0.f; r.rstd = 1.f; r.scale = 1.f; r.shift = 0.f;
  return r;
#endif
  if (b.mode == 3) {
    // the tensor that will be read is the ACTIVATION y = relu(gamma * xhat + beta) of this BatchNorm (of either kind,
    // batch or running statistics), not its input (conv2's input gradient when the block front is recomputed,
    // pointwise.hip): [y > 0] is the ReLU mask and xhat = (y - beta) / gamma wherever the mask is set -- the only places
    // the masked gradient looks at xhat.  Only gamma and beta are read: sums, rmean and rvar may be NULL
    // (mopoe_hip.h states the error bound of the rebuilt xhat)
    const float g = b.gamma[c];
    r.mean = b.beta[c];
    r.rstd = g != 0.f ? 1.0f / g : 0.f;
    r.scale = 1.f;
    r.shift = 0.f;
    return r;
  }
  if (b.mode == 1) {
    const double m = b.sums[c] * b.inv_count;
    double v = b.sums[b.C + c] * b.inv_count - m * m;
    v = v < 0.0 ? 0.0 : v;
    r.mean = (float)m;
    r.rstd = (float)(1.0 / sqrt(v + (double)b.eps));
  } else {
    r.mean = b.rmean[c];
    r.rstd = 1.0f / sqrtf(b.rvar[c] + b.eps);
  }
  const float g = b.gamma[c];
  r.scale = g * r.rstd;
  r.shift = b.beta[c] - r.mean * r.scale;
  return r;
}

__device__ __forceinline__ float mask_at(const mopoe_mask_ref& m, long row, int c, int C) {
  if (m.kind == 0) return 1.0f;
  if (m.kind == 1) return m.mask[(row / m.rows_per_sample) * (long)C + c];
  return m.mask[row * (long)C + c];
}

#ifdef MOPOE_DBG_NO_STAT_ATOMICS   // timing experiment only (A/B library; statistics are then wrong): DESIGN section 4, glue kernels
__device__ __forceinline__ void atomic_add_f64(double* p, double v) { if (v == 1.2345e300) *p = v; }
#else
__device__ __forceinline__ void atomic_add_f64(double* p, double v) { unsafeAtomicAdd(p, v); }
#endif

// ---- bf16 storage (BASELINE configs #3, #5): activations / activation gradients / MFMA operands are bfloat16 in HBM,
// every sum stays fp32 (statistics fp64).  A bf16 value is the upper half of the fp32 with the same value; rounding to
// bf16 is round-to-nearest-even (the compiler's __bf16 conversion: v_cvt_pk_bf16_f32, NaN stays NaN).
typedef unsigned short bf16_t;     // storage type at the C ABI (a plain 16-bit pattern)
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ float bf16_to_f32(bf16_t h) { return __uint_as_float((unsigned)h << 16); }
__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 f = {lo, hi};      // converted as a vector: ONE v_cvt_pk_bf16_f32 (two scalar conversions cost two + a v_perm)
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, bf16x2));
}
__device__ __forceinline__ bf16_t f32_to_bf16(float f) { return (bf16_t)(pack_bf16(f, 0.f) & 0xffffu); }
// the value a float has after a round trip through bf16 storage
__device__ __forceinline__ float round_bf16(float f) { return bf16_lo(pack_bf16(f, 0.f)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// ---- profiling (api.hip) ----------------------------------------------------------------------------
// one kind per kernel instantiation, so that the names bench.py reports are the names rocprofv3 prints.  The conv families'
// kinds stand beside their tile tables (conv_launch.hpp); 124..129 are the block fronts of pointwise.hip
enum { PROF_PW_FRONT = 124, PROF_NKINDS = MOPOE_PROF_KINDS };
struct ProfScope {
  hipStream_t stream;
  int slot;
  // flops / bytes: the launch's ALGORITHMIC work (one read of the input activation + one write of the
  // output per pass; bytes = 0 where not stated)
  ProfScope(hipStream_t s, double flops, int kind, double bytes = 0.0);
  ~ProfScope();
};

}  // namespace mopoe
