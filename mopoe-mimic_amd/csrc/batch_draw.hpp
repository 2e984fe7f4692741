// The arithmetic of one weighted draw (include/mopoe_hip_data.h: mopoe_batch_draw), host and device: the kernel of
// batch.hip calls it per thread, a host program can call it to check the generator against its published vectors.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MOPOE_HD __host__ __device__ __forceinline__
#else
#define MOPOE_HD inline
#endif

namespace mopoe {

MOPOE_HD uint32_t mulhi_u32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

// Philox4x32-10: c = counter in, output words out; k0, k1 = key
MOPOE_HD void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = mulhi_u32(M0, c[0]), lo0 = M0 * c[0];
    const uint32_t hi1 = mulhi_u32(M1, c[2]), lo1 = M1 * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += W0; k1 += W1;
  }
}

// u in [0, 1) of draw i: 53 bits out of the first two output words
MOPOE_HD double draw_uniform(uint64_t seed, uint32_t epoch, uint32_t rank, uint64_t i) {
  uint32_t c[4] = {(uint32_t)(i & 0xffffffffu), (uint32_t)(i >> 32), epoch, rank};
  philox4x32_10(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32));
  return ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6)) * (1.0 / 9007199254740992.0);
}

// first j with cdf[j] > t, clamped to n - 1 (n >= 1)
MOPOE_HD int64_t first_above(const double* cdf, int64_t n, double t) {
  int64_t lo = 0, hi = n - 1;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cdf[mid] > t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

}  // namespace mopoe
