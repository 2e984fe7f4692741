// The exponential moving average of the weights (--ema_decay, include/mopoe_hip_ema.h) for gfx950: two HBM streaming
// kernels with the launch scheme of csrc/adam.hip -- the tensor records travel in the kernel arguments, EMA_SEGS_PER_LAUNCH
// per launch, a block owns one 4096-element chunk of one tensor and finds it with a ballot over the chunk prefix table.
//
//   ema_update_kernel  ema = fmaf(w, p - ema, ema), w = (float)(1 - min(decay, (1 + s) / (10 + s))) from Adam's device step
//                      counter: 12 bytes per element (p read, ema read and written), launched right behind the Adam launch
//                      that wrote p; nothing is stored when the clip state says the step was skipped
//   ema_swap_kernel    p <-> ema as raw 32-bit words (a NaN payload survives), p16 = bf16(new p): evaluation and the
//                      checkpoint under the averaged weights, in place because a captured step has p's address in its nodes
//
// The reference has no weight average; the Adam kernels of csrc/adam.hip are untouched by it.
#include "common.hpp"
#include "../../include/mopoe_hip_ema.h"

namespace mopoe {

constexpr int EMA_SEGS_PER_LAUNCH = 64;      // 64 * (32 + 4) B + scalars < 4 KiB of kernel arguments
constexpr int EMA_CHUNK = 4096;              // elements per block: 256 threads x 4 x 16 bytes
constexpr int EMA_THREADS = 256;

struct EmaPack {
  mopoe_ema_seg seg[EMA_SEGS_PER_LAUNCH];
  int chunk_start[EMA_SEGS_PER_LAUNCH];      // first block of each tensor; INT_MAX past the last one
};

// which tensor block b belongs to: the number of prefix entries <= b, minus one (one entry per lane); wave-uniform
__device__ __forceinline__ int ema_find_seg(const EmaPack& pack, int b) {
  static_assert(EMA_SEGS_PER_LAUNCH == 64, "one prefix entry per lane");
  const unsigned long long le = __ballot(pack.chunk_start[threadIdx.x & 63] <= b);
  return __builtin_amdgcn_readfirstlane(__popcll(le) - 1);
}

__device__ __forceinline__ float ema_one(float e, float p, float w) { return fmaf(w, p - e, e); }

__global__ __launch_bounds__(EMA_THREADS) void ema_update_kernel(const EmaPack pack, int nseg, double decay,
                                                                 const float* __restrict__ step,
                                                                 const float* __restrict__ clip) {
  if (clip && clip[MOPOE_CLIP_SKIP] != 0.f) return;
  const int tid = threadIdx.x;
  const int b = (int)blockIdx.x;
  const int si = ema_find_seg(pack, b);
  if (si < 0 || si >= nseg) return;
  const mopoe_ema_seg s = pack.seg[si];
  const long base = (long)(b - pack.chunk_start[si]) * EMA_CHUNK;
  const double sd = (double)step[0];
  const double warm = (1.0 + sd) / (10.0 + sd);
  const float w = (float)(1.0 - (decay < warm ? decay : warm));

  if (((((uintptr_t)s.p | (uintptr_t)s.ema)) & 15) == 0) {
    float4 p[4], e[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long k = base + (long)(i * EMA_THREADS + tid) * 4;
      ok[i] = k + 3 < s.n;
      if (ok[i]) {
        p[i] = *reinterpret_cast<const float4*>(s.p + k);
        e[i] = *reinterpret_cast<const float4*>(s.ema + k);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!ok[i]) continue;
      const long k = base + (long)(i * EMA_THREADS + tid) * 4;
      e[i].x = ema_one(e[i].x, p[i].x, w);
      e[i].y = ema_one(e[i].y, p[i].y, w);
      e[i].z = ema_one(e[i].z, p[i].z, w);
      e[i].w = ema_one(e[i].w, p[i].w, w);
      *reinterpret_cast<float4*>(s.ema + k) = e[i];
    }
    // the last n % 4 elements of the tensor: one thread of its last block
    const long tail = s.n & ~3L;
    if (tid == 0 && tail >= base && tail < base + EMA_CHUNK) {
      for (long k = tail; k < s.n; ++k) s.ema[k] = ema_one(s.ema[k], s.p[k], w);
    }
  } else {
    for (int i = tid; i < EMA_CHUNK; i += EMA_THREADS) {
      const long k = base + i;
      if (k >= s.n) break;
      s.ema[k] = ema_one(s.ema[k], s.p[k], w);
    }
  }
}

__global__ __launch_bounds__(EMA_THREADS) void ema_swap_kernel(const EmaPack pack, int nseg) {
  const int tid = threadIdx.x;
  const int b = (int)blockIdx.x;
  const int si = ema_find_seg(pack, b);
  if (si < 0 || si >= nseg) return;
  const mopoe_ema_seg s = pack.seg[si];
  const long base = (long)(b - pack.chunk_start[si]) * EMA_CHUNK;
  // raw words: the exchange must not depend on what a float move does to a NaN
  uint32_t* const pw = reinterpret_cast<uint32_t*>(s.p);
  uint32_t* const ew = reinterpret_cast<uint32_t*>(s.ema);

  const bool vec = ((((uintptr_t)s.p | (uintptr_t)s.ema) & 15) == 0) && (s.p16 == nullptr || (((uintptr_t)s.p16) & 7) == 0);
  if (vec) {
    uint4 p[4], e[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long k = base + (long)(i * EMA_THREADS + tid) * 4;
      ok[i] = k + 3 < s.n;
      if (ok[i]) {
        p[i] = *reinterpret_cast<const uint4*>(pw + k);
        e[i] = *reinterpret_cast<const uint4*>(ew + k);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!ok[i]) continue;
      const long k = base + (long)(i * EMA_THREADS + tid) * 4;
      *reinterpret_cast<uint4*>(pw + k) = e[i];
      *reinterpret_cast<uint4*>(ew + k) = p[i];
      if (s.p16) {
        uint2 o;
        o.x = pack_bf16(__uint_as_float(e[i].x), __uint_as_float(e[i].y));
        o.y = pack_bf16(__uint_as_float(e[i].z), __uint_as_float(e[i].w));
        *reinterpret_cast<uint2*>(s.p16 + k) = o;
      }
    }
    // the last n % 4 elements of the tensor: one thread of its last block
    const long tail = s.n & ~3L;
    if (tid == 0 && tail >= base && tail < base + EMA_CHUNK) {
      for (long k = tail; k < s.n; ++k) {
        const uint32_t pp = pw[k], ee = ew[k];
        pw[k] = ee; ew[k] = pp;
        if (s.p16) s.p16[k] = f32_to_bf16(__uint_as_float(ee));
      }
    }
  } else {
    for (int i = tid; i < EMA_CHUNK; i += EMA_THREADS) {
      const long k = base + i;
      if (k >= s.n) break;
      const uint32_t pp = pw[k], ee = ew[k];
      pw[k] = ee; ew[k] = pp;
      if (s.p16) s.p16[k] = f32_to_bf16(__uint_as_float(ee));
    }
  }
}

}  // namespace mopoe

using namespace mopoe;

// every refusal comes before the first launch: a refused call writes nothing
static int ema_check(const char* who, const mopoe_ema_seg* segs, int32_t nseg) {
  if ((!segs && nseg != 0) || nseg < 0) { set_error("%s: bad arguments", who); return MOPOE_ERR_ARG; }
  for (int32_t i = 0; i < nseg; ++i) {
    const mopoe_ema_seg& s = segs[i];
    if (s.n < 0) { set_error("%s: record %d has a negative size", who, (int)i); return MOPOE_ERR_ARG; }
    if (s.n == 0) continue;
    if (!s.p || !s.ema) { set_error("%s: record %d has a NULL p or ema", who, (int)i); return MOPOE_ERR_ARG; }
    if ((s.n + EMA_CHUNK - 1) / EMA_CHUNK > 0x7fffffffL) {
      set_error("%s: record %d has more than 2^43 elements", who, (int)i);
      return MOPOE_ERR_ARG;
    }
  }
  return MOPOE_OK;
}

// launch(pack, records in it, blocks) for every group of up to 64 records with n > 0
template <class Launch>
static int ema_for_each_pack(const mopoe_ema_seg* segs, int32_t nseg, const char* what, Launch launch) {
  int32_t i = 0;
  while (i < nseg) {
    EmaPack pack;
    int n = 0;
    long blocks = 0;
    for (; i < nseg && n < EMA_SEGS_PER_LAUNCH; ++i) {
      const mopoe_ema_seg& s = segs[i];
      if (s.n == 0) continue;
      const long nb = (s.n + EMA_CHUNK - 1) / EMA_CHUNK;
      if (blocks + nb > 0x7fffffffL) break;           // (a launch's grid: next launch takes the rest)
      pack.seg[n] = s;
      pack.chunk_start[n] = (int)blocks;
      blocks += nb;
      ++n;
    }
    for (int k = n; k < EMA_SEGS_PER_LAUNCH; ++k) { pack.seg[k] = mopoe_ema_seg{}; pack.chunk_start[k] = 0x7fffffff; }
    if (n == 0) continue;
    launch(pack, n, (unsigned)blocks);
    if (int rc = check_launch(what)) return rc;
  }
  return MOPOE_OK;
}

extern "C" int mopoe_ema_update(const mopoe_ema_seg* segs, int32_t nseg, double decay, const float* step,
                                const float* clip_state, void* stream) {
  if (int rc = ema_check("ema_update", segs, nseg)) return rc;
  if (!(decay >= 0.0) || !(decay < 1.0)) { set_error("ema_update: decay must be finite and in [0, 1)"); return MOPOE_ERR_ARG; }
  if (!step) { set_error("ema_update: the step counter is NULL"); return MOPOE_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  return ema_for_each_pack(segs, nseg, "ema_update", [&](const EmaPack& pack, int n, unsigned blocks) {
    hipLaunchKernelGGL(ema_update_kernel, dim3(blocks), dim3(EMA_THREADS), 0, st, pack, n, decay, step, clip_state);
  });
}

extern "C" int mopoe_ema_swap(const mopoe_ema_seg* segs, int32_t nseg, void* stream) {
  if (int rc = ema_check("ema_swap", segs, nseg)) return rc;
  hipStream_t st = (hipStream_t)stream;
  return ema_for_each_pack(segs, nseg, "ema_swap", [&](const EmaPack& pack, int n, unsigned blocks) {
    hipLaunchKernelGGL(ema_swap_kernel, dim3(blocks), dim3(EMA_THREADS), 0, st, pack, n);
  });
}
