// Adam over every parameter tensor of the model in a handful of launches (gfx950).
//
// Replaces optim.Adam.step of the reference (mimic/utils/experiment.py:171-178, driven by mimic/run_epochs.py:131) with
// the arithmetic of PyTorch's fused, capturable Adam (float state, the two moment updates and the final `+ eps` carried
// in double like that kernel's double-typed hyper-parameters make them): 7 streams of 4 bytes per parameter, HBM-bound.
// The multi-tensor kernel it replaces needs ~25 launches of <= 320 blocks for the 397 tensors / 65 M parameters of
// BASELINE config #2 (each launch ends in a tail that leaves most CUs idle: 2.8 TB/s); here the tensor records travel
// in the kernel arguments, ADAM_SEGS_PER_LAUNCH per launch, a block owns one 4096-element chunk of one tensor and finds
// it with two ballots over the chunk prefix table.
//
// --max_grad_norm (include/mopoe_hip_optim.h): the global L2 norm of all gradients over the same records and the same
// chunking -- every block stores ONE double partial, one finishing block adds them in a fixed order: deterministic, no
// floating-point atomics -- and a CLIP instantiation of the two Adam kernels that reads {scale, skip} from the clip state.
#include "common.hpp"
#include "../../include/mopoe_hip_optim.h"

namespace mopoe {

constexpr int ADAM_SEGS_PER_LAUNCH = 64;     // 64 * (48 + 4) B + scalars < 4 KiB of kernel arguments
constexpr int ADAM_CHUNK = 4096;             // elements per block: 256 threads x 4 float4
constexpr int ADAM_THREADS = 256;

struct AdamPack {
  mopoe_adam_seg seg[ADAM_SEGS_PER_LAUNCH];
  int chunk_start[ADAM_SEGS_PER_LAUNCH];     // first block of each tensor; INT_MAX past the last one
};

// step += 1; coef = {lr / bias_correction1, sqrt(bias_correction2)} for that step (CLIP: unless the clip state says skip)
template <bool CLIP>
__global__ void adam_prep_kernel(float* step, const float* lr_dev, double lr_host, double beta1, double beta2, float* coef,
                                 const float* clip) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (CLIP && clip[MOPOE_CLIP_SKIP] != 0.f) return;
  const float s = step[0] + 1.f;
  step[0] = s;
  const double lr = lr_dev ? (double)lr_dev[0] : lr_host;
  const float bc1 = (float)(1.0 - pow(beta1, (double)s));
  const float bc2s = (float)sqrt(1.0 - pow(beta2, (double)s));
  coef[0] = (float)(lr / (double)bc1);
  coef[1] = bc2s;
}

struct AdamHyper {
  double beta1, beta2, eps;
  float step_size, bc2_sqrt;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamHyper& h) {
  m = (float)(h.beta1 * (double)m + (1.0 - h.beta1) * (double)g);
  v = (float)(h.beta2 * (double)v + (1.0 - h.beta2) * (double)g * (double)g);
  const float denom = (float)((double)(sqrtf(v) / h.bc2_sqrt) + h.eps);
  p -= h.step_size * m / denom;
}

// CLIP: `clip` is the clip state of mopoe_grad_norm (written by an earlier launch): nothing is stored when it says skip,
// otherwise every gradient is multiplied by its scale (float) as it is loaded.  CLIP = false never reads `clip`.
template <bool CLIP>
__global__ __launch_bounds__(ADAM_THREADS) void adam_kernel(const AdamPack pack, int nseg, const float* __restrict__ coef,
                                                            double beta1, double beta2, double eps, const float* clip) {
  float gs = 1.f;
  if (CLIP) {
    if (clip[MOPOE_CLIP_SKIP] != 0.f) return;
    gs = clip[MOPOE_CLIP_SCALE];
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = (int)blockIdx.x;
  // which tensor: the number of prefix entries <= b (ADAM_SEGS_PER_LAUNCH == 64: one entry per lane)
  static_assert(ADAM_SEGS_PER_LAUNCH == 64, "one prefix entry per lane");
  const unsigned long long le = __ballot(pack.chunk_start[lane] <= b);
  const int si = __builtin_amdgcn_readfirstlane(__popcll(le) - 1);
  if (si < 0 || si >= nseg) return;
  const mopoe_adam_seg s = pack.seg[si];
  const long base = (long)(b - pack.chunk_start[si]) * ADAM_CHUNK;
  AdamHyper h;
  h.beta1 = beta1; h.beta2 = beta2; h.eps = eps;
  h.step_size = coef[0]; h.bc2_sqrt = coef[1];

  const bool vec = ((((uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.v) & 15) == 0) &&
                   (s.p16 == nullptr || (((uintptr_t)s.p16) & 7) == 0);
  if (vec) {
    float4 p[4], g[4], m[4], v[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long e = base + (long)(i * ADAM_THREADS + tid) * 4;
      ok[i] = e + 3 < s.n;
      if (ok[i]) {
        g[i] = *reinterpret_cast<const float4*>(s.g + e);
        p[i] = *reinterpret_cast<const float4*>(s.p + e);
        m[i] = *reinterpret_cast<const float4*>(s.m + e);
        v[i] = *reinterpret_cast<const float4*>(s.v + e);
        if (CLIP) { g[i].x *= gs; g[i].y *= gs; g[i].z *= gs; g[i].w *= gs; }
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!ok[i]) continue;
      const long e = base + (long)(i * ADAM_THREADS + tid) * 4;
      adam_one(p[i].x, g[i].x, m[i].x, v[i].x, h);
      adam_one(p[i].y, g[i].y, m[i].y, v[i].y, h);
      adam_one(p[i].z, g[i].z, m[i].z, v[i].z, h);
      adam_one(p[i].w, g[i].w, m[i].w, v[i].w, h);
      *reinterpret_cast<float4*>(s.p + e) = p[i];
      *reinterpret_cast<float4*>(s.m + e) = m[i];
      *reinterpret_cast<float4*>(s.v + e) = v[i];
      if (s.p16) {
        uint2 o;
        o.x = pack_bf16(p[i].x, p[i].y);
        o.y = pack_bf16(p[i].z, p[i].w);
        *reinterpret_cast<uint2*>(s.p16 + e) = o;
      }
    }
    // the last n % 4 elements of the tensor: one thread of its last block
    const long tail = s.n & ~3L;
    if (tid == 0 && tail >= base && tail < base + ADAM_CHUNK) {
      for (long e = tail; e < s.n; ++e) {
        float pp = s.p[e], mm = s.m[e], vv = s.v[e];
        adam_one(pp, CLIP ? s.g[e] * gs : s.g[e], mm, vv, h);
        s.p[e] = pp; s.m[e] = mm; s.v[e] = vv;
        if (s.p16) s.p16[e] = f32_to_bf16(pp);
      }
    }
  } else {
    for (int i = tid; i < ADAM_CHUNK; i += ADAM_THREADS) {
      const long e = base + i;
      if (e >= s.n) break;
      float pp = s.p[e], mm = s.m[e], vv = s.v[e];
      adam_one(pp, CLIP ? s.g[e] * gs : s.g[e], mm, vv, h);
      s.p[e] = pp; s.m[e] = mm; s.v[e] = vv;
      if (s.p16) s.p16[e] = f32_to_bf16(pp);
    }
  }
}

// ---- gradient norm ---------------------------------------------------------------------------------------------------------
struct NormPack {
  const float* g[ADAM_SEGS_PER_LAUNCH];
  long n[ADAM_SEGS_PER_LAUNCH];
  int chunk_start[ADAM_SEGS_PER_LAUNCH];     // first block of each tensor; INT_MAX past the last one
};

__device__ __forceinline__ double sq64(float x) { return (double)x * (double)x; }

// partial[block] = sum of g^2 over the block's chunk, every element squared and added in double; a fixed order per block
__global__ __launch_bounds__(ADAM_THREADS) void grad_norm_partial_kernel(const NormPack pack, int nseg, double* partial) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int b = (int)blockIdx.x;
  static_assert(ADAM_SEGS_PER_LAUNCH == 64, "one prefix entry per lane");
  const unsigned long long le = __ballot(pack.chunk_start[lane] <= b);
  const int si = __builtin_amdgcn_readfirstlane(__popcll(le) - 1);
  if (si < 0 || si >= nseg) return;
  const float* g = pack.g[si];
  const long n = pack.n[si];
  const long base = (long)(b - pack.chunk_start[si]) * ADAM_CHUNK;
  double acc = 0.0;
  if ((((uintptr_t)g) & 15) == 0) {
    float4 x[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long e = base + (long)(i * ADAM_THREADS + tid) * 4;
      ok[i] = e + 3 < n;
      if (ok[i]) x[i] = *reinterpret_cast<const float4*>(g + e);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!ok[i]) continue;
      acc += sq64(x[i].x);
      acc += sq64(x[i].y);
      acc += sq64(x[i].z);
      acc += sq64(x[i].w);
    }
    // the last n % 4 elements of the tensor: one thread of its last block
    const long tail = n & ~3L;
    if (tid == 0 && tail >= base && tail < base + ADAM_CHUNK) {
      for (long e = tail; e < n; ++e) acc += sq64(g[e]);
    }
  } else {
    for (int i = tid; i < ADAM_CHUNK; i += ADAM_THREADS) {
      const long e = base + i;
      if (e >= n) break;
      acc += sq64(g[e]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  __shared__ double wsum[ADAM_THREADS / 64];
  if (lane == 0) wsum[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partial[b] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// ONE block: thread t adds partial[t], partial[t + 256], ... in index order, a fixed tree adds the 256 sums; thread 0 writes
// the clip state {norm, scale, skip, skipped_total += skip}
__global__ __launch_bounds__(ADAM_THREADS) void grad_norm_finish_kernel(const double* partial, long count, double max_norm,
                                                                        float* state) {
  const int tid = threadIdx.x;
  double acc = 0.0;
  // sixteen loads in flight per thread, added in index order (one load per add would pay a memory round trip per partial:
  // 55 of them in a row at config #2's 14 k chunks); past the end a +0.0 is added, which changes no sum of squares
  constexpr int FLY = 16;
  for (long i = tid; i < count; i += (long)FLY * ADAM_THREADS) {
    double x[FLY];
#pragma unroll
    for (int k = 0; k < FLY; ++k) {
      const long j = i + (long)k * ADAM_THREADS;
      x[k] = j < count ? partial[j] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < FLY; ++k) acc += x[k];
  }
  __shared__ double sh[ADAM_THREADS];
  sh[tid] = acc;
  __syncthreads();
  for (int s = ADAM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) sh[tid] += sh[tid + s];
    __syncthreads();
  }
  if (tid != 0) return;
  const double norm_d = sqrt(sh[0]);
  const float norm = (float)norm_d;
  const bool finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
  float scale = 0.f;
  if (finite) {
    const double sd = max_norm / (norm_d + 1e-6);
    scale = sd < 1.0 ? (float)sd : 1.f;
  }
  const float skip = finite ? 0.f : 1.f;
  state[MOPOE_CLIP_NORM] = norm;
  state[MOPOE_CLIP_SCALE] = scale;
  state[MOPOE_CLIP_SKIP] = skip;
  state[MOPOE_CLIP_SKIPPED_TOTAL] = state[MOPOE_CLIP_SKIPPED_TOTAL] + skip;
}

}  // namespace mopoe

using namespace mopoe;

template <bool CLIP>
static int adam_step_impl(const mopoe_adam_seg* segs, int32_t nseg, float* step, const float* lr_dev, double lr, double beta1,
                          double beta2, double eps, float* coef, const float* clip, void* stream) {
  if ((!segs && nseg != 0) || nseg < 0 || !coef) { set_error("adam_step: bad arguments"); return MOPOE_ERR_ARG; }
  if (CLIP && !clip) { set_error("adam_step_clipped: the clip state is NULL"); return MOPOE_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  if (step) {   // (step == NULL: a further part of a step whose counter and coefficients an earlier call has set)
    hipLaunchKernelGGL(adam_prep_kernel<CLIP>, dim3(1), dim3(64), 0, st, step, lr_dev, lr, beta1, beta2, coef, clip);
    if (int rc = check_launch("adam_prep")) return rc;
  }
  int32_t i = 0;
  while (i < nseg) {
    AdamPack pack;
    int n = 0;
    long blocks = 0;
    for (; i < nseg && n < ADAM_SEGS_PER_LAUNCH; ++i) {
      const mopoe_adam_seg& s = segs[i];
      if (!s.g || s.n == 0) continue;                 // no gradient: the tensor and its state stay as they are
      if (!s.p || !s.m || !s.v || s.n < 0) { set_error("adam_step: record %d is incomplete", (int)i); return MOPOE_ERR_ARG; }
      const long nb = (s.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
      if (nb > 0x7fffffffL) { set_error("adam_step: record %d has more than 2^43 elements", (int)i); return MOPOE_ERR_ARG; }
      if (blocks + nb > 0x7fffffffL) break;           // (a launch's grid: next launch takes the rest)
      pack.seg[n] = s;
      pack.chunk_start[n] = (int)blocks;
      blocks += nb;
      ++n;
    }
    for (int k = n; k < ADAM_SEGS_PER_LAUNCH; ++k) { pack.seg[k] = mopoe_adam_seg{}; pack.chunk_start[k] = 0x7fffffff; }
    if (n == 0) continue;
    hipLaunchKernelGGL(adam_kernel<CLIP>, dim3((unsigned)blocks), dim3(ADAM_THREADS), 0, st, pack, n, coef, beta1, beta2, eps,
                       clip);
    if (int rc = check_launch("adam_step")) return rc;
  }
  return MOPOE_OK;
}

extern "C" int mopoe_adam_step(const mopoe_adam_seg* segs, int32_t nseg, float* step, const float* lr_dev, double lr,
                               double beta1, double beta2, double eps, float* coef, void* stream) {
  return adam_step_impl<false>(segs, nseg, step, lr_dev, lr, beta1, beta2, eps, coef, nullptr, stream);
}

extern "C" int mopoe_adam_step_clipped(const mopoe_adam_seg* segs, int32_t nseg, float* step, const float* lr_dev, double lr,
                                       double beta1, double beta2, double eps, float* coef, const float* state, void* stream) {
  return adam_step_impl<true>(segs, nseg, step, lr_dev, lr, beta1, beta2, eps, coef, state, stream);
}

// chunks of the records that take part (with_g: only those that have a gradient); -1: a record with n < 0 or too many chunks
static long norm_chunks(const mopoe_adam_seg* segs, int32_t nseg, bool with_g) {
  long total = 0;
  for (int32_t i = 0; i < nseg; ++i) {
    const mopoe_adam_seg& s = segs[i];
    if (s.n < 0) return -1;
    if (s.n == 0 || (with_g && !s.g)) continue;
    const long nb = (s.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
    if (nb > 0x7fffffffL || total + nb < total) return -1;
    total += nb;
  }
  return total;
}

extern "C" int64_t mopoe_grad_norm_partials(const mopoe_adam_seg* segs, int32_t nseg) {
  if ((!segs && nseg != 0) || nseg < 0) { set_error("grad_norm_partials: bad arguments"); return MOPOE_ERR_ARG; }
  const long total = norm_chunks(segs, nseg, false);
  if (total < 0) { set_error("grad_norm_partials: a record has a negative size or more than 2^43 elements"); return MOPOE_ERR_ARG; }
  return total;
}

extern "C" int mopoe_grad_norm(const mopoe_adam_seg* segs, int32_t nseg, double max_norm, double* scratch, int64_t scratch_len,
                               float* state, void* stream) {
  // every refusal comes before the first launch: a refused call writes nothing
  if ((!segs && nseg != 0) || nseg < 0) { set_error("grad_norm: bad arguments"); return MOPOE_ERR_ARG; }
  if (!state) { set_error("grad_norm: the clip state is NULL"); return MOPOE_ERR_ARG; }
  if (!scratch || scratch_len < 0) { set_error("grad_norm: the scratch buffer is NULL"); return MOPOE_ERR_ARG; }
  if (!(max_norm >= 0.0) || max_norm > 1.7976931348623157e308) {
    set_error("grad_norm: max_norm must be finite and >= 0");
    return MOPOE_ERR_ARG;
  }
  const long need = norm_chunks(segs, nseg, true);
  if (need < 0) { set_error("grad_norm: a record has a negative size or more than 2^43 elements"); return MOPOE_ERR_ARG; }
  if (need > scratch_len) {
    set_error("grad_norm: scratch holds %ld doubles, the gradients need %ld", (long)scratch_len, need);
    return MOPOE_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  long done = 0;                                      // chunks (= partials) of the launches so far
  int32_t i = 0;
  while (i < nseg) {
    NormPack pack;
    int n = 0;
    long blocks = 0;
    for (; i < nseg && n < ADAM_SEGS_PER_LAUNCH; ++i) {
      const mopoe_adam_seg& s = segs[i];
      if (!s.g || s.n == 0) continue;                 // no gradient: contributes nothing
      const long nb = (s.n + ADAM_CHUNK - 1) / ADAM_CHUNK;
      if (blocks + nb > 0x7fffffffL) break;           // (a launch's grid: next launch takes the rest)
      pack.g[n] = s.g;
      pack.n[n] = s.n;
      pack.chunk_start[n] = (int)blocks;
      blocks += nb;
      ++n;
    }
    for (int k = n; k < ADAM_SEGS_PER_LAUNCH; ++k) { pack.g[k] = nullptr; pack.n[k] = 0; pack.chunk_start[k] = 0x7fffffff; }
    if (n == 0) continue;
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)blocks), dim3(ADAM_THREADS), 0, st, pack, n, scratch + done);
    if (int rc = check_launch("grad_norm_partial")) return rc;
    done += blocks;
  }
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(ADAM_THREADS), 0, st, (const double*)scratch, done, max_norm, state);
  return check_launch("grad_norm_finish");
}
