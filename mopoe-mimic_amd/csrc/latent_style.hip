// Style stage of the factorized representation, forward and backward, for all three modalities in one launch each.
// Runs strictly after the content latent kernel (latent.hip / latent_mixture.hip), whose sample z it reads.
//
// Forward: one thread per element of the three decoder inputs zcat_m = [z_style_m | z] ([B, S_m + D], style columns
// first).  A style column draws z_style = eps * exp(0.5 * logvar) + mu and adds its term of KL(N(mu, logvar) || N(0, I));
// a content column copies z.  The three KL sums are reduced with wavefront shuffles -> LDS -> one double atomic per
// modality per block, and the last block to arrive writes klds_style[3] = KL_m / norm.
// Backward: one thread per (row, column) of [g_z | d_style_PA | d_style_Lateral | d_style_text]: the content column sums
// the present modalities' content-column gradients of zcat, a style column writes d mu and d logvar.
//
// Reference arithmetic: mimic/networks/VAEtrimodalMimic.py:31-62 (style draws), utils/utils.py:45-48 (reparameterize),
// evaluation/losses.py:34-42 (calc_klds_style), divergence_measures/kl_div.py:8-16, ConvNetworksImgMimic.py:43-49 and
// ConvNetworksTextMimic.py:43-54 (torch.cat((z_style, z_content), dim=1)).
#include "common.hpp"

namespace mopoe {

struct StyleArgs {
  const float* mu[3];
  const float* lv[3];
  const float* eps[3];
  int S[3];           // style dims (0 for an absent slot)
  long off[4];        // forward: element offsets of the slots' zcat in the flattened launch; off[3] = total
  int col[4];         // backward: column offsets of [g_z | style 0 | style 1 | style 2]; col[3] = total columns
  int B, D;
  float norm;
};

__device__ __forceinline__ int slot_of(const long* off, long i) {
  return i < off[1] ? 0 : (i < off[2] ? 1 : 2);
}

struct StyleFwdIO {
  const float* z;     // [B, D] content sample
  float* zcat[3];     // [B, S_m + D] decoder inputs
  float* klds;        // [3]
  double* ws;         // [3] sums + [1] arrival counter
};

__global__ __launch_bounds__(256) void latent_style_fwd_kernel(const StyleArgs a, const StyleFwdIO o, int nblocks) {
  __shared__ float red[4][3];
  __shared__ int is_last;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  float klp[3] = {0.f, 0.f, 0.f};
  if (i < a.off[3]) {
    const int m = slot_of(a.off, i);
    const int S = a.S[m], W = S + a.D;
    const long r = i - a.off[m];
    const int b = (int)(r / W), c = (int)(r - (long)b * W);
    float v;
    if (c < S) {
      const long e = (long)b * S + c;
      const float mu = a.mu[m][e], lv = a.lv[m][e];
      v = a.eps[m][e] * expf(0.5f * lv) + mu;
      const float t = 1.0f - expf(lv) - mu * mu + lv;
      klp[0] = m == 0 ? t : 0.f;
      klp[1] = m == 1 ? t : 0.f;
      klp[2] = m == 2 ? t : 0.f;
    } else {
      v = o.z[(long)b * a.D + (c - S)];
    }
    o.zcat[m][r] = v;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int m = 0; m < 3; ++m) {
    const float s = wave_sum(klp[m]);
    if (lane == 0) red[wave][m] = s;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int m = threadIdx.x;
    const float s = red[0][m] + red[1][m] + red[2][m] + red[3][m];
    if (a.S[m] > 0 && s != 0.f) atomic_add_f64(o.ws + m, (double)s);
  }
  // last-block finalisation (agent-scope release/acquire around the arrival counter), as latent.hip
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    const unsigned prev = atomicAdd(reinterpret_cast<unsigned*>(o.ws + 3), 1u);
    is_last = (prev == (unsigned)(nblocks - 1));
  }
  __syncthreads();
  if (is_last && threadIdx.x == 0) {
    __threadfence();
    for (int m = 0; m < 3; ++m) {
      const double s = __hip_atomic_load(o.ws + m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      o.klds[m] = a.S[m] > 0 ? (float)(-0.5 * s / (double)a.norm) : 0.f;
      __hip_atomic_store(o.ws + m, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __hip_atomic_store(reinterpret_cast<unsigned*>(o.ws + 3), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct StyleBwdIO {
  const float* g_zcat[3];
  const float* g_klds;
  float* dmu[3];
  float* dlv[3];
  float* g_z;
};

__global__ __launch_bounds__(256) void latent_style_bwd_kernel(const StyleArgs a, const StyleBwdIO g) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int W = a.col[3];
  if (i >= (long)a.B * W) return;
  const int b = (int)(i / W), j = (int)(i - (long)b * W);
  if (j < a.D) {
    // the content columns of every present modality's decoder input carried the same z
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < 3; ++m)
      if (a.S[m] > 0 && g.g_zcat[m]) s += g.g_zcat[m][(long)b * (a.S[m] + a.D) + a.S[m] + j];
    g.g_z[(long)b * a.D + j] = s;
    return;
  }
  const int m = j < a.col[1] ? 0 : (j < a.col[2] ? 1 : 2);
  const int S = a.S[m], c = j - a.col[m];
  const long e = (long)b * S + c;
  const float mu = a.mu[m][e], lv = a.lv[m][e];
  const float gzs = g.g_zcat[m] ? g.g_zcat[m][(long)b * (S + a.D) + c] : 0.f;
  const float gkl = g.g_klds ? g.g_klds[m] / a.norm : 0.f;
  g.dmu[m][e] = gzs + gkl * mu;
  g.dlv[m][e] = gzs * a.eps[m][e] * 0.5f * expf(0.5f * lv) + gkl * 0.5f * (expf(lv) - 1.0f);
}

static int fill_style_args(StyleArgs& a, const float* const mu[3], const float* const lv[3], const float* const eps[3],
                           const int32_t S[3], int B, int D, float norm, const char* who) {
  if (!mu || !lv || !eps || !S || B <= 0 || D <= 0 || !(norm > 0.f)) { set_error("%s: bad arguments", who); return MOPOE_ERR_ARG; }
  int n = 0;
  long off = 0;
  int col = D;
  a.off[0] = 0;
  a.col[0] = D;
  for (int m = 0; m < 3; ++m) {
    const bool p = mu[m] != nullptr;
    if (p != (lv[m] != nullptr) || p != (eps[m] != nullptr)) {
      set_error("%s: slot %d: mu / logvar / eps presence mismatch", who, m);
      return MOPOE_ERR_ARG;
    }
    if (p && S[m] < 1) { set_error("%s: slot %d: style dim %d < 1", who, m, (int)S[m]); return MOPOE_ERR_ARG; }
    a.mu[m] = mu[m]; a.lv[m] = lv[m]; a.eps[m] = eps[m];
    a.S[m] = p ? S[m] : 0;
    n += p;
    off += p ? (long)B * (S[m] + D) : 0;
    col += a.S[m];
    a.off[m + 1] = off;
    if (m < 2) a.col[m + 1] = col;
  }
  a.col[3] = col;
  if (!n) { set_error("%s: no modality present", who); return MOPOE_ERR_ARG; }
  if (off >= (1L << 31) * 256L || (long)B * col >= (1L << 31) * 256L) { set_error("%s: too large", who); return MOPOE_ERR_ARG; }
  a.B = B; a.D = D; a.norm = norm;
  return 0;
}

}  // namespace mopoe

using namespace mopoe;

extern "C" int mopoe_latent_style_fwd(const float* const smu[3], const float* const slv[3], const float* const eps_s[3],
                                      const int32_t S[3], int32_t B, int32_t D, const float* z, float norm,
                                      float* const zcat[3], float* klds_style, double* ws, void* stream) {
  StyleArgs a;
  if (int rc = fill_style_args(a, smu, slv, eps_s, S, B, D, norm, "latent_style_fwd")) return rc;
  if (!z || !zcat || !klds_style || !ws) { set_error("latent_style_fwd: null input / output"); return MOPOE_ERR_ARG; }
  for (int m = 0; m < 3; ++m)
    if (smu[m] && !zcat[m]) { set_error("latent_style_fwd: slot %d: missing zcat buffer", m); return MOPOE_ERR_ARG; }
  StyleFwdIO o = {z, {zcat[0], zcat[1], zcat[2]}, klds_style, ws};
  const int nblocks = ceil_div(a.off[3], 256);
  hipLaunchKernelGGL(latent_style_fwd_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, a, o, nblocks);
  return check_launch("latent_style_fwd");
}

extern "C" int mopoe_latent_style_bwd(const float* const smu[3], const float* const slv[3], const float* const eps_s[3],
                                      const int32_t S[3], int32_t B, int32_t D, float norm, const float* const g_zcat[3],
                                      const float* g_klds_style, float* const d_smu[3], float* const d_slv[3], float* g_z,
                                      void* stream) {
  StyleArgs a;
  if (int rc = fill_style_args(a, smu, slv, eps_s, S, B, D, norm, "latent_style_bwd")) return rc;
  if (!g_z || !d_smu || !d_slv) { set_error("latent_style_bwd: null output"); return MOPOE_ERR_ARG; }
  StyleBwdIO g;
  g.g_klds = g_klds_style;
  g.g_z = g_z;
  for (int m = 0; m < 3; ++m) {
    const bool p = smu[m] != nullptr;
    g.g_zcat[m] = (p && g_zcat) ? g_zcat[m] : nullptr;
    g.dmu[m] = d_smu[m];
    g.dlv[m] = d_slv[m];
    if (p && (!d_smu[m] || !d_slv[m])) { set_error("latent_style_bwd: slot %d: missing gradient buffer", m); return MOPOE_ERR_ARG; }
  }
  const int nblocks = ceil_div((long)B * a.col[3], 256);
  hipLaunchKernelGGL(latent_style_bwd_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, a, g);
  return check_launch("latent_style_bwd");
}
