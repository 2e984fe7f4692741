// Importance-sampled likelihood estimates of the factorized representation (evaluation only, fp32, forward only).
//
// Sample: one wave per importance-sample row r = k B + b of the [K*B] sample-major layout.  The lanes walk the D content
// columns, then the S style columns of the row: z = eps * exp(0.5 * logvar) + mu (utils.reparameterize) is written into
// the decoder input zcat [K*B, S + D] = [z_style | z], and the row's Gaussian terms
//   t = sum log N(z; 0, I) - sum log N(z; mu, logvar)       (unit_gaussian_log_pdf - gaussian_log_pdf)
// are reduced with wavefront shuffles, separately for the content (t_c) and the style (t_s) columns.  (mu, logvar) are
// [B, .], read at row b: the K repeats of get_latent_samples are an index, not a copy.
//
// Estimates: one workgroup per estimate (PA, Lateral, text marginals, joint).  Thread i walks row i of the reference's
// log_weight.view(batch_size, K) -- consecutive flat entries i K .. i K + K - 1 of the sample-major vector -- and forms its
// log-mean-exp in registers; the B values are summed in a fixed order (per-thread, then a fixed shuffle tree, then the 4
// waves in index order).  No atomics: the same inputs give the same bits.
//   marginal m: w = lp_m + t_c + [m in subset] t_s          (likelihood.py:77 passes the style only for subset members)
//   joint:      w = lp_0 + lp_1 + lp_2 + t_c + 3 t_s        (utils/likelihood.py:211-215 adds it once per modality key)
//
// Reference arithmetic: mimic/evaluation/eval_metrics/likelihood.py:17-96, mimic/utils/likelihood.py:13-220.
#include "common.hpp"

namespace mopoe {

__device__ __forceinline__ void draw_terms(const float* mu, const float* lv, const float* eps, float* out, int n, int lane,
                                           float& lp, float& lq) {
  constexpr float HALF_LOG2PI = 0.91893853320467274f;
  for (int c = lane; c < n; c += MOPOE_WAVE) {
    const float m = mu[c], l = lv[c];
    const float z = eps[c] * expf(0.5f * l) + m;
    out[c] = z;
    const float d = z - m;
    lp += -HALF_LOG2PI - 0.5f * z * z;
    lq += -HALF_LOG2PI - 0.5f * l - d * d / (2.f * expf(l));
  }
}

__global__ __launch_bounds__(256) void lhood_style_sample_kernel(const float* mu, const float* lv, const float* eps,
                                                                 const float* smu, const float* slv, const float* eps_s,
                                                                 long R, int B, int D, int S, float* zcat, float* t_c,
                                                                 float* t_s) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= R) return;                               // whole waves only: the shuffles below see all 64 lanes
  const int lane = threadIdx.x & 63;
  const long b = r % B;
  float* row = zcat + r * (long)(S + D);
  float lp = 0.f, lq = 0.f;
  draw_terms(mu + b * D, lv + b * D, eps + r * D, row + S, D, lane, lp, lq);
  const float tc = wave_sum(lp) - wave_sum(lq);
  lp = lq = 0.f;
  draw_terms(smu + b * S, slv + b * S, eps_s + r * S, row, S, lane, lp, lq);
  const float ts = wave_sum(lp) - wave_sum(lq);
  if (lane == 0) {
    t_c[r] = tc;
    t_s[r] = ts;
  }
}

struct EstArgs {
  const float* lp[3];
  const float* t_c;
  const float* t_s;   // NULL: no style term
  int K, B, mask;
};

__device__ __forceinline__ float log_weight(const EstArgs& a, int j, long r) {
  const float ts = a.t_s ? a.t_s[r] : 0.f;
  if (j < 3) return a.lp[j][r] + a.t_c[r] + (((a.mask >> j) & 1) ? ts : 0.f);
  return a.lp[0][r] + a.lp[1][r] + a.lp[2][r] + a.t_c[r] + 3.f * ts;
}

__global__ __launch_bounds__(256) void lhood_estimates_kernel(const EstArgs a, float* out) {
  __shared__ double part[4];
  const int j = blockIdx.x;
  double acc = 0.0;
  for (int i = threadIdx.x; i < a.B; i += 256) {
    const long r0 = (long)i * a.K;
    float m = -INFINITY;
    for (int k = 0; k < a.K; ++k) m = fmaxf(m, log_weight(a, j, r0 + k));
    float s = 0.f;
    for (int k = 0; k < a.K; ++k) s += expf(log_weight(a, j, r0 + k) - m);
    acc += (double)(m + logf(s / (float)a.K));
  }
  const double w = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) out[j] = (float)((((part[0] + part[1]) + part[2]) + part[3]) / (double)a.B);
}

}  // namespace mopoe

using namespace mopoe;

extern "C" int mopoe_lhood_style_sample(const float* mu, const float* logvar, const float* eps, const float* style_mu,
                                        const float* style_logvar, const float* style_eps, int32_t K, int32_t B, int32_t D,
                                        int32_t S, float* zcat, float* t_c, float* t_s, void* stream) {
  if (!mu || !logvar || !eps || !style_mu || !style_logvar || !style_eps || !zcat || !t_c || !t_s) {
    set_error("lhood_style_sample: null input / output"); return MOPOE_ERR_ARG;
  }
  const long R = (long)K * B;
  if (K < 1 || B < 1 || D < 1 || S < 1 || R > 0x7fffffffL || (R + 3) / 4 > 0x7fffffffL || R * (long)(S + D) > (1L << 40)) {
    set_error("lhood_style_sample: bad sizes K %d B %d D %d S %d", (int)K, (int)B, (int)D, (int)S); return MOPOE_ERR_ARG;
  }
  hipLaunchKernelGGL(lhood_style_sample_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, (hipStream_t)stream, mu, logvar,
                     eps, style_mu, style_logvar, style_eps, R, (int)B, (int)D, (int)S, zcat, t_c, t_s);
  return check_launch("lhood_style_sample");
}

extern "C" int mopoe_lhood_estimates(const float* const lp[3], const float* t_c, const float* t_s, int32_t K, int32_t B,
                                     int32_t subset_mask, float* out, void* stream) {
  if (!lp || !lp[0] || !lp[1] || !lp[2] || !t_c || !out) { set_error("lhood_estimates: null input / output"); return MOPOE_ERR_ARG; }
  if (K < 1 || B < 1 || (long)K * B > 0x7fffffffL || subset_mask < 0 || subset_mask > 7) {
    set_error("lhood_estimates: bad arguments K %d B %d mask %d", (int)K, (int)B, (int)subset_mask); return MOPOE_ERR_ARG;
  }
  EstArgs a = {{lp[0], lp[1], lp[2]}, t_c, t_s, (int)K, (int)B, (int)subset_mask};
  hipLaunchKernelGGL(lhood_estimates_kernel, dim3(4), dim3(256), 0, (hipStream_t)stream, a, out);
  return check_launch("lhood_estimates");
}
