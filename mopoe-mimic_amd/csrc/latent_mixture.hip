// Fused latent-space kernel of the mixture-of-experts methods (method='moe', the MMVAE baseline, and method='jsd', the
// mixture of experts with a dynamic prior), forward and backward.  Same structure as latent.hip: one thread per
// (row b, latent dim d); the subset and component KL sums are reduced with wavefront shuffles -> LDS -> one double atomic
// per sum per block; the last block to finish turns them into klds[] / individual_divs[] / joint_divergence, so the
// forward is a single launch.
//
// Reference arithmetic: mimic/utils/BaseMMVae.py:51-111,139-196 (moe_fusion for every subset and for the joint, the
// singletons as components, the N(0,I) prior component of jsd), mimic/utils/utils.py:55-77 (mixture selection),
// evaluation/divergence_measures/mm_div.py:20-32 (alpha_poe, eps = 1e-8), :67-106 (calc_alphaJSD_modalities,
// calc_group_divergence_moe), kl_div.py:8-16, evaluation/losses.py:24-31.
#include "common.hpp"

namespace mopoe {

constexpr int MAXK = 7;   // subsets
constexpr int MAXC = 4;   // components: the present singletons (+ the prior of jsd)
constexpr int WS_COMP = 7, WS_COUNTER = 15;   // workspace: [0, 7) subset sums, [7, 11) component sums, [15] arrivals
constexpr float POE_EPS = 1e-8f;

struct MixArgs {
  const float* mu[3];
  const float* lv[3];
  const float* eps;
  int B, D, K, C, jsd;
  int subset[MAXK];            // bitmask of active subset k (bit0 PA, bit1 Lateral, bit2 text)
  int comp_mod[MAXC];          // modality slot of component c; -1 for the prior component of jsd
  int member_rs[3][4];         // row partition of a subset of m + 1 members (members in sorted-name order)
  int comp_rs[MAXC + 1];       // row partition of the joint over the C components
  float w[MAXC];               // weights of the joint divergence
  float norm;
};

// one of three per-modality register values by a runtime slot (selects: an indexed array would go to scratch)
__device__ __forceinline__ float sel3(int s, float v0, float v1, float v2) { return s == 0 ? v0 : (s == 1 ? v1 : v2); }

// members of a subset in sorted-name order: Lateral (1), PA (0), text (2); the one that owns row b
__device__ __forceinline__ int subset_member(const MixArgs& a, int sm, int b) {
  const int m = ((sm & 1) + ((sm >> 1) & 1) + ((sm >> 2) & 1)) - 1;
  int j = 0;
#pragma unroll
  for (int mm = 1; mm < 3; ++mm) {
    if (mm == m) {
#pragma unroll
      for (int q = 1; q <= mm; ++q)
        if (b >= a.member_rs[mm][q]) j = q;
    }
  }
  constexpr int order[3] = {1, 0, 2};
  int seen = -1, owner = 1;
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (sm & (1 << order[q])) {
      ++seen;
      if (seen == j) owner = order[q];
    }
  }
  return owner;
}

__device__ __forceinline__ int comp_of_row(const MixArgs& a, int b) {
  int c = 0;
#pragma unroll
  for (int q = 1; q < MAXC; ++q)
    if (q < a.C && b >= a.comp_rs[q]) c = q;
  return c;
}

struct MixFwdOut {
  float *sub_mu, *sub_lv, *comp_mu, *comp_lv, *jm, *jl, *z, *klds, *indiv, *jd, *pd_mu, *pd_lv;
  double* ws;
};

__global__ __launch_bounds__(256) void latent_mixture_fwd_kernel(const MixArgs a, const MixFwdOut o, int nblocks) {
  __shared__ float red[4][MAXK + MAXC];
  __shared__ int is_last;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)a.B * a.D;
  const bool ok = idx < total;
  const long i = ok ? idx : 0;
  const int b = (int)(i / a.D);
  const float m0 = a.mu[0] ? a.mu[0][i] : 0.f, m1 = a.mu[1] ? a.mu[1][i] : 0.f, m2 = a.mu[2] ? a.mu[2][i] : 0.f;
  const float l0 = a.lv[0] ? a.lv[0][i] : 0.f, l1 = a.lv[1] ? a.lv[1][i] : 0.f, l2 = a.lv[2] ? a.lv[2][i] : 0.f;
  float part[MAXK + MAXC];
#pragma unroll
  for (int q = 0; q < MAXK + MAXC; ++q) part[q] = 0.f;
  // subsets: row b of subset k is row b of the member that owns it (an exact copy)
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    if (k < a.K) {
      const int s = subset_member(a, a.subset[k], b);
      const float mu = sel3(s, m0, m1, m2), lv = sel3(s, l0, l1, l2);
      if (ok) {
        o.sub_mu[(long)k * total + i] = mu;
        o.sub_lv[(long)k * total + i] = lv;
        part[k] = 1.0f - expf(lv) - mu * mu + lv;
      }
    }
  }
  // components (mu 0, logvar 0 for the prior) and, for jsd, the dynamic prior alpha_poe over them
  float cm[MAXC], cl[MAXC];
  float tsum = 0.f, msum = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    cm[c] = 0.f; cl[c] = 0.f;
    if (c < a.C) {
      const int s = a.comp_mod[c];
      if (s >= 0) { cm[c] = sel3(s, m0, m1, m2); cl[c] = sel3(s, l0, l1, l2); }
      if (a.jsd) {
        const float T = 1.0f / (expf(cl[c]) + POE_EPS);
        tsum += a.w[c] * T;
        msum += a.w[c] * cm[c] * T;
      }
    }
  }
  float pdm = 0.f, pdl = 0.f, pde = 1.f;
  if (a.jsd) {
    const float var = 1.0f / tsum;
    pdm = var * msum;
    pdl = logf(var);
    pde = expf(pdl);
  }
  const int cj = comp_of_row(a, b);
  if (ok) {
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c < a.C) {
        o.comp_mu[(long)c * total + i] = cm[c];
        o.comp_lv[(long)c * total + i] = cl[c];
        if (a.jsd) {
          const float dm = cm[c] - pdm;
          part[MAXK + c] = 1.0f - expf(cl[c]) / pde - dm * dm / pde + cl[c] - pdl;
        } else {
          part[MAXK + c] = 1.0f - expf(cl[c]) - cm[c] * cm[c] + cl[c];
        }
        if (c == cj) {
          o.jm[i] = cm[c];
          o.jl[i] = cl[c];
          o.z[i] = a.eps[i] * expf(0.5f * cl[c]) + cm[c];
        }
      }
    }
    if (a.jsd) { o.pd_mu[i] = pdm; o.pd_lv[i] = pdl; }
  }
  // block reduction of the K + C partial sums
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < MAXK + MAXC; ++q) {
    const float s = wave_sum(part[q]);
    if (lane == 0) red[wave][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < MAXK + MAXC) {
    const int q = threadIdx.x;
    if ((q < MAXK && q < a.K) || (q >= MAXK && q - MAXK < a.C))
      atomic_add_f64(o.ws + q, (double)(red[0][q] + red[1][q] + red[2][q] + red[3][q]));
  }
  // last-block finalisation (agent-scope release/acquire around the arrival counter)
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    const unsigned prev = atomicAdd(reinterpret_cast<unsigned*>(o.ws + WS_COUNTER), 1u);
    is_last = (prev == (unsigned)(nblocks - 1));
  }
  __syncthreads();
  if (is_last && threadIdx.x == 0) {
    __threadfence();
    for (int k = 0; k < a.K; ++k) {
      const double s = __hip_atomic_load(o.ws + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      o.klds[k] = (float)(-0.5 * s / (double)a.norm);
      __hip_atomic_store(o.ws + k, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float jd = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {   // (unrolled: a.w stays in registers)
      if (c < a.C) {
        const double s = __hip_atomic_load(o.ws + WS_COMP + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const float kl = (float)(-0.5 * s / (double)a.norm);
        o.indiv[c] = kl;
        jd += a.w[c] * kl;
        __hip_atomic_store(o.ws + WS_COMP + c, 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    o.jd[0] = jd;
    __hip_atomic_store(reinterpret_cast<unsigned*>(o.ws + WS_COUNTER), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

struct MixBwdIn {
  const float *g_sub_mu, *g_sub_lv, *g_comp_mu, *g_comp_lv, *g_jm, *g_jl, *g_z, *g_klds, *g_indiv, *g_jd, *g_pd_mu,
      *g_pd_lv;
  float* dmu[3];
  float* dlv[3];
};

__global__ __launch_bounds__(256) void latent_mixture_bwd_kernel(const MixArgs a, const MixBwdIn g) {
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)a.B * a.D;
  if (idx >= total) return;
  const long i = idx;
  const int b = (int)(i / a.D);
  const float m0 = a.mu[0] ? a.mu[0][i] : 0.f, m1 = a.mu[1] ? a.mu[1][i] : 0.f, m2 = a.mu[2] ? a.mu[2][i] : 0.f;
  const float l0 = a.lv[0] ? a.lv[0][i] : 0.f, l1 = a.lv[1] ? a.lv[1][i] : 0.f, l2 = a.lv[2] ? a.lv[2][i] : 0.f;
  float dm3[3] = {0.f, 0.f, 0.f}, dl3[3] = {0.f, 0.f, 0.f};
  const float inv_norm = 1.0f / a.norm;
  // subsets: the upstream gradient of row b goes to the member that owns it
#pragma unroll
  for (int k = 0; k < MAXK; ++k) {
    if (k >= a.K) continue;
    const int s = subset_member(a, a.subset[k], b);
    float gmu = g.g_sub_mu ? g.g_sub_mu[(long)k * total + i] : 0.f;
    float glv = g.g_sub_lv ? g.g_sub_lv[(long)k * total + i] : 0.f;
    if (g.g_klds) {
      const float gk = g.g_klds[k];
      gmu += gk * sel3(s, m0, m1, m2) * inv_norm;
      glv += gk * 0.5f * (expf(sel3(s, l0, l1, l2)) - 1.0f) * inv_norm;
    }
    // (s is present: every member of an active subset is)
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (q == s) { dm3[q] += gmu; dl3[q] += glv; }
  }
  // components: direct gradients, the joint's rows, the divergence
  const float gjd = g.g_jd ? g.g_jd[0] : 0.f;
  const int cj = comp_of_row(a, b);
  float cm[MAXC], cl[MAXC], ce[MAXC], gc[MAXC];
  float tsum = 0.f, msum = 0.f;
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    cm[c] = 0.f; cl[c] = 0.f; gc[c] = 0.f;
    if (c < a.C) {
      const int s = a.comp_mod[c];
      if (s >= 0) { cm[c] = sel3(s, m0, m1, m2); cl[c] = sel3(s, l0, l1, l2); }
      gc[c] = (g.g_indiv ? g.g_indiv[c] : 0.f) + gjd * a.w[c];
    }
    ce[c] = expf(cl[c]);
    if (a.jsd && c < a.C) {
      const float T = 1.0f / (ce[c] + POE_EPS);
      tsum += a.w[c] * T;
      msum += a.w[c] * cm[c] * T;
    }
  }
  float gP = 0.f, gL = 0.f, pdm = 0.f, pde = 1.f, var = 1.f;
  if (a.jsd) {
    var = 1.0f / tsum;
    pdm = var * msum;
    pde = expf(logf(var));
    gP = g.g_pd_mu ? g.g_pd_mu[i] : 0.f;
    gL = g.g_pd_lv ? g.g_pd_lv[i] : 0.f;
  }
#pragma unroll
  for (int c = 0; c < MAXC; ++c) {
    if (c >= a.C) continue;
    const int s = a.comp_mod[c];
    float gmu = 0.f, glv = 0.f;
    if (a.jsd) {
      // f_c = 1 - e_c/E - (mu_c - P)^2/E + lv_c - L, KL_c = -0.5/norm sum f_c, with E = exp(L)
      const float h = -0.5f * gc[c] * inv_norm;
      const float dm = cm[c] - pdm;
      const float r = 1.0f / pde;
      gmu += h * (-2.0f * dm * r);
      glv += h * (1.0f - ce[c] * r);
      gP += h * (2.0f * dm * r);
      gL += h * (ce[c] * r + dm * dm * r - 1.0f);
    } else {
      gmu += gc[c] * cm[c] * inv_norm;
      glv += gc[c] * 0.5f * (ce[c] - 1.0f) * inv_norm;
    }
    if (s < 0) continue;   // the prior component of jsd is a constant
    if (g.g_comp_mu) gmu += g.g_comp_mu[(long)c * total + i];
    if (g.g_comp_lv) glv += g.g_comp_lv[(long)c * total + i];
    if (c == cj) {
      if (g.g_jm) gmu += g.g_jm[i];
      if (g.g_jl) glv += g.g_jl[i];
      if (g.g_z) {
        const float gz = g.g_z[i];
        gmu += gz;
        glv += gz * 0.5f * a.eps[i] * expf(0.5f * cl[c]);
      }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
      if (q == s) { dm3[q] += gmu; dl3[q] += glv; }
  }
  if (a.jsd) {
    // back through alpha_poe: var = 1/S, S = sum_c w_c T_c, P = var * M, M = sum_c w_c mu_c T_c, L = log(var)
    const float gM = gP * var;
    const float gV = gP * (pdm / var) + gL / var;   // (pdm / var = M)
    const float gS = -gV * var * var;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
      if (c >= a.C) continue;
      const int s = a.comp_mod[c];
      if (s < 0) continue;
      const float T = 1.0f / (ce[c] + POE_EPS);
      const float gT = a.w[c] * (gS + gM * cm[c]);
      const float gmu = gM * a.w[c] * T;
      const float glv = gT * (-T * T * ce[c]);   // dT/dlv = -exp(lv) / (exp(lv)+eps)^2
#pragma unroll
      for (int q = 0; q < 3; ++q)
        if (q == s) { dm3[q] += gmu; dl3[q] += glv; }
    }
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    if (a.mu[s]) {
      g.dmu[s][i] = dm3[s];
      g.dlv[s][i] = dl3[s];
    }
  }
}

static int fill_mix_args(MixArgs& a, int method, const float* const mu_in[3], const float* const lv_in[3], const float* eps,
                  int B, int D, const int32_t* member_row_start, const int32_t* comp_row_start, const float* w,
                  float norm) {
  if (method != MOPOE_LATENT_MOE && method != MOPOE_LATENT_JSD) { set_error("latent_mixture: unknown method %d", method); return MOPOE_ERR_ARG; }
  int avail = 0, n = 0;
  for (int s = 0; s < 3; ++s) {
    a.mu[s] = mu_in[s];
    a.lv[s] = lv_in[s];
    if ((mu_in[s] == nullptr) != (lv_in[s] == nullptr)) { set_error("latent_mixture: mu/logvar presence mismatch"); return MOPOE_ERR_ARG; }
    if (mu_in[s]) { avail |= 1 << s; ++n; }
  }
  if (!avail || !eps || B <= 0 || D <= 0 || !member_row_start || !comp_row_start || !w || norm <= 0.f) {
    set_error("latent_mixture: bad arguments");
    return MOPOE_ERR_ARG;
  }
  static const int masks[MAXK] = {1, 2, 4, 3, 5, 6, 7};
  int K = 0;
  for (int k = 0; k < MAXK; ++k)
    if ((masks[k] & ~avail) == 0) a.subset[K++] = masks[k];
  for (int k = K; k < MAXK; ++k) a.subset[k] = 0;
  a.K = K;
  a.jsd = method == MOPOE_LATENT_JSD;
  a.C = n + a.jsd;
  int c = 0;
  for (int s = 0; s < 3; ++s)
    if (mu_in[s]) a.comp_mod[c++] = s;
  for (; c < MAXC; ++c) a.comp_mod[c] = -1;
  for (int m = 0; m < 3; ++m) {
    for (int q = 0; q < 4; ++q) {
      const int v = member_row_start[m * 4 + q];
      a.member_rs[m][q] = q <= m + 1 ? v : B;
    }
    if (a.member_rs[m][0] != 0 || a.member_rs[m][m + 1] != B) { set_error("latent_mixture: member_row_start must span [0, B]"); return MOPOE_ERR_ARG; }
    for (int q = 0; q <= m; ++q)
      if (a.member_rs[m][q] > a.member_rs[m][q + 1]) { set_error("latent_mixture: member_row_start must not decrease"); return MOPOE_ERR_ARG; }
  }
  for (int q = 0; q <= MAXC; ++q) a.comp_rs[q] = q <= a.C ? comp_row_start[q] : B;
  if (a.comp_rs[0] != 0 || a.comp_rs[a.C] != B) { set_error("latent_mixture: comp_row_start must span [0, B]"); return MOPOE_ERR_ARG; }
  for (int q = 0; q < a.C; ++q)
    if (a.comp_rs[q] > a.comp_rs[q + 1]) { set_error("latent_mixture: comp_row_start must not decrease"); return MOPOE_ERR_ARG; }
  for (int q = 0; q < MAXC; ++q) a.w[q] = q < a.C ? w[q] : 0.f;
  a.eps = eps; a.B = B; a.D = D; a.norm = norm;
  return 0;
}

}  // namespace mopoe

using namespace mopoe;

extern "C" int mopoe_latent_mixture_fwd(int32_t method, const float* const mu_in[3], const float* const lv_in[3],
                                        const float* eps, int32_t B, int32_t D, const int32_t* member_row_start,
                                        const int32_t* comp_row_start, const float* w, float norm, float* sub_mu,
                                        float* sub_lv, float* comp_mu, float* comp_lv, float* joint_mu, float* joint_lv,
                                        float* z, float* klds, float* individual_divs, float* joint_div, float* pd_mu,
                                        float* pd_lv, double* ws, void* stream) {
  MixArgs a;
  if (int rc = fill_mix_args(a, method, mu_in, lv_in, eps, B, D, member_row_start, comp_row_start, w, norm)) return rc;
  if (!sub_mu || !sub_lv || !comp_mu || !comp_lv || !joint_mu || !joint_lv || !z || !klds || !individual_divs ||
      !joint_div || !ws || (a.jsd && (!pd_mu || !pd_lv))) {
    set_error("latent_mixture_fwd: null output");
    return MOPOE_ERR_ARG;
  }
  MixFwdOut o = {sub_mu, sub_lv, comp_mu, comp_lv, joint_mu, joint_lv, z, klds, individual_divs, joint_div, pd_mu, pd_lv, ws};
  const int nblocks = ceil_div((long)B * D, 256);
  hipLaunchKernelGGL(latent_mixture_fwd_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, a, o, nblocks);
  return check_launch("latent_mixture_fwd");
}

extern "C" int mopoe_latent_mixture_bwd(int32_t method, const float* const mu_in[3], const float* const lv_in[3],
                                        const float* eps, int32_t B, int32_t D, const int32_t* member_row_start,
                                        const int32_t* comp_row_start, const float* w, float norm, const float* g_sub_mu,
                                        const float* g_sub_lv, const float* g_comp_mu, const float* g_comp_lv,
                                        const float* g_joint_mu, const float* g_joint_lv, const float* g_z,
                                        const float* g_klds, const float* g_individual_divs, const float* g_joint_div,
                                        const float* g_pd_mu, const float* g_pd_lv, float* const d_mu_in[3],
                                        float* const d_lv_in[3], void* stream) {
  MixArgs a;
  if (int rc = fill_mix_args(a, method, mu_in, lv_in, eps, B, D, member_row_start, comp_row_start, w, norm)) return rc;
  MixBwdIn g = {g_sub_mu, g_sub_lv, g_comp_mu, g_comp_lv, g_joint_mu, g_joint_lv, g_z, g_klds, g_individual_divs,
                g_joint_div, a.jsd ? g_pd_mu : nullptr, a.jsd ? g_pd_lv : nullptr,
                {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
  for (int s = 0; s < 3; ++s) {
    g.dmu[s] = d_mu_in[s];
    g.dlv[s] = d_lv_in[s];
    if (mu_in[s] && (!d_mu_in[s] || !d_lv_in[s])) { set_error("latent_mixture_bwd: missing gradient buffer"); return MOPOE_ERR_ARG; }
  }
  const int nblocks = ceil_div((long)B * D, 256);
  hipLaunchKernelGGL(latent_mixture_bwd_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, a, g);
  return check_launch("latent_mixture_bwd");
}
