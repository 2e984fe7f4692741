// Latent-representation evaluation (--eval_lr): batched logistic-regression fit and prediction (evaluation only, fp32).
//
// The reference fits one sklearn LogisticRegression(solver='lbfgs', max_iter=1000) per (modality subset, label) on the
// subset posterior's means of 500 training rows (mimic/evaluation/eval_metrics/representation.py:169-187) and predicts
// with it per test batch (:147-166).  With sklearn's defaults that is, per problem, with y in {0,1}:
//   f(w, b) = C sum_i [ log(1 + exp(m_i)) - y_i m_i ] + 1/2 |w|^2,   m_i = x_i . w + b      (b is NOT penalised)
// strictly convex once both classes occur.  lbfgs stops somewhere within its tolerance of the optimum; this kernel goes to
// the optimum itself.
//
// Fit: ONE launch for all S * L problems, one workgroup of 16 waves per problem, the whole damped-Newton loop inside:
//   pass over X (rows from L2/HBM, 16 at a time staged in LDS): margins, f, gradient g = C X^T (p - y) + [w; 0] and the
//     Hessian H = C X^T diag(p (1 - p)) X + diag(1, .., 1, 0), accumulated as 4 x 4 register blocks into a packed lower
//     triangle in LDS ((D+1)(D+2)/2 floats: 132.6 KB at D = 256, the largest D accepted);
//   Cholesky H = L L^T in place (right-looking, the scaled column kept in a vector so that the trailing update reads rows),
//     two triangular solves for d = -H^{-1} g;
//   backtracking on f (Armijo, at most LR_HALVINGS halvings).  Close to the optimum the decrease of f is below what a float
//     sum of N terms resolves: a full step whose f is equal within that resolution is taken as well, and kept only if it
//     lowered |g|_inf -- otherwise the previous iterate is restored and the loop ends (float32 has nothing more to give).
// Every loop has a fixed bound and every continuation test is written so that a NaN fails it: the kernel returns on any
// input and reports what it reached in info = (Newton steps taken, |grad f|_inf at the returned W).
// Sums run in a fixed order (lane stride, shuffle tree, waves in index order), no atomics: same input, same bits.
#include "common.hpp"

#include <float.h>

namespace mopoe {

constexpr int LR_THREADS = 1024;
constexpr int LR_WAVES = LR_THREADS / MOPOE_WAVE;
constexpr int LR_MAX_D = 256;
constexpr int LR_MAX_N1 = LR_MAX_D + 1;                    // coefficients + intercept
constexpr int LR_DP = (LR_MAX_N1 + 3) & ~3;                // padded to whole 4 x 4 blocks
constexpr int LR_TRI = LR_MAX_N1 * (LR_MAX_N1 + 1) / 2;
constexpr int LR_TILE = LR_WAVES;                          // rows staged per pass step: one per wave
constexpr int LR_HALVINGS = 24;
// LDS: 132,612 (H) + 16,640 (row tile) + 6 * 1,040 (vectors) + 208 = 155,700 B of the 163,840 B one workgroup may declare

struct LrShared {
  float H[LR_TRI];
  __attribute__((aligned(16))) float xt[LR_TILE * LR_DP];
  float w[LR_DP], g[LR_DP], d[LR_DP], wt[LR_DP], wprev[LR_DP], col[LR_DP];
  float st[LR_TILE], rt[LR_TILE], red[LR_WAVES];
  float bc[4];
};

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }

// log(1 + exp(m)) - y m, the probability's residual p - y and p (1 - p), stable for any finite m
__device__ __forceinline__ void logistic_terms(float m, float y, float& loss, float& r, float& s) {
  const float e = expf(-fabsf(m));                 // in (0, 1]
  const float inv = 1.f / (1.f + e);
  const float p = m >= 0.f ? inv : e * inv;
  loss = fmaxf(m, 0.f) + log1pf(e) - y * m;
  r = p - y;
  s = e * inv * inv;
}

// sum of the waves' partial losses in index order + 1/2 |v[0..D)|^2, returned to every thread
__device__ float finish_f(LrShared& sh, float wave_loss, const float* v, int D) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) sh.red[wv] = wave_loss;
  __syncthreads();
  if (wv == 0) {
    float q = 0.f;
    for (int c = lane; c < D; c += MOPOE_WAVE) q += v[c] * v[c];
    q = wave_sum(q);
    if (lane == 0) {
      float f = 0.f;
      for (int k = 0; k < LR_WAVES; ++k) f += sh.red[k];
      sh.bc[0] = f + 0.5f * q;
    }
  }
  __syncthreads();
  const float f = sh.bc[0];
  __syncthreads();        // (bc[0] and red are free again)
  return f;
}

// f at v (v[D] the intercept): rows straight from memory, one wave per row
__device__ float eval_f(LrShared& sh, const float* x, const float* y, int N, int D, int L, float C, const float* v) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float acc = 0.f;
  for (int row = wv; row < N; row += LR_WAVES) {
    const float* xr = x + (long)row * D;
    float part = 0.f;
    for (int c = lane; c < D; c += MOPOE_WAVE) part += xr[c] * v[c];
    const float m = wave_sum(part) + v[D];
    float loss, r, s;
    logistic_terms(m, y[(long)row * L] > 0.5f ? 1.f : 0.f, loss, r, s);
    acc += C * loss;
  }
  return finish_f(sh, acc, v, D);
}

// one pass at sh.w: f (returned), sh.g, sh.H
__device__ float pass_fgh(LrShared& sh, const float* x, const float* y, int N, int D, int L, float C) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = D + 1, dp = (n + 3) & ~3, nb = dp >> 2, nblk = nb * (nb + 1) / 2, ntri = n * (n + 1) / 2;
  for (int e = tid; e < ntri; e += LR_THREADS) sh.H[e] = 0.f;
  if (tid < dp) sh.g[tid] = tid < D ? sh.w[tid] : 0.f;
  __syncthreads();
  if (tid < D) sh.H[tri(tid, tid)] = 1.f;
  float acc_loss = 0.f;
  for (int row0 = 0; row0 < N; row0 += LR_TILE) {
    const int row = row0 + wv;
    float* xrow = sh.xt + wv * dp;
    float part = 0.f;
    if (row < N) {
      const float* xr = x + (long)row * D;
      for (int c = lane; c < dp; c += MOPOE_WAVE) {
        const float v = c < D ? xr[c] : (c == D ? 1.f : 0.f);
        xrow[c] = v;
        part += v * sh.w[c];                       // (w[D] is the intercept, w[c > D] = 0)
      }
    } else {
      for (int c = lane; c < dp; c += MOPOE_WAVE) xrow[c] = 0.f;
    }
    const float m = wave_sum(part);
    float loss = 0.f, r = 0.f, s = 0.f;
    if (row < N) {
      logistic_terms(m, y[(long)row * L] > 0.5f ? 1.f : 0.f, loss, r, s);
      acc_loss += C * loss;
    }
    if (lane == 0) {
      sh.st[wv] = C * s;
      sh.rt[wv] = C * r;
    }
    __syncthreads();
    if (tid < n) {
      float a = sh.g[tid];
#pragma unroll
      for (int t = 0; t < LR_TILE; ++t) a += sh.rt[t] * sh.xt[t * dp + tid];
      sh.g[tid] = a;
    }
    for (int blk = tid; blk < nblk; blk += LR_THREADS) {
      int bi = (int)((sqrtf(8.f * (float)blk + 1.f) - 1.f) * 0.5f);
      if (bi * (bi + 1) / 2 > blk) --bi;
      if ((bi + 1) * (bi + 2) / 2 <= blk) ++bi;
      const int bj = blk - bi * (bi + 1) / 2;
      const int i0 = bi * 4, j0 = bj * 4;
      float a[4][4] = {};
#pragma unroll 4
      for (int t = 0; t < LR_TILE; ++t) {
        const float4 xi = *reinterpret_cast<const float4*>(sh.xt + t * dp + i0);
        const float4 xj = *reinterpret_cast<const float4*>(sh.xt + t * dp + j0);
        const float s = sh.st[t];
        const float vi[4] = {s * xi.x, s * xi.y, s * xi.z, s * xi.w};
        const float vj[4] = {xj.x, xj.y, xj.z, xj.w};
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
          for (int q = 0; q < 4; ++q) a[p][q] += vi[p] * vj[q];
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int i = i0 + p, j = j0 + q;
          if (i < n && j <= i) sh.H[tri(i, j)] += a[p][q];
        }
    }
    __syncthreads();
  }
  return finish_f(sh, acc_loss, sh.w, D);
}

// |g|_inf to every thread; NaN when any entry is not finite
__device__ float grad_norm(LrShared& sh, int n) {
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < MOPOE_WAVE) {
    float mx = 0.f;
    int bad = 0;
    for (int c = lane; c < n; c += MOPOE_WAVE) {
      const float a = fabsf(sh.g[c]);
      if (!(a <= FLT_MAX)) bad = 1;
      else if (a > mx) mx = a;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float other = __shfl_xor(mx, o, 64);
      bad |= __shfl_xor(bad, o, 64);
      if (other > mx) mx = other;
    }
    if (lane == 0) sh.bc[1] = bad ? NAN : mx;
  }
  __syncthreads();
  const float v = sh.bc[1];
  __syncthreads();
  return v;
}

// H = L L^T in place (lower triangle); false when a pivot is not positive (or NaN)
__device__ bool cholesky(LrShared& sh, int n) {
  const int tid = threadIdx.x, tx = tid & 63, ty = tid >> 6;
  for (int k = 0; k < n; ++k) {
    const float piv = sh.H[tri(k, k)];
    if (!(piv > 0.f) || !(piv <= FLT_MAX)) return false;        // (the same value in every thread: a uniform exit)
    const float lkk = sqrtf(piv), inv = 1.f / lkk;
    for (int i = k + 1 + tid; i < n; i += LR_THREADS) {
      const float v = sh.H[tri(i, k)] * inv;
      sh.col[i] = v;
      sh.H[tri(i, k)] = v;
    }
    __syncthreads();
    if (tid == 0) sh.H[tri(k, k)] = lkk;
    for (int i = k + 1 + ty; i < n; i += LR_WAVES) {
      const float ci = sh.col[i];
      float* hrow = sh.H + tri(i, 0);
      for (int j = k + 1 + tx; j <= i; j += MOPOE_WAVE) hrow[j] -= ci * sh.col[j];
    }
    __syncthreads();
  }
  return true;
}

// d = -(L L^T)^{-1} g; returns g . d to every thread
__device__ float newton_direction(LrShared& sh, int n) {
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < n) sh.d[tid] = -sh.g[tid];
  __syncthreads();
  for (int k = 0; k < n; ++k) {                  // L y = -g, y into col
    const float yk = sh.d[k] / sh.H[tri(k, k)];
    for (int i = k + 1 + tid; i < n; i += LR_THREADS) sh.d[i] -= sh.H[tri(i, k)] * yk;
    if (tid == 0) sh.col[k] = yk;
    __syncthreads();
  }
  for (int k = n - 1; k >= 0; --k) {             // L^T d = y
    const float xk = sh.col[k] / sh.H[tri(k, k)];
    const float* hrow = sh.H + tri(k, 0);
    for (int j = tid; j < k; j += LR_THREADS) sh.col[j] -= hrow[j] * xk;
    if (tid == 0) sh.d[k] = xk;
    __syncthreads();
  }
  if (tid < MOPOE_WAVE) {
    float q = 0.f;
    for (int c = lane; c < n; c += MOPOE_WAVE) q += sh.g[c] * sh.d[c];
    q = wave_sum(q);
    if (lane == 0) sh.bc[2] = q;
  }
  __syncthreads();
  const float gd = sh.bc[2];
  __syncthreads();
  return gd;
}

__global__ __launch_bounds__(LR_THREADS) void logreg_fit_kernel(const float* X, const float* Y, int N, int D, int L, float C,
                                                                int max_iter, float tol, float* W, float* info) {
  __shared__ LrShared sh;
  const int tid = threadIdx.x;
  const int s = blockIdx.x / L, l = blockIdx.x % L;
  const float* x = X + (long)s * N * D;
  const float* y = Y + l;
  const int n = D + 1, dp = (n + 3) & ~3;
  if (tid < LR_DP) sh.w[tid] = sh.wprev[tid] = sh.wt[tid] = sh.d[tid] = 0.f;
  __syncthreads();
  int steps = 0;
  bool noise_step = false;
  float gn = NAN, prev_gn = INFINITY;
  for (int it = 0; it <= max_iter; ++it) {
    const float f0 = pass_fgh(sh, x, y, N, D, L, C);
    gn = grad_norm(sh, n);
    if (noise_step && !(gn < prev_gn)) {         // the step below float resolution did not help: take it back, done
      if (tid < dp) sh.w[tid] = sh.wprev[tid];
      __syncthreads();
      gn = prev_gn;
      --steps;
      break;
    }
    if (!(gn > tol)) break;                      // converged (or NaN)
    if (it == max_iter) break;
    if (!cholesky(sh, n)) break;
    const float gd = newton_direction(sh, n);
    if (!(gd < 0.f)) break;
    float t = 1.f;
    bool accepted = false;
    noise_step = false;
    const float slack = 1e-6f * fabsf(f0);       // what a float sum of N losses resolves (about 8 ulp of f)
    for (int h = 0; h < LR_HALVINGS; ++h) {
      if (tid < dp) sh.wt[tid] = tid < n ? sh.w[tid] + t * sh.d[tid] : 0.f;
      __syncthreads();
      const float ft = eval_f(sh, x, y, N, D, L, C, sh.wt);
      if (ft <= f0 + 1e-4f * t * gd) { accepted = true; break; }
      if (h == 0 && ft <= f0 + slack) { accepted = true; noise_step = true; break; }
      t *= 0.5f;
    }
    if (!accepted) break;
    if (tid < dp) {
      sh.wprev[tid] = sh.w[tid];
      sh.w[tid] = sh.wt[tid];
    }
    __syncthreads();
    prev_gn = gn;
    ++steps;
  }
  float* wout = W + (long)blockIdx.x * n;
  if (tid < n) wout[tid] = sh.w[tid];
  if (tid == 0) {
    info[2 * blockIdx.x] = (float)steps;
    info[2 * blockIdx.x + 1] = gn;
  }
}

struct LrRows {
  const float* x[8];
};

// one wave per (subset, row): the L decision values of the row
__global__ __launch_bounds__(256) void logreg_predict_kernel(const LrRows rows, int S, int M, int D, int L, const float* W,
                                                             float* pred, float* dec) {
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= (long)S * M) return;                   // whole waves only
  const int lane = threadIdx.x & 63;
  const int s = (int)(r / M), m = (int)(r % M);
  const float* xr = rows.x[s] + (long)m * D;
  for (int l = 0; l < L; ++l) {
    const float* w = W + ((long)s * L + l) * (D + 1);
    float part = 0.f;
    for (int c = lane; c < D; c += MOPOE_WAVE) part += xr[c] * w[c];
    const float v = wave_sum(part) + w[D];
    if (lane == 0) {
      pred[r * L + l] = v > 0.f ? 1.f : 0.f;
      if (dec) dec[r * L + l] = v;
    }
  }
}

}  // namespace mopoe

using namespace mopoe;

extern "C" int mopoe_logreg_fit(const float* X, const float* Y, int32_t S, int32_t N, int32_t D, int32_t L, float C,
                                int32_t max_iter, float tol, float* W, float* info, void* stream) {
  if (!X || !Y || !W || !info) { set_error("logreg_fit: null input / output"); return MOPOE_ERR_ARG; }
  if (S < 1 || L < 1 || N < 2 || D < 1 || D > LR_MAX_D || max_iter < 0 || !(C > 0.f) || !(tol >= 0.f) ||
      (long)S * L > 65535L || (long)S * N * D > (1L << 40)) {
    set_error("logreg_fit: bad sizes S %d N %d D %d (1..%d) L %d max_iter %d C %g tol %g", (int)S, (int)N, (int)D, LR_MAX_D,
              (int)L, (int)max_iter, (double)C, (double)tol);
    return MOPOE_ERR_ARG;
  }
  hipLaunchKernelGGL(logreg_fit_kernel, dim3((unsigned)(S * L)), dim3(LR_THREADS), 0, (hipStream_t)stream, X, Y, (int)N, (int)D,
                     (int)L, C, (int)max_iter, tol, W, info);
  return check_launch("logreg_fit");
}

extern "C" int mopoe_logreg_predict(const float* const* x, int32_t S, int32_t M, int32_t D, int32_t L, const float* W,
                                    float* pred, float* dec, void* stream) {
  if (!x || !W || !pred) { set_error("logreg_predict: null input / output"); return MOPOE_ERR_ARG; }
  if (S < 1 || S > 8 || M < 1 || D < 1 || L < 1 || (long)S * M > 0x7fffffffL) {
    set_error("logreg_predict: bad sizes S %d (1..8) M %d D %d L %d", (int)S, (int)M, (int)D, (int)L);
    return MOPOE_ERR_ARG;
  }
  LrRows rows = {};
  for (int s = 0; s < S; ++s) {
    if (!x[s]) { set_error("logreg_predict: null row pointer %d", s); return MOPOE_ERR_ARG; }
    rows.x[s] = x[s];
  }
  hipLaunchKernelGGL(logreg_predict_kernel, dim3((unsigned)(((long)S * M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, rows,
                     (int)S, (int)M, (int)D, (int)L, W, pred, dec);
  return check_launch("logreg_predict");
}
