// iw_eval.hip -- importance-weighted log-likelihood of held-out windows.
//
// One importance sample k of window r has the log weight
//   l = - sum_t nll_t                                           (rownll: the training pass's Bernoulli NLL per frame)
//       + sum_{t,l} 0.5 (lvz + eps_z^2 - z^2),  z = mz + exp(lvz/2) eps_z       (log p(z) - log q(z|x,w))
//       + sum_c     0.5 (lvw + eps_w^2 - pr - s^2 / exp(pr)),  s = mw + exp(lvw/2) eps_w   (log p(s) - log q(s|x))
// formed in fp64 from the fp32 pieces the forward pass leaves, and folded into a per-window running log-sum-exp.
// One wave per window, no atomics: every state entry has one owner, so the result is bitwise reproducible.
#include "common.h"

namespace clv {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int IW_ROWS = 4;        // windows (waves) per workgroup

__global__ __launch_bounds__(64 * IW_ROWS) void iw_accumulate_kernel(int T, int L, int C1, int nvalid, const float* rownll,
                                                                    const float* zargs, const float* eps_z, const float* wargs,
                                                                    const float* eps_w, double prior, double* state,
                                                                    int32_t* step_dev) {
  const int row = blockIdx.x * IW_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row < nvalid) {
    double acc = 0.0;
    const int64_t r0 = (int64_t)row * T;
    for (int t = lane; t < T; t += 64) acc -= (double)rownll[r0 + t];
    // latent term over the window's T * L entries: entry i = t * L + l of the window
    const int TL = T * L;
    for (int i = lane; i < TL; i += 64) {
      const int t = i / L, l = i - t * L;
      const float* za = zargs + (r0 + t) * 2 * L;
      const double m = (double)za[l], lv = (double)za[L + l], e = (double)eps_z[r0 * L + i];
      const double z = m + exp(0.5 * lv) * e;
      acc += 0.5 * (lv + e * e - z * z);
    }
    if (C1 > 0) {
      const double ip = exp(-prior);
      for (int c = lane; c < C1; c += 64) {
        const float* wa = wargs + (int64_t)row * 2 * C1;
        const double m = (double)wa[c], lv = (double)wa[C1 + c], e = (double)eps_w[(int64_t)row * C1 + c];
        const double s = m + exp(0.5 * lv) * e;
        acc += 0.5 * (lv + e * e - prior - s * s * ip);
      }
    }
    const double lw = wave_sum_f64(acc);
    if (lane == 0) {
      double* st = state + (int64_t)row * 4;
      const double m0 = st[0];
      // a NaN weight takes over the shift (and from there every later update): the window reports NaN
      const double m1 = (lw > m0 || lw != lw) ? lw : m0;
      // exp(m0 - m1) and exp(l - m1) without -inf - (-inf): an empty state or a zero weight contributes nothing
      const double a = (m0 == -INFINITY) ? 0.0 : exp(m0 - m1);
      const double b = (lw == -INFINITY) ? 0.0 : exp(lw - m1);
      st[0] = m1;
      st[1] = st[1] * a + b;
      st[2] = st[2] * (a * a) + b * b;
      st[3] = st[3] + lw;
    }
  }
  // the sample counter of the eps draw: advanced once, after this launch's work (nothing in this launch reads it)
  if (step_dev && blockIdx.x == 0 && threadIdx.x == 0) *step_dev += 1;
}

__global__ __launch_bounds__(256) void iw_finish_kernel(int nvalid, int K, const double* state, double* log_p, double* elbo,
                                                         double* ess) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= nvalid) return;
  const double* st = state + (int64_t)row * 4;
  const double m = st[0], s1 = st[1], s2 = st[2];
  log_p[row] = m + log(s1) - log((double)K);
  elbo[row] = st[3] / (double)K;
  ess[row] = s1 * s1 / s2;          // (sum e^{l-m})^2 / sum e^{2(l-m)}: the shift cancels
}

}  // namespace clv

using namespace clv;

extern "C" int clv_iw_accumulate(int R, int T, int L, int C1, const float* rownll, const float* zargs, const float* eps_z,
                                 const float* wargs, const float* eps_w, float w_log_var_prior, int nvalid, double* state,
                                 int32_t* step_dev, void* stream) {
  if (R <= 0 || T <= 0 || L <= 0 || C1 < 0 || nvalid <= 0 || nvalid > R || !rownll || !zargs || !eps_z || !state)
    return CLV_EINVAL;
  if (C1 > 0 && (!wargs || !eps_w)) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("iw_accumulate", s);
  hipLaunchKernelGGL(iw_accumulate_kernel, dim3((nvalid + IW_ROWS - 1) / IW_ROWS), dim3(64 * IW_ROWS), 0, s, T, L, C1, nvalid,
                     rownll, zargs, eps_z, wargs, eps_w, (double)w_log_var_prior, state, step_dev);
  return launch_status();
}

extern "C" int clv_iw_finish(int R, int nvalid, int K, const double* state, double* log_p, double* elbo, double* ess,
                             void* stream) {
  if (R <= 0 || nvalid <= 0 || nvalid > R || K <= 0 || !state || !log_p || !elbo || !ess) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("iw_finish", s);
  hipLaunchKernelGGL(iw_finish_kernel, dim3((nvalid + 255) / 256), dim3(256), 0, s, nvalid, K, state, log_p, elbo, ess);
  return launch_status();
}
