// smc.hip -- particle-filter sampling under a constraint roll (sequential Monte Carlo).
//
// G melodies own P particle rows each, r = m * P + p (R = G * P rows in one launch).  Per generated frame, replayed from
// one captured graph, the frame chain of the engine runs unchanged up to x_hat; then
//   clv_smc_sample    one wave per row: Bernoulli draw + constraint (as clv_bernoulli_sample_clamped, roll row m = r / P),
//                     the frame's log weight increment l_r in fp64, the frame as uint8 into the per-step history;
//   clv_smc_resample  one workgroup per melody: log Z, normalized log weights, ESS, systematic resampling, ancestors A_t;
//   clv_smc_gather    the rows of the state buffers permuted by A_t (through a scratch buffer: a gather is not in place);
// and once at the end clv_smc_backtrack draws the returned paths from the final weights and walks the lineage.
// With a key prior every particle carries its own label row: clv_smc_init_w draws the rows once per chunk,
// the gather moves them with the state, clv_smc_w_posterior (in the frame, after the gather) writes the weighted mean of
// the rows, and clv_smc_take_w copies the rows of the returned paths.
// Particle Gibbs reruns the filter with row m * P pinned to the path retained from the sweep before:
// clv_smc_pin_z and clv_smc_pin_frame put that path's latents, frames and bridge into the pinned row, in the frame;
// clv_smc_resample_conditional is clv_smc_resample with conditional multinomial resampling (one kernel body, two instances);
// clv_smc_backtrack_path writes the lineage clv_smc_backtrack drew as the next retained path, latents included.
// A filter stream stops the filter after any frame and continues it: clv_smc_resample_carry is clv_smc_resample
// with a Philox step offset and a carry of the weights (the same kernel body), clv_smc_commit emits the pending frames on
// which every lineage agrees and keeps the rest in a ring per melody, clv_smc_collapse draws the particle a melody is forced
// onto (or ends on) and writes its pending lineage.
// Every output element has one owner and no kernel uses atomics, so every result is bitwise reproducible.
#include "common.h"
#include "philox.h"

namespace clv {

constexpr uint32_t SMC_STREAM = 0xFFFFFFFDu;        // trainer.py's stream map, next to the IW pair
constexpr uint32_t SMC_W_STREAM = 0xFFFFFFFCu;      // the particles' keys: step 0 the categorical u0, step 1 the eps
constexpr uint32_t GIBBS_STREAM = 0xFFFFFFFAu;      // a conditional sweep's own uniform per particle (0xFFFFFFFB: key_track)
constexpr uint32_t COLLAPSE_STREAM = 0xFFFFFFF8u;   // a filter stream's forced pick; 0xFFFFFFF9: the transposer
constexpr int SMC_MAX_C = 32;                        // classes of a label row (MAXC of the label kernels)
constexpr int SMC_MAX_P = 1024;                      // particles per melody: one workgroup holds them
constexpr int SMC_MAX_BUFS = 8;
constexpr float SMC_CLIP_LO = 1e-7f, SMC_CLIP_HI = 1.0f - 1e-7f;   // Keras float32 BCE clip (BCE_CLIP_* on the logits)

__device__ __forceinline__ double smc_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double smc_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// workgroup-wide sum / max of one value per thread (a fixed order: butterfly in the wave, then the waves in turn)
__device__ double block_sum(double v, double* red) {
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = smc_wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = 0.0;
  for (int i = 0; i < nw; ++i) s += red[i];
  __syncthreads();
  return s;
}
__device__ double block_max(double v, double* red) {
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = smc_wave_max(v);
  if ((threadIdx.x & 63) == 0) red[w] = v;
  __syncthreads();
  double s = red[0];
  for (int i = 1; i < nw; ++i) s = fmax(s, red[i]);
  __syncthreads();
  return s;
}

// cum[p] = sum_{q <= p} v_q over the workgroup (wave scan, then the wave totals)
__device__ void block_inclusive_scan(double v, double* cum, double* red) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) red[w] = v;
  __syncthreads();
  double base = 0.0;
  for (int i = 0; i < w; ++i) base += red[i];
  cum[threadIdx.x] = base + v;
  __syncthreads();
}

// systematic resampling: draw i of n takes the first particle p with n * cum[p] > u0 + i (the last one if none)
__device__ __forceinline__ int systematic_pick(const double* cum, int P, double n, double x) {
  int lo = 0, hi = P - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (n * cum[mid] > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__device__ __forceinline__ double smc_uniform(uint64_t seed, int64_t melody, uint32_t step, uint32_t stream = SMC_STREAM) {
  return (double)philox_uniform_at((uint64_t)melody, (uint32_t)seed, (uint32_t)(seed >> 32), stream, step);
}

constexpr int SMC_ROWS = 4;        // rows (waves) per workgroup of the row kernels

__global__ __launch_bounds__(64 * SMC_ROWS) void smc_sample_kernel(int R, int D, int P, int nsteps, int S, const float* p,
                                                                  const float* u, const uint8_t* clamp,
                                                                  const int32_t* step_dev, float* x, double* ell,
                                                                  uint8_t* hist) {
  const int row = blockIdx.x * SMC_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= R) return;
  const int k = *step_dev - S;
  const bool on = k >= 0 && k < nsteps;
  const int64_t base = (int64_t)row * D;
  const uint8_t* cr = clamp + ((int64_t)(row / P) * nsteps + (on ? k : 0)) * D;
  uint8_t* hr = hist + ((int64_t)(on ? k : 0) * R + row) * D;
  double l = 0.0;
  for (int j = lane; j < D; j += 64) {
    const float pj = p[base + j], uj = u[base + j];
    const uint8_t cb = on ? cr[j] : (uint8_t)255;
    float xs = (uj <= pj) ? 1.f : 0.f;
    if (cb <= 1) {
      xs = (float)cb;
      const float q = fminf(fmaxf(pj, SMC_CLIP_LO), SMC_CLIP_HI);
      l += cb ? log((double)q) : log(1.0 - (double)q);
    }
    x[base + j] = xs;
    if (on) hr[j] = (uint8_t)xs;
  }
  if (on) {
    l = smc_wave_sum(l);
    if (lane == 0) ell[row] = l;
  }
}

// CONDITIONAL (particle Gibbs): row m * P is the retained path and keeps itself as its ancestor; every other
// particle draws its own uniform (GIBBS_STREAM, index = its GLOBAL row) and takes the first q with cum[q] > u, the last
// one if none -- conditional multinomial resampling.  Weights, log Z, ESS and the rule are the filter's.
// t0, carry (a filter stream): the Philox step of the uniforms is t0 + the chain step, and with carry the
// launch's step 0 continues logW, logZ and nres instead of starting them.  0, 0: the filter of one call.
template <bool CONDITIONAL>
__global__ __launch_bounds__(SMC_MAX_P) void smc_resample_kernel(int P, int nsteps, int S, uint64_t seed, int64_t m0,
                                                                 double tau, const double* ell, double* logW, double* logZ,
                                                                 double* ess, int32_t* nres, int32_t* flag, int32_t* anc,
                                                                 const int32_t* step_dev, int R, uint32_t t0, int carry) {
  __shared__ double red[SMC_MAX_P / 64];
  __shared__ double cum[SMC_MAX_P];
  const int k = *step_dev - S;
  if (k < 0 || k >= nsteps) return;             // seed steps and the bridge carry no weight (uniform exit: no barrier hit)
  const bool first = k == 0 && !carry;
  const int m = blockIdx.x, p = threadIdx.x;
  const bool mine = p < P;
  const int64_t r = (int64_t)m * P + p;
  const double logP = log((double)P);
  // step 0 starts from uniform weights, log Z = 0 and no resamples: nothing to initialise before the first replay
  const double lw = mine ? (first ? -logP : logW[r]) + ell[r] : -INFINITY;
  const double M = block_max(lw, red);
  const double a = mine ? exp(lw - M) : 0.0;
  const double s1 = block_sum(a, red);
  const double s2 = block_sum(a * a, red);
  const double lse = M + log(s1);
  const double wn = lw - lse;                   // normalized log weight after this frame
  const double e = s1 * s1 / s2;                // = 1 / sum exp(2 wn); exactly P for uniform weights
  const bool resample = e < tau * (double)P;
  if (resample) {
    block_inclusive_scan(mine ? exp(wn) : 0.0, cum, red);
    if (mine) {
      if (CONDITIONAL) {
        const double up = (double)philox_uniform_at((uint64_t)((m0 + m) * P + p), (uint32_t)seed, (uint32_t)(seed >> 32),
                                                    GIBBS_STREAM, t0 + (uint32_t)(k + S));
        anc[(int64_t)k * R + r] = m * P + (p == 0 ? 0 : systematic_pick(cum, P, 1.0, up));
      } else {
        const double u0 = smc_uniform(seed, m0 + m, t0 + (uint32_t)(k + S));
        anc[(int64_t)k * R + r] = m * P + systematic_pick(cum, P, (double)P, u0 + (double)p);
      }
      logW[r] = -logP;
    }
  } else if (mine) {
    anc[(int64_t)k * R + r] = (int32_t)r;
    logW[r] = wn;
  }
  if (p == 0) {
    logZ[m] = (first ? 0.0 : logZ[m]) + lse;
    ess[(int64_t)m * nsteps + k] = e;
    nres[m] = (first ? 0 : nres[m]) + (resample ? 1 : 0);
    flag[m] = resample ? 1 : 0;
  }
}

struct SmcBufs {
  float* buf[SMC_MAX_BUFS];
  int width[SMC_MAX_BUFS];        // floats per row
  int64_t off[SMC_MAX_BUFS];      // the buffer's slab in the scratch buffer (floats)
  int n;
};

// TO_SCRATCH: scratch row r = buffer row A_t[r]; otherwise buffer row r = scratch row r.  Only melodies that resampled
// at this step move (flag); every other row keeps its state.
template <bool TO_SCRATCH>
__global__ __launch_bounds__(64 * SMC_ROWS) void smc_gather_kernel(int R, int P, int nsteps, int S, SmcBufs b, float* scratch,
                                                                  const int32_t* anc, const int32_t* flag,
                                                                  const int32_t* step_dev) {
  const int row = blockIdx.x * SMC_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= R) return;
  const int k = *step_dev - S;
  if (k < 0 || k >= nsteps || !flag[row / P]) return;
  const int64_t src = TO_SCRATCH ? (int64_t)anc[(int64_t)k * R + row] : (int64_t)row;
  for (int i = 0; i < b.n; ++i) {
    const int w = b.width[i];
    float* s = scratch + b.off[i] + (int64_t)row * w;
    if (TO_SCRATCH) {
      const float* in = b.buf[i] + src * w;
      for (int j = lane; j < w; j += 64) s[j] = in[j];
    } else {
      float* out = b.buf[i] + src * w;
      for (int j = lane; j < w; j += 64) out[j] = s[j];
    }
  }
}

__global__ __launch_bounds__(SMC_MAX_P) void smc_backtrack_kernel(int P, int nsteps, int D, int n_out, uint64_t seed,
                                                                  int64_t m0, int step, const double* logW,
                                                                  const int32_t* anc, const uint8_t* hist, float* Xs,
                                                                  int32_t* picks, int R) {
  __shared__ double red[SMC_MAX_P / 64];
  __shared__ double cum[SMC_MAX_P];
  const int m = blockIdx.x, p = threadIdx.x;
  block_inclusive_scan(p < P ? exp(logW[(int64_t)m * P + p]) : 0.0, cum, red);
  const double u0 = smc_uniform(seed, m0 + m, (uint32_t)step);
  const int lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  for (int o = threadIdx.x >> 6; o < n_out; o += nw) {
    const int pick = systematic_pick(cum, P, (double)n_out, u0 + (double)o);
    int64_t r = (int64_t)m * P + pick;
    if (picks && lane == 0) picks[(int64_t)m * n_out + o] = pick;
    float* out = Xs + ((int64_t)m * n_out + o) * nsteps * D;
    for (int k = nsteps - 1; k >= 0; --k) {
      r = anc[(int64_t)k * R + r];              // the row before step k's resampling: its frame k is the path's
      const uint8_t* h = hist + ((int64_t)k * R + r) * D;
      for (int j = lane; j < D; j += 64) out[(int64_t)k * D + j] = (float)h[j];
    }
  }
}

// One workgroup per melody, thread p owns row r = m * P + p of wr [R, C].
// mode 0 (categorical): cum = inclusive fp64 sums of probs[m] in class order; particle p takes the first class with
// P * cum_c > u0 + p (systematic_pick: the last class if none) and writes its one-hot row.
// mode 1 (logistic-normal): s_c = mean + exp(log_var / 2) * eps (float32, eps at the GLOBAL row), w = softmax([s, 0]).
__global__ __launch_bounds__(SMC_MAX_P) void smc_init_w_kernel(int P, int C, int mode, uint64_t seed, int64_t m0,
                                                               const double* probs, const float* mean,
                                                               const float* log_var, float* wr) {
  __shared__ double cum[SMC_MAX_C];
  const int m = blockIdx.x, p = threadIdx.x;
  const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  if (mode == 0) {
    if (p == 0) {
      const double* pm = probs + (int64_t)m * C;
      double s = 0.0;
      for (int c = 0; c < C; ++c) cum[c] = s += pm[c];
    }
    __syncthreads();
    if (p >= P) return;
    const double u0 = (double)philox_uniform_at((uint64_t)(m0 + m), k0, k1, SMC_W_STREAM, 0u);
    const int key = systematic_pick(cum, C, (double)P, u0 + (double)p);
    float* out = wr + ((int64_t)m * P + p) * C;
    for (int c = 0; c < C; ++c) out[c] = c == key ? 1.f : 0.f;
    return;
  }
  if (p >= P) return;
  const int C1 = C - 1;
  const uint64_t e0 = (uint64_t)((m0 + m) * P + p) * (uint64_t)C1;
  const float* mu = mean + (int64_t)m * C1;
  const float* lv = log_var + (int64_t)m * C1;
  float s[SMC_MAX_C];
  float M = 0.f;                                 // the appended zero takes part in the max
  for (int c = 0; c < C1; ++c) {
    s[c] = mu[c] + expf(0.5f * lv[c]) * philox_normal_at(e0 + c, k0, k1, SMC_W_STREAM, 1u);
    M = fmaxf(M, s[c]);
  }
  s[C1] = 0.f;
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += s[c] = expf(s[c] - M);
  float* out = wr + ((int64_t)m * P + p) * C;
  for (int c = 0; c < C; ++c) out[c] = s[c] / sum;
}

constexpr int SMC_POST_THREADS = 256;

// out[m, k, c] = sum_p exp(logW[r]) * wr[r, c] from the weights and rows the next step starts from (after the gather).
// The weights go through LDS once; then a wave per class: every lane sums its particles p = lane, lane + 64, ... in that
// order, the lanes by the butterfly, and lane 0 owns the output element.
__global__ __launch_bounds__(SMC_POST_THREADS) void smc_w_posterior_kernel(int P, int C, int nsteps, int S, const double* logW,
                                                                           const float* wr, const int32_t* step_dev,
                                                                           double* out) {
  __shared__ double wexp[SMC_MAX_P];
  const int k = *step_dev - S;
  if (k < 0 || k >= nsteps) return;             // uniform exit before the barrier, as smc_resample_kernel
  const int m = blockIdx.x;
  const double* lw = logW + (int64_t)m * P;
  for (int p = threadIdx.x; p < P; p += SMC_POST_THREADS) wexp[p] = exp(lw[p]);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const float* rows = wr + (int64_t)m * P * C;
  double* o = out + ((int64_t)m * nsteps + k) * C;
  for (int c = threadIdx.x >> 6; c < C; c += SMC_POST_THREADS / 64) {
    double a = 0.0;
    for (int p = lane; p < P; p += 64) a += wexp[p] * (double)rows[(int64_t)p * C + c];
    a = smc_wave_sum(a);
    if (lane == 0) o[c] = a;
  }
}

// w_out[m, o, :] = wr[m * P + picks[m, o], :]: the label row of the particle each returned path was drawn from
__global__ void smc_take_w_kernel(int n, int P, int C, int n_out, const int32_t* picks, const float* wr, float* w_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = i % C, mo = i / C, m = mo / n_out;
  const int pick = min(max(picks[mo], 0), P - 1);
  w_out[i] = wr[((int64_t)m * P + pick) * C + c];
}

// ---- particle Gibbs: a conditional sweep pins row m * P of every melody to the retained path ----
// z[m * P, :] = z_ref[m, c, :] at chain step c = *step_dev (seed steps included); a thread per element of the G pinned rows
__global__ void smc_pin_z_kernel(int n, int P, int L, int T, const float* z_ref, const int32_t* step_dev, float* z) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = *step_dev;
  if (c < 0 || c >= T) return;
  const int m = i / L, j = i - m * L;
  z[(int64_t)m * P * L + j] = z_ref[((int64_t)m * T + c) * L + j];
}

// after the draw: at returned step k the pinned row's sample and its history row become x_ref[m, k, :]; at step S - 1
// (S > 0) the sample becomes the retained bridge.  A wave per melody; no other row and no other step is touched.
__global__ __launch_bounds__(64 * SMC_ROWS) void smc_pin_frame_kernel(int G, int P, int D, int nsteps, int S,
                                                                     const uint8_t* x_ref, const float* bridge,
                                                                     const int32_t* step_dev, float* x, uint8_t* hist) {
  const int m = blockIdx.x * SMC_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= G) return;
  const int k = *step_dev - S;
  float* xr = x + (int64_t)m * P * D;
  if (k >= 0 && k < nsteps) {
    const uint8_t* src = x_ref + ((int64_t)m * nsteps + k) * D;
    uint8_t* hr = hist + ((int64_t)k * G * P + (int64_t)m * P) * D;
    for (int j = lane; j < D; j += 64) {
      const uint8_t b = src[j];
      xr[j] = (float)b;
      hr[j] = b;
    }
  } else if (k == -1 && S > 0 && bridge) {
    const float* src = bridge + (int64_t)m * D;
    for (int j = lane; j < D; j += 64) xr[j] = src[j];
  }
}

// the path of pick picks[m] walked back as smc_backtrack_kernel walks it, written as the next retained path: frames
// (uint8), the latents of every chain step, the bridge; renewed[m, k] = the row frame k came from is not the pinned one.
// Seed steps and the bridge come from the lineage's root, the row at k = 0: nothing resamples before it.
__global__ __launch_bounds__(64 * SMC_ROWS) void smc_backtrack_path_kernel(int G, int P, int nsteps, int S, int D, int L,
                                                                          const int32_t* picks, const int32_t* anc,
                                                                          const uint8_t* hist, const float* zhist,
                                                                          const float* bridge_rows, uint8_t* x_ref,
                                                                          float* z_ref, float* bridge_ref, uint8_t* renewed) {
  const int m = blockIdx.x * SMC_ROWS + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (m >= G) return;
  const int64_t R = (int64_t)G * P, first = (int64_t)m * P;
  const int T = S + nsteps;
  int64_t r = first + min(max(picks[m], 0), P - 1);
  for (int k = nsteps - 1; k >= 0; --k) {
    r = min(max((int64_t)anc[(int64_t)k * R + r], first), first + P - 1);     // a melody's lineage stays in its rows
    const uint8_t* h = hist + ((int64_t)k * R + r) * D;
    uint8_t* xo = x_ref + ((int64_t)m * nsteps + k) * D;
    for (int j = lane; j < D; j += 64) xo[j] = h[j];
    const float* zs = zhist + ((int64_t)(S + k) * R + r) * L;
    float* zo = z_ref + ((int64_t)m * T + S + k) * L;
    for (int j = lane; j < L; j += 64) zo[j] = zs[j];
    if (lane == 0) renewed[(int64_t)m * nsteps + k] = r != first ? 1 : 0;
  }
  for (int t = 0; t < S; ++t) {
    const float* zs = zhist + ((int64_t)t * R + r) * L;
    float* zo = z_ref + ((int64_t)m * T + t) * L;
    for (int j = lane; j < L; j += 64) zo[j] = zs[j];
  }
  if (S > 0 && bridge_rows && bridge_ref)
    for (int j = lane; j < D; j += 64) bridge_ref[(int64_t)m * D + j] = bridge_rows[r * D + j];
}

// ---- a filter stream: the filter stops after any frame; frames on which every lineage agrees go out ----
// The pending store keeps, per melody, the steps that are not emitted yet in a ring of `cap` slots: pending step j of
// melody m lives in slot (head[m] + j) % cap, its ancestors in panc [cap, R] (global rows, as anc) and its frames in phist
// [cap, R, D]; len[m] steps are live.  A melody's rows of a slot belong to that melody alone.
__device__ __forceinline__ int smc_local(int32_t row, int m, int P) { return min(max((int)row - m * P, 0), P - 1); }

// One workgroup per melody; thread p walks lineage p back through the n steps of the chunk just run (anc, hist) and then
// through the len[m] pending ones.  Step j is coalesced when all P lineages pass through one row; the first such step
// met on the way back, and every step before it, is final: from there on all threads hold the same row and copy its
// frames out (out [G, out_cap, D], row j = pending step j), and no further test is needed.  The chunk's steps that stay
// pending are appended to the ring.  The caller keeps len[m] + n <= min(cap, out_cap); a melody that breaks this is left
// as it is and reports ncommit[m] = -1.
__global__ __launch_bounds__(SMC_MAX_P) void smc_commit_kernel(int P, int D, int n, int R, const int32_t* anc,
                                                               const uint8_t* hist, int cap, int32_t* panc, uint8_t* phist,
                                                               int32_t* head, int32_t* len, int out_cap, int32_t* ncommit,
                                                               uint8_t* out, int words) {
  __shared__ int s_lo[SMC_MAX_P / 64], s_hi[SMC_MAX_P / 64];
  const int m = blockIdx.x, p = threadIdx.x, lane = p & 63, w = p >> 6, nw = blockDim.x >> 6;
  const int h0 = head[m], l0 = len[m];
  const int total = l0 + n;
  if (h0 < 0 || h0 >= cap || l0 < 0 || l0 > cap || total > cap || total > out_cap) {      // uniform over the workgroup
    if (p == 0) ncommit[m] = -1;
    return;
  }
  const int64_t first = (int64_t)m * P;
  int cur = min(p, P - 1);                       // the threads past P repeat lineage P - 1: no effect on the test
  bool one = false;
  int nc = 0;
  for (int j = total - 1; j >= 0; --j) {
    const bool old = j < l0;
    const int64_t at = old ? (int64_t)((h0 + j) % cap) * R : (int64_t)(j - l0) * R;
    cur = smc_local((old ? panc : anc)[at + first + cur], m, P);
    if (!one) {
      int lo = cur, hi = cur;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, 64));
        hi = max(hi, __shfl_xor(hi, o, 64));
      }
      if (lane == 0) { s_lo[w] = lo; s_hi[w] = hi; }
      __syncthreads();
      lo = s_lo[0], hi = s_hi[0];
      for (int i = 1; i < nw; ++i) { lo = min(lo, s_lo[i]); hi = max(hi, s_hi[i]); }
      __syncthreads();
      if (lo == hi) { one = true; nc = j + 1; }  // the same for every thread: steps 0 .. j are final
    }
    if (one) {
      const uint8_t* h = (old ? phist : hist) + (at + first + cur) * D;
      uint8_t* o = out + ((int64_t)m * out_cap + j) * D;
      for (int i = p; i < D; i += blockDim.x) o[i] = h[i];
    }
  }
  const int64_t nb = (int64_t)P * D;             // a melody's bytes of one step
  for (int j = max(l0, nc); j < total; ++j) {    // what stays pending of the chunk joins the ring; its slots hold nothing live
    const int64_t src = (int64_t)(j - l0) * R + first, dst = (int64_t)((h0 + j) % cap) * R + first;
    for (int q = p; q < P; q += blockDim.x) panc[dst + q] = anc[src + q];
    if (words) {
      const uint32_t* s4 = (const uint32_t*)(hist + src * D);
      uint32_t* d4 = (uint32_t*)(phist + dst * D);
      for (int64_t i = p; i < nb / 4; i += blockDim.x) d4[i] = s4[i];
    } else {
      for (int64_t i = p; i < nb; i += blockDim.x) phist[dst * D + i] = hist[src * D + i];
    }
  }
  __syncthreads();
  if (p == 0) {
    head[m] = (h0 + nc) % cap;
    len[m] = total - nc;
    ncommit[m] = nc;
  }
}

// One workgroup per melody with pick_of[m] != 0 (NULL: every melody): one particle drawn from the current weights as
// smc_backtrack_kernel draws its single path (the same scan, the same search, n = 1); its lineage through the pending
// steps goes to out [G, out_cap, D].  final_: the uniform is the backtrack's (SMC_STREAM) and nothing else is written.
// Otherwise the uniform is COLLAPSE_STREAM's and the melody restarts from the pick: anc_row [R] = the picked row for all
// of its rows and flag[m] = 1 (what smc_gather_kernel reads), logW = -log P, no pending step.
__global__ __launch_bounds__(SMC_MAX_P) void smc_collapse_kernel(int P, int D, int R, uint64_t seed, int64_t m0, uint32_t step,
                                                                 int final_, const int32_t* pick_of, double* logW, int cap,
                                                                 const int32_t* panc, const uint8_t* phist,
                                                                 const int32_t* head, int32_t* len, int out_cap,
                                                                 int32_t* picks, uint8_t* out, int32_t* anc_row,
                                                                 int32_t* flag) {
  __shared__ double red[SMC_MAX_P / 64];
  __shared__ double cum[SMC_MAX_P];
  const int m = blockIdx.x, p = threadIdx.x;
  if (pick_of && !pick_of[m]) return;            // uniform over the workgroup: such a melody is not touched at all
  const int h0 = head[m], l0 = len[m];
  const int64_t first = (int64_t)m * P;
  block_inclusive_scan(p < P ? exp(logW[first + p]) : 0.0, cum, red);
  if (h0 < 0 || h0 >= cap || l0 < 0 || l0 > cap || l0 > out_cap) {
    if (p == 0) picks[m] = -1;
    return;
  }
  const double u0 = smc_uniform(seed, m0 + m, step, final_ ? SMC_STREAM : COLLAPSE_STREAM);
  const int pick = systematic_pick(cum, P, 1.0, u0);
  int cur = pick;
  for (int j = l0 - 1; j >= 0; --j) {
    const int64_t at = (int64_t)((h0 + j) % cap) * R + first;
    cur = smc_local(panc[at + cur], m, P);
    const uint8_t* h = phist + (at + cur) * D;
    uint8_t* o = out + ((int64_t)m * out_cap + j) * D;
    for (int i = p; i < D; i += blockDim.x) o[i] = h[i];
  }
  if (p == 0) picks[m] = pick;
  if (final_) return;
  if (p < P) {
    anc_row[first + p] = (int32_t)(first + pick);
    logW[first + p] = -log((double)P);
  }
  if (p == 0) {
    flag[m] = 1;
    len[m] = 0;
  }
}

static inline int smc_block(int P) { return (P + 63) / 64 * 64; }

}  // namespace clv

using namespace clv;

extern "C" int clv_smc_sample(int R, int D, int P, int nsteps, int S, const float* p, const float* u, const uint8_t* clamp,
                              const int32_t* step_dev, float* x, double* ell, uint8_t* hist, void* stream) {
  if (R <= 0 || D <= 0 || P <= 0 || R % P != 0 || nsteps <= 0 || S < 0 || !p || !u || !clamp || !step_dev || !x || !ell ||
      !hist)
    return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_sample", s);
  hipLaunchKernelGGL(smc_sample_kernel, dim3((R + SMC_ROWS - 1) / SMC_ROWS), dim3(64 * SMC_ROWS), 0, s, R, D, P, nsteps, S,
                     p, u, clamp, step_dev, x, ell, hist);
  return launch_status();
}

extern "C" int clv_smc_resample(int G, int P, int nsteps, int S, uint64_t seed, int64_t m0, double tau, const double* ell,
                                double* logW, double* logZ, double* ess, int32_t* nres, int32_t* flag, int32_t* anc,
                                const int32_t* step_dev, void* stream) {
  if (G <= 0 || P <= 0 || P > SMC_MAX_P || nsteps <= 0 || S < 0 || m0 < 0 || !(tau >= 0.0 && tau <= 1.0) || !ell ||
      !logW || !logZ || !ess || !nres || !flag || !anc || !step_dev)
    return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_resample", s);
  hipLaunchKernelGGL(smc_resample_kernel<false>, dim3(G), dim3(smc_block(P)), 0, s, P, nsteps, S, seed, m0, tau, ell, logW,
                     logZ, ess, nres, flag, anc, step_dev, G * P, 0u, 0);
  return launch_status();
}

extern "C" int clv_smc_resample_conditional(int G, int P, int nsteps, int S, uint64_t seed, int64_t m0, double tau,
                                            const double* ell, double* logW, double* logZ, double* ess, int32_t* nres,
                                            int32_t* flag, int32_t* anc, const int32_t* step_dev, void* stream) {
  if (G <= 0 || P <= 0 || P > SMC_MAX_P || nsteps <= 0 || S < 0 || m0 < 0 || !(tau >= 0.0 && tau <= 1.0) || !ell ||
      !logW || !logZ || !ess || !nres || !flag || !anc || !step_dev)
    return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_resample_conditional", s);
  hipLaunchKernelGGL(smc_resample_kernel<true>, dim3(G), dim3(smc_block(P)), 0, s, P, nsteps, S, seed, m0, tau, ell, logW,
                     logZ, ess, nres, flag, anc, step_dev, G * P, 0u, 0);
  return launch_status();
}

extern "C" int clv_smc_pin_z(int G, int P, int L, int T, const float* z_ref, const int32_t* step_dev, float* z,
                             void* stream) {
  if (G <= 0 || P <= 0 || L <= 0 || T <= 0 || !z_ref || !step_dev || !z) return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX || (int64_t)G * L > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_pin_z", s);
  const int n = G * L;
  hipLaunchKernelGGL(smc_pin_z_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, P, L, T, z_ref, step_dev, z);
  return launch_status();
}

extern "C" int clv_smc_pin_frame(int G, int P, int D, int nsteps, int S, const uint8_t* x_ref, const float* bridge,
                                 const int32_t* step_dev, float* x, uint8_t* hist, void* stream) {
  if (G <= 0 || P <= 0 || D <= 0 || nsteps <= 0 || S < 0 || !x_ref || !step_dev || !x || !hist) return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_pin_frame", s);
  hipLaunchKernelGGL(smc_pin_frame_kernel, dim3((G + SMC_ROWS - 1) / SMC_ROWS), dim3(64 * SMC_ROWS), 0, s, G, P, D, nsteps,
                     S, x_ref, bridge, step_dev, x, hist);
  return launch_status();
}

extern "C" int clv_smc_backtrack_path(int G, int P, int nsteps, int S, int D, int L, const int32_t* picks,
                                      const int32_t* anc, const uint8_t* hist, const float* zhist, const float* bridge_rows,
                                      uint8_t* x_ref, float* z_ref, float* bridge_ref, uint8_t* renewed, void* stream) {
  if (G <= 0 || P <= 0 || nsteps <= 0 || S < 0 || D <= 0 || L <= 0 || !picks || !anc || !hist || !zhist || !x_ref ||
      !z_ref || !renewed)
    return CLV_EINVAL;
  if (S > 0 && (!bridge_rows != !bridge_ref)) return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_backtrack_path", s);
  hipLaunchKernelGGL(smc_backtrack_path_kernel, dim3((G + SMC_ROWS - 1) / SMC_ROWS), dim3(64 * SMC_ROWS), 0, s, G, P, nsteps,
                     S, D, L, picks, anc, hist, zhist, bridge_rows, x_ref, z_ref, bridge_ref, renewed);
  return launch_status();
}

extern "C" int clv_smc_gather(int R, int P, int nsteps, int S, int nbuf, float* const* bufs, const int* widths,
                              float* scratch, const int32_t* anc, const int32_t* flag, const int32_t* step_dev,
                              void* stream) {
  if (R <= 0 || P <= 0 || R % P != 0 || nsteps <= 0 || S < 0 || nbuf <= 0 || nbuf > SMC_MAX_BUFS || !bufs || !widths ||
      !scratch || !anc || !flag || !step_dev)
    return CLV_EINVAL;
  SmcBufs b{};
  int64_t off = 0;
  for (int i = 0; i < nbuf; ++i) {
    if (!bufs[i] || widths[i] <= 0) return CLV_EINVAL;
    b.buf[i] = bufs[i];
    b.width[i] = widths[i];
    b.off[i] = off;
    off += (int64_t)widths[i] * R;
  }
  b.n = nbuf;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_gather", s);
  const dim3 grid((R + SMC_ROWS - 1) / SMC_ROWS), block(64 * SMC_ROWS);
  hipLaunchKernelGGL(smc_gather_kernel<true>, grid, block, 0, s, R, P, nsteps, S, b, scratch, anc, flag, step_dev);
  hipLaunchKernelGGL(smc_gather_kernel<false>, grid, block, 0, s, R, P, nsteps, S, b, scratch, anc, flag, step_dev);
  return launch_status();
}

extern "C" int clv_smc_backtrack(int G, int P, int nsteps, int D, int n_out, uint64_t seed, int64_t m0, int step,
                                 const double* logW, const int32_t* anc, const uint8_t* hist, float* Xs, int32_t* picks,
                                 void* stream) {
  if (G <= 0 || P <= 0 || P > SMC_MAX_P || nsteps <= 0 || D <= 0 || n_out <= 0 || m0 < 0 || step < 0 || !logW || !anc ||
      !hist || !Xs)
    return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_backtrack", s);
  hipLaunchKernelGGL(smc_backtrack_kernel, dim3(G), dim3(smc_block(P)), 0, s, P, nsteps, D, n_out, seed, m0, step, logW, anc,
                     hist, Xs, picks, G * P);
  return launch_status();
}

extern "C" int clv_smc_init_w(int G, int P, int C, int mode, uint64_t seed, int64_t m0, const double* probs,
                              const float* mean, const float* log_var, float* wr, void* stream) {
  if (G <= 0 || P <= 0 || P > SMC_MAX_P || C < 2 || C > SMC_MAX_C || m0 < 0 || !wr) return CLV_EINVAL;
  if (mode == 0 ? !probs : (mode != 1 || !mean || !log_var)) return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_init_w", s);
  hipLaunchKernelGGL(smc_init_w_kernel, dim3(G), dim3(smc_block(P)), 0, s, P, C, mode, seed, m0, probs, mean, log_var, wr);
  return launch_status();
}

extern "C" int clv_smc_w_posterior(int G, int P, int C, int nsteps, int S, const double* logW, const float* wr,
                                   const int32_t* step_dev, double* out, void* stream) {
  if (G <= 0 || P <= 0 || P > SMC_MAX_P || C < 2 || C > SMC_MAX_C || nsteps <= 0 || S < 0 || !logW || !wr || !step_dev ||
      !out)
    return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_w_posterior", s);
  hipLaunchKernelGGL(smc_w_posterior_kernel, dim3(G), dim3(SMC_POST_THREADS), 0, s, P, C, nsteps, S, logW, wr, step_dev,
                     out);
  return launch_status();
}

extern "C" int clv_smc_take_w(int G, int P, int C, int n_out, const int32_t* picks, const float* wr, float* w_out,
                              void* stream) {
  if (G <= 0 || P <= 0 || P > SMC_MAX_P || C < 2 || C > SMC_MAX_C || n_out <= 0 || !picks || !wr || !w_out)
    return CLV_EINVAL;
  const int64_t n = (int64_t)G * n_out * C;
  if ((int64_t)G * P > INT32_MAX || n > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_take_w", s);
  hipLaunchKernelGGL(smc_take_w_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (int)n, P, C, n_out, picks, wr,
                     w_out);
  return launch_status();
}

// ---- a filter stream ----
extern "C" int clv_smc_resample_carry(int G, int P, int nsteps, int S, uint64_t seed, int64_t m0, double tau,
                                      const double* ell, double* logW, double* logZ, double* ess, int32_t* nres,
                                      int32_t* flag, int32_t* anc, const int32_t* step_dev, uint32_t t0, int carry,
                                      void* stream) {
  if (G <= 0 || P <= 0 || P > SMC_MAX_P || nsteps <= 0 || S < 0 || m0 < 0 || !(tau >= 0.0 && tau <= 1.0) || !ell ||
      !logW || !logZ || !ess || !nres || !flag || !anc || !step_dev)
    return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_resample_carry", s);
  hipLaunchKernelGGL(smc_resample_kernel<false>, dim3(G), dim3(smc_block(P)), 0, s, P, nsteps, S, seed, m0, tau, ell, logW,
                     logZ, ess, nres, flag, anc, step_dev, G * P, t0, carry);
  return launch_status();
}

extern "C" int clv_smc_commit(int G, int P, int D, int n, const int32_t* anc, const uint8_t* hist, int cap,
                              int32_t* pend_anc, uint8_t* pend_hist, int32_t* head, int32_t* len, int out_cap,
                              int32_t* ncommit, uint8_t* out, void* stream) {
  if (G <= 0 || P <= 0 || P > SMC_MAX_P || D <= 0 || n <= 0 || cap <= 0 || out_cap <= 0 || !anc || !hist || !pend_anc ||
      !pend_hist || !head || !len || !ncommit || !out)
    return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_commit", s);
  const int words = ((int64_t)P * D) % 4 == 0 && (((uintptr_t)hist | (uintptr_t)pend_hist) & 3) == 0;
  hipLaunchKernelGGL(smc_commit_kernel, dim3(G), dim3(smc_block(P)), 0, s, P, D, n, G * P, anc, hist, cap, pend_anc,
                     pend_hist, head, len, out_cap, ncommit, out, words);
  return launch_status();
}

extern "C" int clv_smc_collapse(int G, int P, int D, uint64_t seed, int64_t m0, uint32_t step, int final_pick,
                                const int32_t* pick_of, double* logW, int cap, const int32_t* pend_anc,
                                const uint8_t* pend_hist, const int32_t* head, int32_t* len, int out_cap, int32_t* picks,
                                uint8_t* out, int32_t* anc_row, int32_t* flag, void* stream) {
  if (G <= 0 || P <= 0 || P > SMC_MAX_P || D <= 0 || cap <= 0 || out_cap <= 0 || m0 < 0 || !logW || !pend_anc ||
      !pend_hist || !head || !len || !picks || !out)
    return CLV_EINVAL;
  if (!final_pick && (!anc_row || !flag)) return CLV_EINVAL;
  if ((int64_t)G * P > INT32_MAX) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_collapse", s);
  hipLaunchKernelGGL(smc_collapse_kernel, dim3(G), dim3(smc_block(P)), 0, s, P, D, G * P, seed, m0, step, final_pick,
                     pick_of, logW, cap, pend_anc, pend_hist, head, len, out_cap, picks, out, anc_row, flag);
  return launch_status();
}
