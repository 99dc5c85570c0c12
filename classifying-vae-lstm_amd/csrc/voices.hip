// voices.hip -- sampling a frame given how many of its notes sound (voice-count constraints).
//
// The output head factorises over the D notes, so the number of sounding notes of a frame is a sum of independent
// Bernoullis and conditioning the frame on lo <= count <= hi is an exact dynamic programme over (note, count):
//   B[D][c] = [lo <= c <= hi],   B[j][c] = (1 - q_j) B[j+1][c] + q_j B[j+1][c+1]   (fp64, q = clip(p, 1e-7, 1 - 1e-7) in
//   float32, 0 / 1 for a note the roll forces), B[0][0] = P(count in range | forced notes);
//   notes ascending, c = 0: a forced note takes its value; a free one a = q_j B[j+1][c+1], b = (1 - q_j) B[j+1][c],
//   x_j = 0 if a == 0, 1 if b == 0, else [u_j <= a / B[j][c]]; c += x_j.
// Sixteen lanes per row, one per count c = 0 .. 15 (hi <= 15), four rows per wave: lane c carries B[j+1][c] in a register
// down the notes, takes B[j+1][c+1] from its neighbour, and decides x_j AS IF the walk stood at count c -- one bit per
// (note, count) in two 64-bit masks per lane (D <= 128).  The table itself is never stored.  The walk up the notes then only
// follows bits: the mask word of lane c of the row's group.  The frame's (q, u) pairs are staged once through LDS (8 bytes
// per note; q = 0 / 1 exactly marks a forced note, which no clipped probability equals), where the sixteen lanes of a row
// read them by broadcast.  No atomics, every output element has one owner; every address is formed before the first load.
//   clv_bernoulli_sample_voices   the voices twin of clv_bernoulli_sample_clamped (the frame chains)
//   clv_smc_sample_voices         the voices twin of clv_smc_sample (the particle filter): also the uint8 history row and
//                                 ell = (sum over forced notes of log q) + log B[0][0]
// A frame whose pair is (0, 255), or any pair that is not lo <= hi <= 15, is free: it takes the twins' own draw and weight,
// bit for bit (the forced notes' logs are summed in clv_smc_sample's order: notes l and l + 64, then the butterfly).
#include "common.h"

namespace clv {

constexpr int VOICES_GROUP = 16;        // lanes per row: the counts 0 .. 15
constexpr int VOICES_WAVE_ROWS = 64 / VOICES_GROUP;
constexpr int VOICES_WAVES = 4;         // waves per workgroup
constexpr int VOICES_ROWS = VOICES_WAVES * VOICES_WAVE_ROWS;      // rows per workgroup
constexpr int VOICES_MAX_D = 128;       // two 64-bit decision masks per lane
constexpr int VOICES_NOTES = VOICES_MAX_D / VOICES_GROUP;         // notes a lane loads and stores: c, c + 16, ...
constexpr int VOICES_MAX_COUNT = VOICES_GROUP - 1;
constexpr float VOICES_CLIP_LO = 1e-7f, VOICES_CLIP_HI = 1.0f - 1e-7f;    // SMC_CLIP_* of csrc/smc.hip

// one row's notes downwards: B (lane c: [lo <= c <= hi] in, B[0][c] out) and the decision bits of notes < 64 and >= 64
__device__ __forceinline__ void voices_recurse(int D, int c, const float2* qu, double& B, uint64_t& m0, uint64_t& m1) {
#pragma clang fp contract(off)          // two products and a sum, each rounded, as the fp64 reference forms them
  for (int j = D - 1; j >= 0; --j) {
    const float2 v = qu[j];
    const double qd = (double)v.x;                   // 0 / 1: the roll forces the note
    double Bn = __shfl_down(B, 1, VOICES_GROUP);     // B[j+1][c+1]
    if (c == VOICES_GROUP - 1) Bn = 0.0;             // B[.][16] = 0
    const double a = qd * Bn, b = (1.0 - qd) * B;
    const double Bj = b + a;
    const bool forced = v.x == 0.f || v.x == 1.f;
    const bool one = forced ? v.x == 1.f : a == 0.0 ? false : b == 0.0 ? true : (double)v.y <= a / Bj;
    const uint64_t bit = (uint64_t)(one ? 1 : 0) << (j & 63);
    if (j >= 64) m1 |= bit; else m0 |= bit;
    B = Bj;
  }
}

// one row's notes upwards from count 0: the bits of the frame, the same in the row's sixteen lanes
__device__ __forceinline__ void voices_walk(int D, uint64_t m0, uint64_t m1, uint64_t& x0, uint64_t& x1) {
  int c = 0;
  for (int j = 0; j < D; ++j) {
    const uint64_t m = j >= 64 ? m1 : m0;
    const uint32_t mine = (j & 32) ? (uint32_t)(m >> 32) : (uint32_t)m;
    const uint32_t w = (uint32_t)__shfl((int)mine, c & (VOICES_GROUP - 1), VOICES_GROUP);
    const uint32_t bit = (w >> (j & 31)) & 1u;
    if (j >= 64) x1 |= (uint64_t)bit << (j & 63); else x0 |= (uint64_t)bit << (j & 63);
    c += (int)bit;
  }
}

template <bool SMC>
__global__ __launch_bounds__(64 * VOICES_WAVES) void voices_sample_kernel(int R, int D, int P, int nsteps, int S, const float* p,
                                                                          const float* u, const uint8_t* clamp,
                                                                          const uint8_t* voices, const int32_t* step_dev,
                                                                          float* x, double* ell, uint8_t* hist, double* logb) {
  __shared__ float2 qu_all[VOICES_ROWS][VOICES_MAX_D + 2];      // + 2: the four rows of a wave read four different banks
  const int slot = threadIdx.x / VOICES_GROUP, c = threadIdx.x % VOICES_GROUP;
  const int row_ = blockIdx.x * VOICES_ROWS + slot;
  const bool live = row_ < R;
  const int row = live ? row_ : R - 1;               // a slot past the end recomputes the last row and stores nothing
  const int k = *step_dev - S;
  const bool on = k >= 0 && k < nsteps;
  const int64_t base = (int64_t)row * D;
  const int64_t frame = (int64_t)(row / P) * nsteps + (on ? k : 0);       // the melody's roll row and pair
  const uint8_t* cr = clamp ? clamp + frame * D : nullptr;
  const uint8_t* vp = voices + frame * 2;
  uint8_t* hr = SMC ? hist + ((int64_t)(on ? k : 0) * R + row) * D : nullptr;
  float2* qu = qu_all[slot];
  const int lo = vp[0], hi = vp[1];
  float xs[VOICES_NOTES];
  double t[VOICES_NOTES];
#pragma unroll
  for (int i = 0; i < VOICES_NOTES; ++i) {
    const int j = c + VOICES_GROUP * i;
    xs[i] = 0.f;
    t[i] = 0.0;
    if (j < D) {
      const float pj = p[base + j], uj = u[base + j];
      const int cb = on && cr ? cr[j] : 255;
      const float q = fminf(fmaxf(pj, VOICES_CLIP_LO), VOICES_CLIP_HI);
      // the twins' draw and weight: [u <= p], the roll's byte over it, the forced notes' log q
      xs[i] = cb <= 1 ? (float)cb : (uj <= pj) ? 1.f : 0.f;
      if (SMC && cb <= 1) t[i] = cb ? log((double)q) : log(1.0 - (double)q);
      qu[j] = make_float2(cb == 0 ? 0.f : cb == 1 ? 1.f : q, uj);
    }
  }
  __syncthreads();
  const bool counted = on && lo <= hi && hi <= VOICES_MAX_COUNT;
  double lb = 0.0;
  if (__any(counted)) {                              // the wave's rows run together; a free row's result is dropped
    double B = (counted && c >= lo && c <= hi) ? 1.0 : 0.0;
    uint64_t m0 = 0, m1 = 0, x0 = 0, x1 = 0;
    voices_recurse(D, c, qu, B, m0, m1);
    voices_walk(D, m0, m1, x0, x1);
    if (counted) {
#pragma unroll
      for (int i = 0; i < VOICES_NOTES; ++i) {
        const int j = c + VOICES_GROUP * i;
        xs[i] = (float)(((i < 4 ? x0 : x1) >> (j & 63)) & 1u);
      }
      if (c == 0) lb = log(B);                       // B[0][0]
    }
  }
#pragma unroll
  for (int i = 0; i < VOICES_NOTES; ++i) {
    const int j = c + VOICES_GROUP * i;
    if (live && j < D) {
      x[base + j] = xs[i];
      if (SMC && on) hr[j] = (uint8_t)xs[i];
    }
  }
  if (SMC && on) {
    // clv_smc_sample's order: lane l of its wave holds notes l and l + 64, then the butterfly over 32, 16, 8, 4, 2, 1
    double l = ((t[0] + t[4]) + (t[2] + t[6])) + ((t[1] + t[5]) + (t[3] + t[7]));
#pragma unroll
    for (int o = VOICES_GROUP / 2; o > 0; o >>= 1) l += __shfl_xor(l, o, VOICES_GROUP);
    if (live && c == 0) ell[row] = l + lb;           // lb = 0 for a free frame: the twin's sum, bit for bit
  }
  if (logb && live && c == 0) logb[row] = lb;
}

static inline bool voices_args_ok(int64_t R, int D, int nsteps, int S, const void* p, const void* u, const void* voices,
                                  const void* step_dev, const void* x) {
  return R > 0 && R <= INT32_MAX && D > 0 && D <= VOICES_MAX_D && nsteps > 0 && S >= 0 && p && u && voices && step_dev && x;
}

}  // namespace clv

using namespace clv;

extern "C" int clv_bernoulli_sample_voices(int64_t n, int D, int nsteps, int S, const float* p, const float* u,
                                           const uint8_t* clamp, const uint8_t* voices, const int32_t* step_dev, float* x,
                                           double* logb, void* stream) {
  if (n <= 0 || D <= 0 || n % D != 0 || !voices_args_ok(n / D, D, nsteps, S, p, u, voices, step_dev, x)) return CLV_EINVAL;
  const int R = (int)(n / D);
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("bernoulli_sample_voices", s);
  hipLaunchKernelGGL(voices_sample_kernel<false>, dim3((R + VOICES_ROWS - 1) / VOICES_ROWS), dim3(64 * VOICES_WAVES), 0, s, R,
                     D, 1, nsteps, S, p, u, clamp, voices, step_dev, x, (double*)nullptr, (uint8_t*)nullptr, logb);
  return launch_status();
}

extern "C" int clv_smc_sample_voices(int R, int D, int P, int nsteps, int S, const float* p, const float* u,
                                     const uint8_t* clamp, const uint8_t* voices, const int32_t* step_dev, float* x,
                                     double* ell, uint8_t* hist, double* logb, void* stream) {
  if (P <= 0 || R % P != 0 || !ell || !hist || !voices_args_ok(R, D, nsteps, S, p, u, voices, step_dev, x)) return CLV_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  ProfScope pr("smc_sample_voices", s);
  hipLaunchKernelGGL(voices_sample_kernel<true>, dim3((R + VOICES_ROWS - 1) / VOICES_ROWS), dim3(64 * VOICES_WAVES), 0, s, R, D,
                     P, nsteps, S, p, u, clamp, voices, step_dev, x, ell, hist, logb);
  return launch_status();
}
