// key_track.hip -- key tracking: the label head of both families on every window of a batch of pieces, straight
// from the byte roll (clv_key_track_windows), and the HMM smoothing of the rows it leaves (clv_key_track_smooth).
//
// Windows.  A window is T frames of D bytes; at hop 1 consecutive windows share T - 1 of them, and as float rows of a GEMM
// they would be T * D * 4 bytes each.  Here a workgroup takes a tile of KT_WAVES consecutive windows of one piece and turns
// the tile's frames into ONE BIT PER NOTE, once: every lane loads a byte, a ballot is a 64-bit word of the tile's bit string
// (in LDS, at most 8 KB).  A window is the T * D bits from bit (its place in the tile) * min(hop, T) * D on, a wave owns a
// window, and its lanes hold the window's words (two per lane cover the 8192 bits the entry admits).  The notes that are on
// come out of those words in ascending order by scalar bit scans -- no memory access -- and are the rows of Kh the wave
// adds, KT_R loads of a lane in flight, lanes owning float2 columns of hW.  The sum of a window is one chain in ascending row
// order whatever else the launch holds, so a window's results do not depend on its tile, its piece's neighbours or hop.
// The Wargs layer (kernel staged in LDS once per workgroup, hW broadcast by readlane) and the softmax tail run in the same
// wave; nothing but wargs and logp is written.
//
// Smoothing.  One workgroup (one wave: lane = class) per piece, fp64, four sweeps over the piece's rows: Viterbi scores
// (kept in `post`, renormalised per row), the backtrack (which recomputes each maximum from the stored scores, first index
// first), the scaled forward pass (alpha in `post`) and the backward pass (beta renormalised per row; post = the marginals).
// Rows are requested KS_PF at a time ahead of their use.  Every sum has a fixed order: bitwise reproducible.
#include "common.h"
#include "philox.h"

namespace clv {

constexpr int KT_WAVES = 8;                      // windows of a tile = waves of a workgroup
constexpr int KT_NT = 64 * KT_WAVES;
constexpr int KT_R = 16;                         // rows of Kh a lane has in flight
constexpr int KT_MAXBITS = 8192;                 // T * D of a window
constexpr int KT_WORDS = KT_WAVES * KT_MAXBITS / 64 + 2;
constexpr int KT_MAXH = 128, KT_MAXC = 32;
constexpr uint32_t KT_STREAM = 0xFFFFFFFBu;      // KEY_STREAM of trainer.py

typedef unsigned long long u64;

struct KeyTrackArgs {
  int N, T, D, Hd, C, hop, K;
  const uint8_t* frames;
  const long long* piece_off;
  const long long* win_off;
  const float* Kh; const float* bh; const float* Ka; const float* ba;
  uint32_t k0, k1;
  long long piece0;
  float* wargs; float* logp;
};

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ u64 readlane64(u64 v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(KT_NT) void key_track_windows_kernel(KeyTrackArgs a) {
  __shared__ u64 s_bits[KT_WORDS];
  __shared__ float s_Ka[KT_MAXH * 2 * (KT_MAXC - 1)];
  __shared__ float s_ba[64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int T = a.T, D = a.D, Hd = a.Hd, C = a.C, hop = a.hop;
  const int C1 = C - 1, NA = 2 * C1, nx = T * D, n2 = Hd / 2;
  const int sl = hop < T ? hop : T;              // frame slots of the tile's bit string from one window to the next
  for (int i = tid; i < Hd * NA; i += KT_NT) s_Ka[i] = a.Ka[i];
  if (tid < NA) s_ba[tid] = a.ba[tid];           // (the tile loop's barrier stands between these stores and their readers)
  const int lc = min(lane, n2 - 1);
  const float2* K2 = reinterpret_cast<const float2*>(a.Kh);
  const float2 b2 = make_float2(a.bh[2 * lc], a.bh[2 * lc + 1]);
  const int nwords = (nx + 63) / 64;             // <= 128: words lane and lane + 64 of a window

  for (long long n = blockIdx.y; n < a.N; n += gridDim.y) {
    const long long f0 = a.piece_off[n], P = a.piece_off[n + 1] - f0;
    if (P < T || P >= (1ll << 24)) continue;     // no window / refused by the host (nothing is written)
    const long long J = (P - T) / hop + 1;
    const long long r0 = a.win_off[n];
    for (long long j0 = (long long)blockIdx.x * KT_WAVES; j0 < J; j0 += (long long)gridDim.x * KT_WAVES) {
      const int nw = (int)min((long long)KT_WAVES, J - j0);
      const int tbits = ((nw - 1) * sl + T) * D;                     // <= KT_WAVES * 8192; all inside the piece
      const uint8_t* base = a.frames + (size_t)(f0 + j0 * hop) * D;
      __syncthreads();                           // the previous tile's readers are done with s_bits
      // byte k of the tile's string: contiguous frames at hop < T, else window i = k / nx starts i * hop frames on
      for (int w0 = wave; w0 * 64 < tbits; w0 += 4 * KT_WAVES) {     // 4 loads of a lane in flight, none behind a condition
        unsigned char v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int k = min((w0 + q * KT_WAVES) * 64 + lane, tbits - 1);
          const long long goff = hop < T ? (long long)k : (long long)(k / nx) * hop * D + (k % nx);
          v[q] = base[goff];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int w = w0 + q * KT_WAVES;
          const u64 m = __ballot(w * 64 + lane < tbits && v[q] != 0);
          if (lane == 0 && w * 64 < tbits) s_bits[w] = m;
        }
      }
      if (tid < 2) s_bits[(tbits + 63) / 64 + tid] = 0;              // what the funnel reads past the last word
      __syncthreads();
      if (wave >= nw) continue;                  // (wave-uniform; the barriers above are reached by every wave: j0, J are the block's)
      const long long j = j0 + wave;
      const long long t = j * hop;               // < 2^24
      const int bit0 = wave * sl * D;
      auto word = [&](int l) -> u64 {            // bits [64 l, 64 l + 64) of this wave's window, zero from bit nx on
        const int lw = min(l, nwords - 1);
        const int bit = bit0 + 64 * lw, wi = bit >> 6, sh = bit & 63;
        const u64 lo = s_bits[wi], hi = s_bits[wi + 1];
        u64 v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
        const int lim = nx - 64 * l;
        if (lim < 64) v = lim > 0 ? v & ((1ull << lim) - 1ull) : 0ull;
        return v;
      };
      const u64 wA = word(lane), wB = word(lane + 64);
      u64 nzA = __ballot(wA != 0), nzB = __ballot(wB != 0);
      u64 m = 0;
      int rbase = 0;
      float2 acc = make_float2(0.f, 0.f);
      for (;;) {
        int kk[KT_R];
        bool on[KT_R];
#pragma unroll
        for (int q = 0; q < KT_R; ++q) {         // the next KT_R set bits, ascending: scalar work only
          if (m == 0) {
            if (nzA) {
              const int i = __builtin_ctzll(nzA);
              nzA &= nzA - 1;
              m = readlane64(wA, i); rbase = 64 * i;
            } else if (nzB) {
              const int i = __builtin_ctzll(nzB);
              nzB &= nzB - 1;
              m = readlane64(wB, i); rbase = 64 * (i + 64);
            }
          }
          on[q] = m != 0;
          const int bit = on[q] ? __builtin_ctzll(m) : 0;
          m = on[q] ? (m & (m - 1)) : 0;
          kk[q] = on[q] ? rbase + bit : 0;
        }
        if (!on[0]) break;
        float2 kr[KT_R];
#pragma unroll
        for (int q = 0; q < KT_R; ++q) kr[q] = K2[(size_t)kk[q] * n2 + lc];      // (an absent row reads row 0 and is not added)
#pragma unroll
        for (int q = 0; q < KT_R; ++q) {
          acc.x = on[q] ? acc.x + kr[q].x : acc.x;
          acc.y = on[q] ? acc.y + kr[q].y : acc.y;
        }
      }
      const float hx = fmaxf(acc.x + b2.x, 0.f), hy = fmaxf(acc.y + b2.y, 0.f);
      // wargs = hW . Ka + ba: lane = column, hW broadcast from the lanes that own it, ascending k
      const int cc = min(lane, NA - 1);
      float wa = 0.f;
      for (int k2 = 0; k2 < n2; ++k2) {
        const float h0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hx), k2));
        const float h1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, hy), k2));
        wa = fmaf(h0, s_Ka[(2 * k2) * NA + cc], wa);
        wa = fmaf(h1, s_Ka[(2 * k2 + 1) * NA + cc], wa);
      }
      wa += s_ba[cc];
      const size_t row = (size_t)(r0 + j);
      if (lane < NA) a.wargs[row * NA + lane] = wa;
      const float mean = wa;                                         // lanes < C1
      const float lv = __shfl(wa, min(C1 + lane, NA - 1), 64);       // lanes < C1
      const float NEG = -__builtin_huge_valf();
      float out;
      if (a.K == 0) {
        const float s = lane < C1 ? mean : lane == C1 ? 0.f : NEG;
        const float mx = wave_max(s);
        const float e = lane < C ? expf(s - mx) : 0.f;
        const float lse = mx + logf(wave_sum(e));
        out = s - lse;
      } else {
        const float sd = expf(0.5f * lv);
        const uint64_t i0 = ((((uint64_t)(a.piece0 + n)) << 24) + (uint64_t)t) * 32ull + (uint64_t)min(lane, 31);
        float pacc = 0.f;
        for (int k = 0; k < a.K; ++k) {
          const float eps = philox_normal_at(i0, a.k0, a.k1, KT_STREAM, (uint32_t)k);
          const float s = lane < C1 ? mean + sd * eps : lane == C1 ? 0.f : NEG;
          const float mx = wave_max(s);
          const float e = lane < C ? expf(s - mx) : 0.f;
          pacc += e / wave_sum(e);
        }
        out = logf(pacc / (float)a.K);
      }
      if (lane < C) a.logp[row * C + lane] = out;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
constexpr int KS_LD = 33;          // row stride of the transition matrices in LDS (doubles): rows and columns conflict-free
constexpr int KS_PF = 8;           // rows requested ahead

struct KeySmoothArgs {
  int N, C;
  const long long* win_off;
  const float* logp;
  const double* log_prior; const double* log_trans;
  double kappa;
  double* post; int32_t* path; double* log_evidence; double* piece_post;
};

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(64) void key_track_smooth_kernel(KeySmoothArgs a) {
  __shared__ double s_A[KT_MAXC * KS_LD], s_LA[KT_MAXC * KS_LD], s_v[2][KT_MAXC];
  const int n = blockIdx.x, c = threadIdx.x, C = a.C;
  const bool act = c < C;
  const int cc = min(c, C - 1);
  const long long r0 = a.win_off[n], J = a.win_off[n + 1] - r0;
  const double NEG = -__builtin_huge_val();
  const double lp = a.log_prior ? a.log_prior[cc] : -log((double)C);
  if (J <= 0) {                    // no rows: the prior, and nothing else
    const double mx = wave_max_d(act ? lp : NEG);
    const double e = act ? exp(lp - mx) : 0.0;
    const double s = wave_sum_d(e);
    if (act) a.piece_post[(size_t)n * C + c] = e / s;
    if (c == 0) a.log_evidence[n] = 0.0;
    return;
  }
  for (int i = c; i < C * C; i += 64) {
    const double la = a.log_trans[i];
    s_LA[(i / C) * KS_LD + i % C] = la;
    s_A[(i / C) * KS_LD + i % C] = exp(la);
  }
  __syncthreads();
  const float* X = a.logp + (size_t)r0 * C + cc;
  double* Pp = a.post + (size_t)r0 * C + cc;
  const double kappa = a.kappa;
  const float NEGF = -__builtin_huge_valf();
  // kappa * (row - its maximum), this lane's class
  auto emit = [&](float x) -> double {
    const float mx = wave_max(act ? x : NEGF);
    return kappa * ((double)x - (double)mx);
  };

  // ---- sweep 1: Viterbi scores, renormalised per row, into post ----
  double d = NEG;
  int buf = 0;
  for (long long jb = 0; jb < J; jb += KS_PF) {
    float x[KS_PF];
#pragma unroll
    for (int q = 0; q < KS_PF; ++q) x[q] = X[(size_t)min(jb + q, J - 1) * C];
#pragma unroll
    for (int q = 0; q < KS_PF; ++q) {
      const long long j = jb + q;
      if (j >= J) break;
      const double le = emit(x[q]);
      double v;
      if (j == 0) {
        v = lp + le;
      } else {
        if (act) s_v[buf][c] = d;
        __syncthreads();
        double best = NEG;
        for (int cp = 0; cp < C; ++cp) best = fmax(best, s_v[buf][cp] + s_LA[cp * KS_LD + cc]);
        buf ^= 1;
        v = best + le;
      }
      v = act ? v : NEG;
      d = v - wave_max_d(v);
      if (act) Pp[(size_t)j * C] = d;
    }
  }
  // ---- sweep 2: the backtrack; every maximum again from the stored scores, the first index first ----
  int nxt;
  {
    const double mx = wave_max_d(act ? d : NEG);
    nxt = __builtin_ctzll(__ballot(act && d == mx));
    if (c == 0) a.path[r0 + J - 1] = nxt;
  }
  for (long long jb = J - 2; jb >= 0; jb -= KS_PF) {
    double dv[KS_PF];
#pragma unroll
    for (int q = 0; q < KS_PF; ++q) dv[q] = Pp[(size_t)max(jb - q, 0ll) * C];
#pragma unroll
    for (int q = 0; q < KS_PF; ++q) {
      const long long j = jb - q;
      if (j < 0) break;
      const double v = act ? dv[q] + s_LA[cc * KS_LD + nxt] : NEG;
      const double mx = wave_max_d(v);
      nxt = __builtin_ctzll(__ballot(act && v == mx));
      if (c == 0) a.path[r0 + j] = nxt;
    }
  }
  __syncthreads();
  // ---- sweep 3: scaled forward pass, alpha into post; the evidence and the one-key posterior on the way ----
  double al = 0.0, logc = 0.0, summax = 0.0, S = 0.0;
  for (long long jb = 0; jb < J; jb += KS_PF) {
    float x[KS_PF];
#pragma unroll
    for (int q = 0; q < KS_PF; ++q) x[q] = X[(size_t)min(jb + q, J - 1) * C];
#pragma unroll
    for (int q = 0; q < KS_PF; ++q) {
      const long long j = jb + q;
      if (j >= J) break;
      const float mx = wave_max(act ? x[q] : NEGF);
      const double eh = act ? exp(kappa * ((double)x[q] - (double)mx)) : 0.0;
      summax += (double)mx;
      S += (double)x[q];
      double v;
      if (j == 0) {
        v = exp(lp) * eh;
      } else {
        if (act) s_v[buf][c] = al;
        __syncthreads();
        double s = 0.0;
        for (int cp = 0; cp < C; ++cp) s = fma(s_v[buf][cp], s_A[cp * KS_LD + cc], s);
        buf ^= 1;
        v = s * eh;
      }
      v = act ? v : 0.0;
      const double cj = wave_sum_d(v);
      al = v / cj;
      logc += log(cj);
      if (act) Pp[(size_t)j * C] = al;
    }
  }
  if (c == 0) a.log_evidence[n] = logc + kappa * summax;
  {
    const double z = act ? lp + kappa * S : NEG;
    const double mx = wave_max_d(z);
    const double e = act ? exp(z - mx) : 0.0;
    const double s = wave_sum_d(e);
    if (act) a.piece_post[(size_t)n * C + c] = e / s;
  }
  // ---- sweep 4: backward pass; beta renormalised per row, post = alpha * beta normalised ----
  double be = act ? 1.0 : 0.0;     // row J - 1 keeps alpha (its beta is 1)
  for (long long jb = J - 2; jb >= 0; jb -= KS_PF) {
    float x[KS_PF];
    double av[KS_PF];
#pragma unroll
    for (int q = 0; q < KS_PF; ++q) {
      x[q] = X[(size_t)(max(jb - q, 0ll) + 1) * C];
      av[q] = Pp[(size_t)max(jb - q, 0ll) * C];
    }
#pragma unroll
    for (int q = 0; q < KS_PF; ++q) {
      const long long j = jb - q;
      if (j < 0) break;
      const float mx = wave_max(act ? x[q] : NEGF);
      const double eh = act ? exp(kappa * ((double)x[q] - (double)mx)) : 0.0;
      if (act) s_v[buf][c] = eh * be;
      __syncthreads();
      double s = 0.0;
      for (int cn = 0; cn < C; ++cn) s = fma(s_A[cc * KS_LD + cn], s_v[buf][cn], s);
      buf ^= 1;
      s = act ? s : 0.0;
      be = s / wave_max_d(s);
      const double g = act ? av[q] * be : 0.0;
      const double gs = wave_sum_d(g);
      if (act) Pp[(size_t)j * C] = g / gs;
    }
  }
}

}  // namespace clv

using namespace clv;

extern "C" int clv_key_track_windows(int N, int T, int D, int Hd, int C, int hop, int K, const uint8_t* frames,
                                     const int64_t* piece_off, const int64_t* win_off, const float* Kh, const float* bh,
                                     const float* Ka, const float* ba, uint64_t seed, int64_t piece0, float* wargs, float* logp,
                                     void* stream) {
  if (N <= 0 || T <= 0 || D < 2 || D > KT_MAXH || D % 2 || Hd < 2 || Hd > KT_MAXH || Hd % 2 || C < 2 || C > KT_MAXC ||
      (long long)T * D > KT_MAXBITS || hop < 1 || K < 0 || K > 1024 || piece0 < 0)
    return CLV_EINVAL;
  if (!frames || !piece_off || !win_off || !Kh || !bh || !Ka || !ba || !wargs || !logp || ((uintptr_t)Kh) % 8) return CLV_EINVAL;
  KeyTrackArgs a{N, T, D, Hd, C, hop, K, frames, (const long long*)piece_off, (const long long*)win_off, Kh, bh, Ka, ba,
                 (uint32_t)seed, (uint32_t)(seed >> 32), (long long)piece0, wargs, logp};
  // the entry does not know the pieces' lengths (they are on the device): workgroups (x, y) walk the tiles x, x + gx, .. of
  // the pieces y, y + gy, ..; a few thousand workgroups in all, so that few pieces still fill the device
  int gx = 4096 / N;
  gx = gx < 8 ? 8 : gx > 1024 ? 1024 : gx;
  const int gy = N < 65535 ? N : 65535;
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("key_track_windows", s);
  hipLaunchKernelGGL(key_track_windows_kernel, dim3(gx, gy), dim3(KT_NT), 0, s, a);
  return launch_status();
}

extern "C" int clv_key_track_smooth(int N, int C, const int64_t* win_off, const float* logp, const double* log_prior,
                                    const double* log_trans, double kappa, double* post, int32_t* path, double* log_evidence,
                                    double* piece_post, void* stream) {
  if (N <= 0 || C < 2 || C > KT_MAXC || !(kappa > 0.0) || !(kappa <= 1.0)) return CLV_EINVAL;
  if (!win_off || !logp || !log_trans || !post || !path || !log_evidence || !piece_post) return CLV_EINVAL;
  KeySmoothArgs a{N, C, (const long long*)win_off, logp, log_prior, log_trans, kappa, post, path, log_evidence, piece_post};
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("key_track_smooth", s);
  hipLaunchKernelGGL(key_track_smooth_kernel, dim3(N), dim3(64), 0, s, a);
  return launch_status();
}
