// novelty.hip -- the novelty audit: for every window of W frames of a batch of query pieces, the nearest
// window of a corpus of pieces in Hamming distance, over every corpus offset and every transposition in -S..S that keeps the
// query window's notes on the keyboard (clv_roll_nearest).  All integer work; three launches.
//
// Packing.  Every frame of both rolls becomes 128 bits, one uint4 (bit d = note d, D <= 116), every corpus frame gets the
// number of its piece if a window may start there (W frames left in the piece) and -1 otherwise, and the key of every
// query window is set to all ones.
//
// Search.  dist of the window pair (a, g) is a sum of W frame distances down a diagonal of the frame-by-frame distance
// matrix, so a lane that walks a diagonal keeps a running sum: the next pair costs the frame pair that enters and the one
// that leaves.  A workgroup takes a tile of RN_TQ consecutive window starts of ONE query piece and walks corpus tiles of
// RN_NT diagonals: lane l of tile k owns the diagonal that starts at (a0, k RN_NT - (RN_TQ - 1) + l) and makes at most
// RN_TQ steps down it, so over all k every pair (a0 + i, g) is met exactly once, those with g < 0 or past the corpus's end
// on zero frames.  Both tiles sit in LDS as 16-byte frames with their W - 1 halo; the corpus is ONE string of frames, and
// what keeps a window inside its piece is a penalty word per corpus start (from the packing launch's piece numbers, the
// query piece's `exclude` folded in): the running sum itself never looks at piece ends.  A transposition is a 128-bit
// shift of the query tile, made once per (corpus tile, shift) in LDS; the step loop reads it at a wave-uniform address.
// At step i every lane holds a candidate for the same query window a0 + i, so each lane keeps its own minimum per step in
// registers -- best[RN_TQ], the step loop is unrolled -- over every corpus tile and shift the workgroup walks, and only
// then are the minima folded: across the wave, across the waves through LDS, and with one 64-bit atomic minimum per (query
// window, workgroup) into the key buffer.  The key is (dist + penalties, rank(s), g) in one word, so the minimum over a
// totally ordered key is the contract's lexicographic choice whatever the tiling or the order of the atomics.
//
// Unpacking.  key -> dist, shift, cframe; a key that kept a penalty had no candidate.
#include "common.h"

namespace clv {

constexpr int RN_NT = 256;                       // diagonals of a corpus tile = threads of a workgroup
constexpr int RN_TQ = 32;                        // window starts of a query tile = steps down a diagonal
constexpr int RN_WAVES = RN_NT / 64;
constexpr int RN_MAXW = 1024, RN_MAXD = 116, RN_MAXS = 12;
constexpr unsigned RN_BIG = 1u << 20;            // added to dist (< 2^18) where the corpus window is no candidate
constexpr unsigned RN_NOSHIFT = 1u << 31;        // set in the key where the shift is not allowed for the query window
constexpr unsigned RN_NONE = 1u << 25;           // key >> 32 at or above this: a penalty is in it

typedef unsigned long long u64;

struct RollArgs {
  int Nq, Nc, W, hop, S, D;
  long long Fq, Fc, Wq, ntiles;
  const uint8_t* q_roll; const long long* q_off;
  const uint8_t* c_roll; const long long* c_off;
  const long long* qwin_off; const int32_t* exclude;
  uint4* qp; uint4* cp; int32_t* cinfo; u64* keys;
  int32_t* dist; int32_t* shift; long long* cframe;
};

// ---- packing ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pack_word(const uint8_t* row, int w, int D) {
  unsigned v = 0;
  const int d0 = 32 * w, nd = min(32, D - d0);
  for (int k = 0; k < nd; ++k) v |= (row[d0 + k] != 0 ? 1u : 0u) << k;
  return v;
}

__global__ __launch_bounds__(256) void roll_pack_kernel(RollArgs a) {
  const long long nq = 4 * a.Fq, nc = 4 * a.Fc;
  const long long total = max(max(nq, nc), a.Wq);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    if (i < nq) reinterpret_cast<unsigned*>(a.qp)[i] = pack_word(a.q_roll + (size_t)(i >> 2) * a.D, (int)(i & 3), a.D);
    if (i < nc) reinterpret_cast<unsigned*>(a.cp)[i] = pack_word(a.c_roll + (size_t)(i >> 2) * a.D, (int)(i & 3), a.D);
    if (i < a.Fc) {                              // the piece of corpus frame i: the last m with c_off[m] <= i
      int lo = 0, hi = a.Nc;                     // c_off[lo] <= i < c_off[hi] (c_off[0] = 0, c_off[Nc] = Fc)
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.c_off[mid] <= i) lo = mid; else hi = mid;
      }
      a.cinfo[i] = i + a.W <= a.c_off[lo + 1] ? lo : -1;
    }
    if (i < a.Wq) a.keys[i] = ~0ull;
  }
}

// ---- search ----------------------------------------------------------------------------------------------------------------
// s > 0: towards the higher notes.  Bits pushed past either end are dropped: only a shift that is not allowed loses any
__device__ __forceinline__ uint4 shift128(uint4 v, int s) {
  uint4 r = v;
  if (s > 0) {
    const int k = s, b = 32 - s;
    r.w = (v.w << k) | (v.z >> b);
    r.z = (v.z << k) | (v.y >> b);
    r.y = (v.y << k) | (v.x >> b);
    r.x = v.x << k;
  } else if (s < 0) {
    const int k = -s, b = 32 + s;
    r.x = (v.x >> k) | (v.y << b);
    r.y = (v.y >> k) | (v.z << b);
    r.z = (v.z >> k) | (v.w << b);
    r.w = v.w >> k;
  }
  return r;
}
__device__ __forceinline__ int frame_dist(uint4 q, uint4 c) {
  return __popc(q.x ^ c.x) + __popc(q.y ^ c.y) + __popc(q.z ^ c.z) + __popc(q.w ^ c.w);
}
__device__ __forceinline__ u64 wave_min_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// LDS of the search launch: sQ0 [nfq] the query tile, sQ [nfq] the same shifted, sC [nfc] the corpus tile (uint4 each),
// sRed [RN_WAVES * RN_TQ] u64, sPen [nfc] unsigned, sQpen [RN_TQ], sMask [RN_TQ]
__host__ __device__ inline int rn_nfq(int W) { return RN_TQ + W - 1; }
__host__ __device__ inline int rn_nfc(int W) { return RN_NT + RN_TQ + W - 2; }
inline size_t rn_lds_bytes(int W) {
  return 16 * (size_t)(2 * rn_nfq(W) + rn_nfc(W)) + 8 * RN_WAVES * RN_TQ + 4 * (size_t)(rn_nfc(W) + 2 * RN_TQ);
}

__global__ __launch_bounds__(RN_NT) void roll_search_kernel(RollArgs a) {
  extern __shared__ uint4 rn_smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int W = a.W, S = a.S, D = a.D, hop = a.hop;
  const int nfq = rn_nfq(W), nfc = rn_nfc(W);
  uint4* sQ0 = rn_smem;
  uint4* sQ = sQ0 + nfq;
  uint4* sC = sQ + nfq;
  u64* sRed = reinterpret_cast<u64*>(sC + nfc);
  unsigned* sPen = reinterpret_cast<unsigned*>(sRed + RN_WAVES * RN_TQ);
  unsigned* sQpen = sPen + nfc;
  unsigned* sMask = sQpen + RN_TQ;
  const uint4 zero = make_uint4(0, 0, 0, 0);

  for (long long n = blockIdx.y; n < a.Nq; n += gridDim.y) {
    const long long f0 = a.q_off[n], P = a.q_off[n + 1] - f0;
    if (P < W) continue;                         // no window (block-uniform, like every `continue` below)
    const long long r0 = a.qwin_off[n];
    const int excl = a.exclude ? a.exclude[n] : -1;
    for (long long a0 = 0; a0 + W <= P; a0 += RN_TQ) {
      const int nw = (int)min((long long)RN_TQ, P - W + 1 - a0);       // window starts of this tile
      if ((a0 + hop - 1) / hop * hop >= a0 + nw) continue;             // none of them on the hop grid
      const int nf = (int)min((long long)nfq, P - a0);                 // frames the piece still has
      __syncthreads();                           // the tile before this one is read to its end
      for (int t = tid; t < nfq; t += RN_NT) sQ0[t] = t < nf ? a.qp[f0 + a0 + t] : zero;
      __syncthreads();
      if (tid < RN_TQ) {                         // the shifts window a0 + tid allows, as bits s + S; 0: no row for it
        unsigned m = 0;
        if (tid < nw && (a0 + tid) % hop == 0) {
          uint4 o = zero;
          for (int t = 0; t < W; ++t) {
            const uint4 v = sQ0[tid + t];
            o.x |= v.x; o.y |= v.y; o.z |= v.z; o.w |= v.w;
          }
          int smin = -S, smax = S;
          if (o.x | o.y | o.z | o.w) {
            const int lo = o.x ? __builtin_ctz(o.x) : o.y ? 32 + __builtin_ctz(o.y) : o.z ? 64 + __builtin_ctz(o.z) : 96 + __builtin_ctz(o.w);
            const int hi = o.w ? 127 - __builtin_clz(o.w) : o.z ? 95 - __builtin_clz(o.z) : o.y ? 63 - __builtin_clz(o.y) : 31 - __builtin_clz(o.x);
            smin = max(smin, -lo);
            smax = min(smax, D - 1 - hi);
          }
          for (int s = smin; s <= smax; ++s) m |= 1u << (s + S);
        }
        sMask[tid] = m;
      }
      __syncthreads();
      unsigned any = 0;
      for (int i = 0; i < RN_TQ; ++i) any |= sMask[i];
      u64 best[RN_TQ];
#pragma unroll
      for (int i = 0; i < RN_TQ; ++i) best[i] = ~0ull;

      for (long long k = blockIdx.x; k < a.ntiles; k += gridDim.x) {
        const long long G0 = k * RN_NT - (RN_TQ - 1);
        __syncthreads();                         // the corpus tile before this one is read to its end
        for (int j = tid; j < nfc; j += RN_NT) {
          const long long g = G0 + j;
          const bool in = g >= 0 && g < a.Fc;
          sC[j] = in ? a.cp[g] : zero;
          int m = -1;
          if (in && j < RN_NT + RN_TQ - 1) m = a.cinfo[g];
          sPen[j] = m >= 0 && m != excl ? 0u : RN_BIG;
        }
        for (int s = -S; s <= S; ++s) {
          if (!((any >> (s + S)) & 1u)) continue;
          __syncthreads();                       // sC is written; the shift before this one is read to its end
          for (int t = tid; t < nfq; t += RN_NT) sQ[t] = shift128(sQ0[t], s);
          if (tid < RN_TQ) sQpen[tid] = (sMask[tid] >> (s + S)) & 1u ? 0u : RN_NOSHIFT;
          __syncthreads();
          const unsigned rank = s == 0 ? 0u : s < 0 ? (unsigned)(-2 * s - 1) : (unsigned)(2 * s);
          int sum = 0;
          for (int t = 0; t < W; ++t) sum += frame_dist(sQ[t], sC[tid + t]);
          const unsigned glo = (unsigned)(G0 + tid);                   // (a start below 0 carries RN_BIG)
#pragma unroll
          for (int i = 0; i < RN_TQ; ++i) {
            if (i < nw) {                        // (no break: best[] keeps constant indices, in registers)
              const unsigned hi = ((((unsigned)sum + sPen[tid + i]) << 5) | rank) | sQpen[i];
              const u64 key = ((u64)hi << 32) | (u64)(glo + (unsigned)i);
              best[i] = key < best[i] ? key : best[i];
              if (i + 1 < nw) sum += frame_dist(sQ[i + W], sC[tid + i + W]) - frame_dist(sQ[i], sC[tid + i]);
            }
          }
        }
      }
      // fold: the lanes of a wave, the waves through LDS, one atomic per window that has a row
#pragma unroll
      for (int i = 0; i < RN_TQ; ++i) {
        if (i < nw) {
          const u64 v = wave_min_u64(best[i]);
          if (lane == 0) sRed[wave * RN_TQ + i] = v;
        }
      }
      __syncthreads();
      if (tid < nw && (a0 + tid) % hop == 0) {
        u64 v = sRed[tid];
        for (int w = 1; w < RN_WAVES; ++w) v = min(v, sRed[w * RN_TQ + tid]);
        if ((unsigned)(v >> 32) < RN_NONE) atomicMin(&a.keys[r0 + (a0 + tid) / hop], v);
      }
    }
  }
}

// ---- unpacking -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void roll_unpack_kernel(RollArgs a) {
  for (long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x; r < a.Wq; r += (long long)gridDim.x * blockDim.x) {
    const u64 key = a.keys[r];
    const unsigned hi = (unsigned)(key >> 32);
    if (hi >= RN_NONE) {
      a.dist[r] = -1; a.shift[r] = 0; a.cframe[r] = -1;
    } else {
      const int rank = (int)(hi & 31u);
      a.dist[r] = (int)(hi >> 5);
      a.shift[r] = rank == 0 ? 0 : (rank & 1) ? -(rank + 1) / 2 : rank / 2;
      a.cframe[r] = (long long)(key & 0xFFFFFFFFull);
    }
  }
}

inline size_t rn_workspace_bytes(long long Fq, long long Fc, long long Wq) {
  return 16 * (size_t)(Fq + Fc) + align_up(4 * (size_t)Fc, 16) + 8 * (size_t)Wq + 64;
}

}  // namespace clv

using namespace clv;

extern "C" size_t clv_roll_nearest_workspace_bytes(int64_t Fq, int64_t Fc, int64_t Wq) {
  if (Fq < 0 || Fc < 0 || Wq < 0 || Fq >= (1ll << 31) || Fc >= (1ll << 31) || Wq >= (1ll << 31)) return 0;
  return rn_workspace_bytes(Fq, Fc, Wq);
}

extern "C" int clv_roll_nearest(int Nq, int Nc, int W, int hop, int S, int D, int64_t Fq, int64_t Fc, int64_t Wq,
                                const uint8_t* q_roll, const int64_t* q_off, const uint8_t* c_roll, const int64_t* c_off,
                                const int64_t* qwin_off, const int32_t* exclude, void* workspace, size_t workspace_bytes,
                                int32_t* dist, int32_t* shift, int64_t* cframe, void* stream) {
  if (Nq < 1 || Nc < 1 || W < 1 || W > RN_MAXW || hop < 1 || S < 0 || S > RN_MAXS || D < 1 || D > RN_MAXD) return CLV_EINVAL;
  if (Fq < 0 || Fc < 0 || Wq < 0 || Fq >= (1ll << 31) || Fc >= (1ll << 31) || Wq >= (1ll << 31)) return CLV_EINVAL;
  if (!q_roll || !q_off || !c_roll || !c_off || !qwin_off || !workspace || !dist || !shift || !cframe) return CLV_EINVAL;
  if (((uintptr_t)workspace) % 16 || workspace_bytes < rn_workspace_bytes(Fq, Fc, Wq)) return CLV_EINVAL;
  if (Wq == 0) return CLV_OK;                    // no query window: nothing to write
  RollArgs a{};
  a.Nq = Nq; a.Nc = Nc; a.W = W; a.hop = hop; a.S = S; a.D = D;
  a.Fq = Fq; a.Fc = Fc; a.Wq = Wq;
  // diagonals start at -(RN_TQ - 1) .. Fc - W: a corpus shorter than a window has no tile, and every key stays all ones
  a.ntiles = Fc >= W ? (Fc - W + RN_TQ + RN_NT - 1) / RN_NT : 0;
  a.q_roll = q_roll; a.q_off = (const long long*)q_off; a.c_roll = c_roll; a.c_off = (const long long*)c_off;
  a.qwin_off = (const long long*)qwin_off; a.exclude = exclude;
  char* ws = (char*)workspace;
  a.qp = (uint4*)ws; ws += 16 * (size_t)Fq;
  a.cp = (uint4*)ws; ws += 16 * (size_t)Fc;
  a.cinfo = (int32_t*)ws; ws += align_up(4 * (size_t)Fc, 16);
  a.keys = (u64*)ws;
  a.dist = dist; a.shift = shift; a.cframe = (long long*)cframe;
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("roll_nearest", s);
  const long long items = 4 * Fq > 4 * Fc ? (4 * Fq > Wq ? 4 * Fq : Wq) : (4 * Fc > Wq ? 4 * Fc : Wq);
  const int gp = (int)((items + 255) / 256 < 4096 ? (items + 255) / 256 : 4096);
  hipLaunchKernelGGL(roll_pack_kernel, dim3(gp), dim3(256), 0, s, a);
  if (a.ntiles > 0) {
    // workgroups (x, y) walk the corpus tiles x, x + gx, .. for the query pieces y, y + gy, ..: a few thousand in all,
    // so that few query pieces still fill the device and many do not multiply the atomics
    long long gx = (4096 + Nq - 1) / Nq;
    gx = gx < 1 ? 1 : gx > a.ntiles ? a.ntiles : gx;
    const int gy = Nq < 65535 ? Nq : 65535;
    hipLaunchKernelGGL(roll_search_kernel, dim3((unsigned)gx, gy), dim3(RN_NT), rn_lds_bytes(W), s, a);
  }
  const int gu = (int)((Wq + 255) / 256 < 4096 ? (Wq + 255) / 256 : 4096);
  hipLaunchKernelGGL(roll_unpack_kernel, dim3(gu), dim3(256), 0, s, a);
  return launch_status();
}
