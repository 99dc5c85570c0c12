// stats.hip -- the roll statistics audit: per piece of a batch of byte rolls, nine histograms of its texture
// (clv_roll_stats): which notes sound, on which scale degrees, how many at once, at which intervals, for how long, how much
// a frame differs from the one before it, how the outer voices step, how wide the chord is.  All integer work, one launch
// behind a memset of the table.
//
// A workgroup of RS_NT threads takes tiles of RS_NT consecutive frames of the whole string of frames (a grid-stride loop),
// one frame per thread.  The tile is packed from the bytes into LDS as 128-bit frames (bit d = note d, D <= 116, as in
// novelty.hip) with a halo: the frame before the tile (for the onset, `change` and the steps) and the Lmax - 1 frames after
// it (for the length of a note that starts in the tile).  A frame's piece is found by binary search in `off`; a neighbour
// frame of another piece counts as silence for the note lengths and does not exist for `change` and the steps, so nothing
// is counted across a piece boundary, whatever the tile boundaries are.  A note is counted by the thread of its ONSET frame:
// it walks forward through the halo and drops the notes that ended into the bin of their length, what still sounds after
// Lmax - 1 further frames (or a longer run, which no thread follows to its end) goes to the last bin.
//
// The counts go to a 32-bit histogram of ONE piece in LDS (a tile holds at most RS_NT * 116 cells, far below 2^32); a tile
// that covers several pieces handles them one after another.  Its non-zero bins are then added to the piece's row of the
// table with 64-bit integer atomics: integer sums do not depend on their order, so a row is bit for bit independent of the
// tiling, the grid, the other pieces of the batch and the order of the atomics.  No float anywhere.
#include "common.h"

namespace clv {

constexpr int RS_NT = 256;                       // frames of a tile = threads of a workgroup
constexpr int RS_MAXD = 116, RS_MAXL = 64, RS_MAXN = 1 << 20;
constexpr int RS_V = CLV_STATS_VOICES, RS_C = CLV_STATS_CHANGE, RS_M = CLV_STATS_STEP;
constexpr int RS_NF = 1 + RS_NT + RS_MAXL - 1;   // frames of a tile in LDS: one before, the tile, Lmax - 1 after
constexpr int RS_MAXGRID = 2048;               // workgroups of a launch: 8 per CU; more tiles are walked in a grid-stride loop
constexpr int RS_MAXS = 3 * RS_MAXD + 12 + (RS_V + 1) + RS_MAXL + (RS_C + 1) + 2 * (2 * RS_M + 1);

__host__ __device__ inline int rs_columns(int D, int Lmax) {
  return 3 * D + 12 + (RS_V + 1) + Lmax + (RS_C + 1) + 2 * (2 * RS_M + 1);
}

struct StatsArgs {
  int N, D, Lmax, low, S;
  long long F, ntiles;
  const uint8_t* roll; const long long* off; const int32_t* tonic;
  unsigned long long* table;
};

// bit i = byte i of x is not zero: the high bit of every non-zero byte, then the eight of them gathered by one multiply
__device__ __forceinline__ unsigned rs_bits8(unsigned long long x) {
  const unsigned long long m = 0x7f7f7f7f7f7f7f7full;
  const unsigned long long t = (((x & m) + m) | x) & ~m;
  return (unsigned)(((t >> 7) * 0x0102040810204080ull) >> 56);
}
// notes 32 w .. 32 w + 31 of a frame as bits: eight bytes per load where the word's bytes are 8-byte aligned (every frame
// at D = 88 and a 16-byte aligned roll) and eight of them are left in the frame, byte by byte otherwise
__device__ __forceinline__ unsigned rs_pack_word(const uint8_t* row, int w, int D) {
  unsigned v = 0;
  const int d0 = 32 * w, nd = min(32, D - d0);
  const bool aligned = ((uintptr_t)(row + d0) & 7) == 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int b = 8 * k;
    if (aligned && b + 8 <= nd) {
      v |= rs_bits8(*reinterpret_cast<const unsigned long long*>(row + d0 + b)) << b;
    } else {
      for (int j = b; j < min(nd, b + 8); ++j) v |= (row[d0 + j] != 0 ? 1u : 0u) << j;
    }
  }
  return v;
}
__device__ __forceinline__ bool rs_any(uint4 v) { return (v.x | v.y | v.z | v.w) != 0u; }
__device__ __forceinline__ int rs_popc(uint4 v) { return __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w); }
__device__ __forceinline__ uint4 rs_and(uint4 a, uint4 b) { return make_uint4(a.x & b.x, a.y & b.y, a.z & b.z, a.w & b.w); }
__device__ __forceinline__ uint4 rs_andn(uint4 a, uint4 b) { return make_uint4(a.x & ~b.x, a.y & ~b.y, a.z & ~b.z, a.w & ~b.w); }
__device__ __forceinline__ uint4 rs_xor(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
// the lowest / highest set note of a frame that has one
__device__ __forceinline__ int rs_lowest(uint4 v) {
  return v.x ? __builtin_ctz(v.x) : v.y ? 32 + __builtin_ctz(v.y) : v.z ? 64 + __builtin_ctz(v.z) : 96 + __builtin_ctz(v.w);
}
__device__ __forceinline__ int rs_highest(uint4 v) {
  return v.w ? 127 - __builtin_clz(v.w) : v.z ? 95 - __builtin_clz(v.z) : v.y ? 63 - __builtin_clz(v.y) : 31 - __builtin_clz(v.x);
}
// v >> k over the 128 bits, 1 <= k <= 127: whole words first (selects, no indexed registers), then the bits
__device__ __forceinline__ uint4 rs_shr(uint4 v, int k) {
  const int q = k >> 5, r = k & 31;
  const unsigned a0 = q == 0 ? v.x : q == 1 ? v.y : q == 2 ? v.z : v.w;
  const unsigned a1 = q == 0 ? v.y : q == 1 ? v.z : q == 2 ? v.w : 0u;
  const unsigned a2 = q == 0 ? v.z : q == 1 ? v.w : 0u;
  const unsigned a3 = q == 0 ? v.w : 0u;
  typedef unsigned long long u64;
  return make_uint4((unsigned)((((u64)a1 << 32) | a0) >> r), (unsigned)((((u64)a2 << 32) | a1) >> r),
                    (unsigned)((((u64)a3 << 32) | a2) >> r), a3 >> r);
}

__global__ __launch_bounds__(RS_NT) void roll_stats_kernel(StatsArgs a) {
  __shared__ uint4 sF[RS_NF];                    // sF[1 + i] = frame g0 + i; zero outside 0 .. F-1
  __shared__ unsigned sH[RS_MAXS];               // the histogram of the piece in hand
  __shared__ int sPiece[RS_NT];                  // the piece of every frame of the tile
  const int tid = threadIdx.x, lane = tid & 63;
  const int D = a.D, Lmax = a.Lmax, S = a.S;
  const int nf = 1 + RS_NT + Lmax - 1;
  // the sections' first bins
  const int oDeg = D, oVoi = oDeg + 12, oInt = oVoi + RS_V + 1, oDur = oInt + D, oChg = oDur + Lmax, oTop = oChg + RS_C + 1,
            oBot = oTop + 2 * RS_M + 1, oSpan = oBot + 2 * RS_M + 1;

  for (long long k = blockIdx.x; k < a.ntiles; k += gridDim.x) {
    const long long g0 = k * RS_NT;
    const int nv = (int)min((long long)RS_NT, a.F - g0);               // frames of this tile
    __syncthreads();                             // the tile before this one is read to its end
    for (int i = tid; i < 4 * nf; i += RS_NT) {
      const long long g = g0 - 1 + (i >> 2);
      reinterpret_cast<unsigned*>(sF)[i] = g >= 0 && g < a.F ? rs_pack_word(a.roll + (size_t)g * D, i & 3, D) : 0u;
    }
    const long long g = g0 + tid;
    int n = -1;
    long long p0 = 0, p1 = 0;
    if (tid < nv) {                              // the piece of frame g: off[n] <= g < off[n + 1]
      int lo = 0, hi = a.N;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.off[mid] <= g) lo = mid; else hi = mid;
      }
      n = lo; p0 = a.off[n]; p1 = a.off[n + 1];
    }
    sPiece[tid] = n;
    __syncthreads();

    for (int first = 0; first < nv;) {           // the pieces of the tile, one after another (block-uniform)
      const int cur = sPiece[first];
      const long long end = a.off[cur + 1];
      const int next = (int)min((long long)nv, max(end - g0, (long long)first + 1));
      for (int b = tid; b < S; b += RS_NT) sH[b] = 0u;
      __syncthreads();
      if (tid >= first && tid < next && n == cur) {
        const uint4 zero = make_uint4(0, 0, 0, 0);
        const uint4 f = sF[1 + tid];
        const bool has_prev = g > p0;
        const uint4 prev = has_prev ? sF[tid] : zero;
        const int tn0 = a.tonic ? a.tonic[cur] : 0;
        const int tn = tn0 >= 0 && tn0 < 12 ? tn0 : 0;
        // pitch, degree: one count per sounding cell
        const unsigned fw[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          unsigned m = fw[w];
          while (m) {
            const int d = 32 * w + __builtin_ctz(m);
            m &= m - 1;
            atomicAdd(&sH[d], 1u);
            atomicAdd(&sH[oDeg + (d + a.low + 12 - tn) % 12], 1u);
          }
        }
        const int nn = rs_popc(f);
        atomicAdd(&sH[oVoi + min(nn, RS_V)], 1u);
        if (nn) {
          const int lowest = rs_lowest(f), span = rs_highest(f) - lowest;
          atomicAdd(&sH[oSpan + span], 1u);
          // interval k: the pairs of notes k apart = the notes of f that f shifted down by k also has.  Every lane starts
          // at another k, so that the lanes of a wave do not all add to the same bin in the same instruction
          int kk = span ? 1 + lane % span : 1;
          for (int j = 0; j < span; ++j) {
            const int c = rs_popc(rs_and(f, rs_shr(f, kk)));
            if (c) atomicAdd(&sH[oInt + kk], (unsigned)c);
            kk = kk == span ? 1 : kk + 1;
          }
        }
        if (has_prev) {
          atomicAdd(&sH[oChg + min(rs_popc(rs_xor(f, prev)), RS_C)], 1u);
          if (nn && rs_any(prev)) {
            const int top = rs_highest(f) - rs_highest(prev), bot = rs_lowest(f) - rs_lowest(prev);
            atomicAdd(&sH[oTop + min(max(top, -RS_M), RS_M) + RS_M], 1u);
            atomicAdd(&sH[oBot + min(max(bot, -RS_M), RS_M) + RS_M], 1u);
          }
        }
        // duration: the notes that start here, followed to their ends
        uint4 alive = rs_andn(f, prev);
        for (int l = 1; l < Lmax && rs_any(alive); ++l) {
          const uint4 nxt = g + l < p1 ? sF[1 + tid + l] : zero;
          const int c = rs_popc(rs_andn(alive, nxt));
          if (c) atomicAdd(&sH[oDur + l - 1], (unsigned)c);
          alive = rs_and(alive, nxt);
        }
        const int c = rs_popc(alive);
        if (c) atomicAdd(&sH[oDur + Lmax - 1], (unsigned)c);
      }
      __syncthreads();
      for (int b = tid; b < S; b += RS_NT) {
        const unsigned c = sH[b];
        if (c) atomicAdd(&a.table[(size_t)cur * S + b], (unsigned long long)c);
      }
      __syncthreads();                           // sH is read before the next piece clears it
      first = next;
    }
  }
}

}  // namespace clv

using namespace clv;

extern "C" int clv_roll_stats_column_count(int D, int Lmax) {
  if (D < 1 || D > RS_MAXD || Lmax < 1 || Lmax > RS_MAXL) return 0;
  return rs_columns(D, Lmax);
}

extern "C" int clv_roll_stats(int N, int D, int Lmax, int low, int64_t F, const uint8_t* roll, const int64_t* off,
                              const int32_t* tonic, int64_t* table, void* stream) {
  if (N < 1 || N > RS_MAXN || D < 1 || D > RS_MAXD || Lmax < 1 || Lmax > RS_MAXL || low < 0 || low > 127 || F < 0)
    return CLV_EINVAL;
  if ((!roll && F > 0) || !off || !table) return CLV_EINVAL;
  StatsArgs a{};
  a.N = N; a.D = D; a.Lmax = Lmax; a.low = low; a.S = rs_columns(D, Lmax);
  a.F = F; a.ntiles = (F + RS_NT - 1) / RS_NT;
  a.roll = roll; a.off = (const long long*)off; a.tonic = tonic; a.table = (unsigned long long*)table;
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("roll_stats", s);
  CLV_HIP_TRY(hipMemsetAsync(table, 0, sizeof(int64_t) * (size_t)N * (size_t)a.S, s));
  if (a.ntiles > 0) {                            // pieces of 0 frames appear in no tile: their rows stay zero
    const int grid = (int)(a.ntiles < RS_MAXGRID ? a.ntiles : RS_MAXGRID);
    hipLaunchKernelGGL(roll_stats_kernel, dim3(grid), dim3(RS_NT), 0, s, a);
  }
  return launch_status();
}
