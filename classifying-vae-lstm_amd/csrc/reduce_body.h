// reduce_body.h -- the workgroup bodies of the split-K reduction launch: a pending job's blocks, the loss means, the few-row
// rider products.  Shared by gemm.hip (clv_splitk_reduce_multi: a launch of their own, every block at full occupancy) and
// tail_launch.hip (the same blocks behind the workgroups of the hW kernel gradient, at that product's footprint).
#pragma once
#include "reduce_job.h"

namespace clv {

__device__ __forceinline__ float apply_act(float v, int act, float aux) {
  if (act == CLV_ACT_RELU) return fmaxf(v, 0.f);
  if (act == CLV_ACT_SIGMOID) return sigmoidf_(v);
  if (act == CLV_ACT_MASKPOS) return aux > 0.f ? v : 0.f;
  return v;
}

// sum of `splits` partial slabs + epilogue.  64 outputs x 4 slab-lanes per block, 8 loads in flight
// per thread (a serial loop over the slabs is latency-bound: ~0.5 us per dependent HBM load).
//
// LO (both forms): the slab sums for a launch that gets few waves per CU (tail_launch.hip: 12, the hW product's LDS).  The
// plain form has its eight loads in flight only in the main loop; a job with fewer slabs than one round (the LSTM products: 64
// slabs, two thirds of a step's slab bytes) runs the tail loop, ONE load per thread outstanding, and only occupancy hides
// that.  LO requests the eight loads of every round together whatever the slab count -- unconditional, slab index clamped,
// the value masked where it is added -- and adds them in the plain form's order: in a whole round value i goes to
// accumulator i, in the last, partial round every value goes to accumulator 0, in slab order.  The other side of each
// select adds +0.0f, which leaves an accumulator as it is (one that started at +0 is never -0), so the sums are bit for
// bit the plain form's.
template <bool LO>
__device__ __forceinline__ void reduce_block(const ReduceJob& g, unsigned blk, float (*red)[64]) {
  const int splits = g.splits;
  const size_t mn = (size_t)g.M * g.N;
  const int ex = threadIdx.x & 63, zy = threadIdx.x >> 6;
  const size_t idx = (size_t)blk * 64 + ex;
  float v = 0.f;
  if constexpr (LO) {
    const float* p = g.partial + (idx < mn ? idx : 0);
    float a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = 0.f;
    for (int z = zy; z < splits; z += 32) {
      float r[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = p[(size_t)min(z + 4 * i, splits - 1) * mn];
      const bool full = z + 28 < splits;
      a[0] += r[0];
#pragma unroll
      for (int i = 1; i < 8; ++i) {
        const float t = z + 4 * i < splits ? r[i] : 0.f;
        a[i] += full ? t : 0.f;
        a[0] += full ? 0.f : t;
      }
    }
    v = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
  } else if (idx < mn) {
    const float* p = g.partial + idx;
    int z = zy;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f;
    for (; z + 28 < splits; z += 32) {
      a0 += p[(size_t)(z + 0) * mn]; a1 += p[(size_t)(z + 4) * mn]; a2 += p[(size_t)(z + 8) * mn];
      a3 += p[(size_t)(z + 12) * mn]; a4 += p[(size_t)(z + 16) * mn]; a5 += p[(size_t)(z + 20) * mn];
      a6 += p[(size_t)(z + 24) * mn]; a7 += p[(size_t)(z + 28) * mn];
    }
    for (; z < splits; z += 4) a0 += p[(size_t)z * mn];
    v = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
  }
  red[zy][ex] = v;
  __syncthreads();
  if (zy == 0 && idx < mn) {
    v = (red[0][ex] + red[1][ex]) + (red[2][ex] + red[3][ex]);
    int row = (int)(idx / g.N);
    const int col = (int)(idx % g.N);
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MAX_PROB; ++i)
      if (i < g.nprob && row >= g.prob[i].row0) pi = i;
    float* Cptr = g.prob[pi].C;
    const int ldc = g.prob[pi].ldc;
    row -= g.prob[pi].row0;
    v *= g.alpha;
    if (g.bias) v += g.bias[col];
    const size_t o = (size_t)row * ldc + col;
    if (g.beta != 0.f) v += g.beta * Cptr[o];
    v = apply_act(v, g.act, g.act == CLV_ACT_MASKPOS ? g.aux[o] : 0.f);
    Cptr[o] = v;
  }
}
// The same with 4 consecutive outputs per thread (16-byte loads of the slabs: a quarter of the load instructions; the
// slabs of the bf16 weight-gradient kernel are 32 MB per LSTM).  Needs N % 4 == 0 and 16-byte aligned rows everywhere
// (reduce_vec_ok).  A block still covers 64 outputs (the same number of blocks: ~4 per CU for an LSTM's gradients), now
// as 16 float4 lanes x 16 slab lanes, every thread with up to 8 loads in flight.
template <bool LO>
__device__ __forceinline__ void reduce_block_v4(const ReduceJob& g, unsigned blk, float4 (*red)[16]) {
  const int splits = g.splits;
  const size_t mn = (size_t)g.M * g.N;
  const int ex = threadIdx.x & 15, zy = threadIdx.x >> 4;
  const size_t idx = ((size_t)blk * 16 + ex) * 4;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  auto add = [](float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; };
  if constexpr (LO) {
    const float* p = g.partial + (idx < mn ? idx : 0);          // (mn % 4 == 0: a float4 inside the slab is whole)
    auto at = [&](int z) { return *reinterpret_cast<const float4*>(p + (size_t)z * mn); };
    auto pick = [](bool c, const float4& b) { return make_float4(c ? b.x : 0.f, c ? b.y : 0.f, c ? b.z : 0.f, c ? b.w : 0.f); };
    float4 a[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = v;
    for (int z = zy; z < splits; z += 128) {
      float4 r[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) r[i] = at(min(z + 16 * i, splits - 1));
      const bool full = z + 112 < splits;
      add(a[0], r[0]);
#pragma unroll
      for (int i = 1; i < 8; ++i) {
        const bool in = z + 16 * i < splits;
        add(a[i], pick(full, r[i]));
        add(a[0], pick(in && !full, r[i]));
      }
    }
    add(a[0], a[1]); add(a[2], a[3]); add(a[4], a[5]); add(a[6], a[7]);
    add(a[0], a[2]); add(a[4], a[6]);
    add(a[0], a[4]);
    v = a[0];
  } else if (idx < mn) {
    const float* p = g.partial + idx;
    auto at = [&](int z) { return *reinterpret_cast<const float4*>(p + (size_t)z * mn); };
    float4 a0 = v, a1 = v, a2 = v, a3 = v, a4 = v, a5 = v, a6 = v, a7 = v;
    int z = zy;
    for (; z + 112 < splits; z += 128) {
      add(a0, at(z)); add(a1, at(z + 16)); add(a2, at(z + 32)); add(a3, at(z + 48));
      add(a4, at(z + 64)); add(a5, at(z + 80)); add(a6, at(z + 96)); add(a7, at(z + 112));
    }
    for (; z < splits; z += 16) add(a0, at(z));
    add(a0, a1); add(a2, a3); add(a4, a5); add(a6, a7);
    add(a0, a2); add(a4, a6);
    add(a0, a4);
    v = a0;
  }
  red[zy][ex] = v;
  __syncthreads();
  if (zy == 0 && idx < mn) {
    float4 t[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                  // fixed order: ((0+1)+(2+3)) per group of four, then the groups
      t[q] = red[4 * q][ex];
      float4 u = red[4 * q + 2][ex];
      add(t[q], red[4 * q + 1][ex]); add(u, red[4 * q + 3][ex]);
      add(t[q], u);
    }
    add(t[0], t[1]); add(t[2], t[3]); add(t[0], t[2]);
    v = t[0];
    int row = (int)(idx / g.N);
    const int col = (int)(idx % g.N);
    int pi = 0;
#pragma unroll
    for (int i = 1; i < MAX_PROB; ++i)
      if (i < g.nprob && row >= g.prob[i].row0) pi = i;
    float* Cptr = g.prob[pi].C;
    row -= g.prob[pi].row0;
    const size_t o = (size_t)row * g.prob[pi].ldc + col;
    float r[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float w = r[j] * g.alpha;
      if (g.bias) w += g.bias[col + j];
      if (g.beta != 0.f) w += g.beta * Cptr[o + j];
      r[j] = apply_act(w, g.act, g.act == CLV_ACT_MASKPOS ? g.aux[o + j] : 0.f);
    }
    *reinterpret_cast<float4*>(Cptr + o) = make_float4(r[0], r[1], r[2], r[3]);
  }
}
inline bool reduce_vec_ok(const ReduceJob& j) {
  if (j.N % 4 || ((uintptr_t)j.partial) % 16) return false;
  const int n = j.nprob == 0 ? 1 : j.nprob;
  for (int i = 0; i < n; ++i)
    if (j.prob[i].ldc % 4 || ((uintptr_t)j.prob[i].C) % 16) return false;
  return true;
}
inline unsigned reduce_blocks(const ReduceJob& j) {          // j.pad_ = 1: the 4-wide form
  const size_t mn = (size_t)j.M * j.N;
  return (unsigned)((mn + 63) / 64);
}
// several pending reductions in one launch (the weight gradients of a whole backward pass)
constexpr int MAX_JOBS = 16;
struct ReduceTable { int njobs; unsigned blk0[MAX_JOBS + 1]; ReduceJob job[MAX_JOBS]; };
// up to five strided means riding in the same launch (the loss terms of a step): one block each, after the jobs' blocks
struct MeanTerms { int n_terms; const float* x[5]; int n[5]; int stride[5]; float* out; };
__device__ __forceinline__ void mean_block(const MeanTerms& m, int k, float4 (*red)[16]) {
  const float* x = m.x[0]; int n = m.n[0], st = m.stride[0];
#pragma unroll
  for (int i = 1; i < 5; ++i)
    if (k == i) { x = m.x[i]; n = m.n[i]; st = m.stride[i]; }
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int i = threadIdx.x;
  if (st == 1 && ((uintptr_t)x) % 16 == 0) {        // contiguous term: float4 loads, 4 in flight per thread
    const float4* x4 = reinterpret_cast<const float4*>(x);
    const int n4 = n / 4;
    int j = threadIdx.x;
    for (; j + 768 < n4; j += 1024) {
      const float4 a = x4[j], b = x4[j + 256], c = x4[j + 512], d = x4[j + 768];
      a0 += (a.x + a.y) + (a.z + a.w); a1 += (b.x + b.y) + (b.z + b.w);
      a2 += (c.x + c.y) + (c.z + c.w); a3 += (d.x + d.y) + (d.z + d.w);
    }
    for (; j < n4; j += 256) { const float4 a = x4[j]; a0 += (a.x + a.y) + (a.z + a.w); }
    i = 4 * n4 + threadIdx.x;
  }
  for (; i + 768 < n; i += 1024) {
    a0 += x[(size_t)i * st]; a1 += x[(size_t)(i + 256) * st];
    a2 += x[(size_t)(i + 512) * st]; a3 += x[(size_t)(i + 768) * st];
  }
  for (; i < n; i += 256) a0 += x[(size_t)i * st];
  const float acc = wave_sum((a0 + a1) + (a2 + a3));
  float* part = reinterpret_cast<float*>(red);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) m.out[k] = ((part[0] + part[1]) + (part[2] + part[3])) / (float)n;
}
// Few-row products over a short K riding in the same launch (clv_splitk_reduce_multi): C[r, :] = sum_k A[k, r] B[k, :] for
// r < R rows of A [K, lda] plus, with `ones`, the column sums of B as one more row -- the label rows and the bias of an
// LSTM input-kernel gradient over K = batch rows of sum_t dz (cl_vrnn/model.py:194,223: the RepeatVector(W) columns).
// A launch of their own was 8.6 us for 2 MFLOP.  A block owns 64 columns; 4 k-lanes stride through K with every row's
// accumulator in registers; the A chunk is staged in LDS (broadcast reads).
constexpr int SR_ROWS = 16, SR_KC = 32;
constexpr int SR_LDS_FLOATS = 3 * SR_ROWS * 64;      // the block's LDS scratch (sbuf), 16-byte aligned
struct SkinnySet { const float* A; int lda, R, ones; const float* B; int ldb, N, K; float* C; int ldc; float* Cones; };
struct SkinnyRider { int nsets, blocks_per_set; SkinnySet set[2]; };
__device__ __forceinline__ void skinny_rider_block(const SkinnyRider& sr, int blk, float* sbuf) {
  // one buffer: the A^T chunk [SR_KC][SR_ROWS] while the products run, the k-lanes' partial sums [3][SR_ROWS][64] at the end
  float (*At)[SR_ROWS] = reinterpret_cast<float (*)[SR_ROWS]>(sbuf);
  const bool second = blk >= sr.blocks_per_set;
  const SkinnySet g = second ? sr.set[1] : sr.set[0];
  const int tid = threadIdx.x, cx = tid & 63, kl = tid >> 6;
  const int col = (blk - (second ? sr.blocks_per_set : 0)) * 64 + cx;
  const bool live = col < g.N;
  const int R = g.R + (g.ones ? 1 : 0);
  float acc[SR_ROWS];
#pragma unroll
  for (int r = 0; r < SR_ROWS; ++r) acc[r] = 0.f;
  for (int kc = 0; kc < g.K; kc += SR_KC) {
    __syncthreads();
#pragma unroll
    for (int e0 = 0; e0 < SR_KC * SR_ROWS; e0 += 256) {      // A^T chunk (+ the ones row) -> LDS
      const int e = e0 + tid, kk = e / SR_ROWS, r = e % SR_ROWS, k = kc + kk;
      float v = 0.f;
      if (k < g.K) v = r < g.R ? g.A[(size_t)k * g.lda + r] : (r == g.R && g.ones ? 1.f : 0.f);
      At[kk][r] = v;
    }
    float breg[SR_KC / 4];
#pragma unroll
    for (int j = 0; j < SR_KC / 4; ++j) {                    // this thread's B values of the chunk, all in flight
      const int k = kc + kl + 4 * j;
      const float v = g.B[(size_t)min(k, g.K - 1) * g.ldb + min(col, g.N - 1)];
      breg[j] = v * ((live && k < g.K) ? 1.f : 0.f);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SR_KC / 4; ++j) {
      const float4* arow = reinterpret_cast<const float4*>(At[kl + 4 * j]);
#pragma unroll
      for (int r4 = 0; r4 < SR_ROWS / 4; ++r4) {
        const float4 a = arow[r4];
        acc[4 * r4] = fmaf(a.x, breg[j], acc[4 * r4]);
        acc[4 * r4 + 1] = fmaf(a.y, breg[j], acc[4 * r4 + 1]);
        acc[4 * r4 + 2] = fmaf(a.z, breg[j], acc[4 * r4 + 2]);
        acc[4 * r4 + 3] = fmaf(a.w, breg[j], acc[4 * r4 + 3]);
      }
    }
  }
  __syncthreads();
  float (*redk)[SR_ROWS][64] = reinterpret_cast<float (*)[SR_ROWS][64]>(sbuf);
  if (kl > 0) {
#pragma unroll
    for (int r = 0; r < SR_ROWS; ++r) redk[kl - 1][r][cx] = acc[r];
  }
  __syncthreads();
  if (kl == 0 && live) {
#pragma unroll
    for (int r = 0; r < SR_ROWS; ++r) {
      if (r < R) {
        const float v = ((acc[r] + redk[0][r][cx]) + (redk[1][r][cx] + redk[2][r][cx]));
        if (r < g.R) g.C[(size_t)r * g.ldc + col] = v;
        else g.Cones[col] = v;
      }
    }
  }
}

// One block of the launch behind its first `bid` blocks: riders first (they are short chains of dependent loads, and at the
// end of the grid they were the launch's tail: the launch got as much longer as the products' own launch had taken), then
// the jobs' blocks, then the means.  lds: SR_LDS_FLOATS floats, 16-byte aligned (every role's scratch overlays it).
template <bool LO>
__device__ __forceinline__ void reduce_launch_block(const ReduceTable& t, const MeanTerms& m, const SkinnyRider& sr, unsigned blk, float* lds) {
  float4 (*red)[16] = reinterpret_cast<float4 (*)[16]>(lds);
  const unsigned nrider = (unsigned)(sr.nsets * sr.blocks_per_set);
  if (blk < nrider) { skinny_rider_block(sr, blk, lds); return; }
  const unsigned bid = blk - nrider;
  if (bid >= t.blk0[t.njobs]) { mean_block(m, bid - t.blk0[t.njobs], red); return; }
  int ji = 0;
#pragma unroll
  for (int i = 1; i < MAX_JOBS; ++i)
    if (i < t.njobs && bid >= t.blk0[i]) ji = i;
  if (t.job[ji].pad_) reduce_block_v4<LO>(t.job[ji], bid - t.blk0[ji], red);
  else reduce_block<LO>(t.job[ji], bid - t.blk0[ji], reinterpret_cast<float (*)[64]>(red));
}

// CLV_REDUCE_PAD_LDS (a measurement knob: unused dynamic LDS for a reduction launch without a product, at most 36 KB)
inline int reduce_pad_lds() {
  static const int pad = env_int("CLV_REDUCE_PAD_LDS", 0);
  return pad < 0 ? 0 : (pad > 36864 ? 36864 : pad);
}

// The arguments of clv_splitk_reduce_multi as the launch's tables; *blocks = its grid (0: nothing to do).  CLV_OK / CLV_EINVAL.
inline int reduce_launch_tables(const clv_reduce_job* jobs, int njobs, const float* const* x, const int* n, const int* stride,
                                int n_terms, float* means_out, const clv_skinny_product* riders, int n_riders,
                                ReduceTable& t, MeanTerms& m, SkinnyRider& sr, unsigned* blocks) {
  sr = SkinnyRider{};
  if (n_riders < 0 || n_riders > 2 || (n_riders > 0 && !riders)) return CLV_EINVAL;
  for (int i = 0; i < n_riders; ++i) {
    const clv_skinny_product& r = riders[i];
    if (!r.A || !r.B || !r.C || r.rows < 1 || r.rows + (r.bias_row ? 1 : 0) > SR_ROWS || r.N <= 0 || r.K <= 0 ||
        (i > 0 && r.N != riders[0].N))
      return CLV_EINVAL;
    sr.set[i] = SkinnySet{r.A, r.lda, r.rows, r.bias_row ? 1 : 0, r.B, r.ldb, r.N, r.K, r.C, r.ldc, r.bias_row};
  }
  sr.nsets = n_riders;
  sr.blocks_per_set = n_riders ? (riders[0].N + 63) / 64 : 0;
  if (njobs < 0 || (njobs > 0 && !jobs) || n_terms < 0 || n_terms > 5) return CLV_EINVAL;
  if (n_terms > 0 && (!x || !n || !stride || !means_out)) return CLV_EINVAL;
  m = MeanTerms{};
  m.n_terms = n_terms; m.out = means_out;
  for (int i = 0; i < n_terms; ++i) {
    if (!x[i] || n[i] <= 0) return CLV_EINVAL;
    m.x[i] = x[i]; m.n[i] = n[i]; m.stride[i] = stride[i];
  }
  t.njobs = 0;
  unsigned blk = 0;
  for (int i = 0; i < njobs; ++i) {
    ReduceJob j;
    memcpy(&j, &jobs[i], sizeof(j));
    if (j.splits <= 1 || !j.partial) continue;          // finished inside its GEMM
    if (t.njobs == MAX_JOBS) return CLV_EINVAL;
    j.pad_ = reduce_vec_ok(j) ? 1 : 0;
    t.blk0[t.njobs] = blk;
    t.job[t.njobs++] = j;
    blk += reduce_blocks(j);
  }
  t.blk0[t.njobs] = blk;
  *blocks = (t.njobs == 0 && n_terms == 0 && n_riders == 0) ? 0u : blk + (unsigned)n_terms + (unsigned)(sr.nsets * sr.blocks_per_set);
  return CLV_OK;
}

}  // namespace clv
