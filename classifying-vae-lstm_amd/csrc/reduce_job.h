// reduce_job.h -- a pending slab reduction: the struct behind clv_reduce_job, and the one place that builds a producer's
// job and decides whether it runs now or waits in the caller's queue (every file with a `clv_reduce_job* job` includes it)
#pragma once
#include <initializer_list>

#include "common.h"

namespace clv {

constexpr int MAX_PROB = 4;

// One pending split-K reduction: everything the epilogue needs, small enough that a table of them
// travels as kernel arguments (clv_reduce_job in the C ABI is this struct, opaque).
struct ReduceProb { float* C; int ldc; int row0; };
struct ReduceJob {
  const float* partial;    // [splits][M][N] raw partial sums
  int M, N, splits, nprob;
  float alpha, beta;
  const float* bias;
  const float* aux;
  int act;
  int pad_;                // set by the reduce launchers: 1 = 4 outputs per thread (16-byte slab loads)
  ReduceProb prob[MAX_PROB];   // nprob == 0: prob[0] is the single output
};
static_assert(sizeof(ReduceJob) <= sizeof(clv_reduce_job), "clv_reduce_job too small");

int launch_reduce(const ReduceJob& j, hipStream_t s);     // gemm.hip: one reduction, now

// Entry points clear their job first thing, before any argument check: whatever they return, *job is either a pending
// reduction or all zero (the multi-reduce skips zero jobs).
inline void clear_job(clv_reduce_job* job) { if (job) memset(job, 0, sizeof(*job)); }

// The job of a slab producer: C_p = beta * C_p + sum over `splits` slabs [M][N] of the rows from row0_p on, no epilogue.
inline ReduceJob slab_job(const void* partial, int M, int N, int splits, float beta, std::initializer_list<ReduceProb> outs) {
  ReduceJob j;
  memset(&j, 0, sizeof(j));
  j.partial = (const float*)partial; j.M = M; j.N = N; j.splits = splits;
  j.alpha = 1.f; j.beta = beta; j.act = CLV_ACT_NONE;
  for (const ReduceProb& o : outs) j.prob[j.nprob++] = o;      // (callers pass at most MAX_PROB)
  return j;
}
// ... of a layer's kernel [bias_row, N] and, in slab row bias_row, its bias [N]
inline ReduceJob kernel_bias_job(const void* partial, int M, int N, int splits, float* dK, float* db, int bias_row) {
  return slab_job(partial, M, N, splits, 0.f, {{dK, N, 0}, {db, N, bias_row}});
}

// The fate of a job, and the only place that writes a caller's clv_reduce_job after a launch: more than one slab and a
// queue to wait in -> pending; else reduced now (one slab still goes through the reduction: it scatters the rows).
inline int finish_or_defer(const ReduceJob& j, int splits, clv_reduce_job* job, hipStream_t s) {
  if (job && splits > 1) {
    memcpy(job, &j, sizeof(j));      // the caller reduces later (clv_splitk_reduce_multi)
    return CLV_OK;
  }
  clear_job(job);
  return launch_reduce(j, s);
}

}  // namespace clv
