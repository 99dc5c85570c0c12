// tail_launch.hip -- the launch that ends the backward pass of the single-GPU step: the hW kernel gradient (outer_bf16.hip) and
// the split-K reduction of every other weight gradient (gemm.hip: clv_splitk_reduce_multi) as two kinds of workgroup in ONE
// launch   (gfx950)
//
// The two are independent (both read what the BPTT kernel left, only the optimizer reads their results) and complementary:
// the reduction waits on memory for most of its wave cycles and issues no MFMA, the product is MFMA + LDS on fewer workgroups
// than the chip has CUs.  On two streams they finish together in the time of the longer one; a captured step replays its
// launches on one queue, so they share the chip only as workgroups of one grid (the way vrnn_front_kernel does it,
// label_head.hip).
//
// Every workgroup of a launch gets the same resources, here the product's: 256 threads and OD_LDS = 48 KB, three workgroups =
// 12 waves per CU where the reduction alone has 20.  Hence
//  * the product runs as 4 waves (64 inputs per workgroup) instead of 6 or 3: a row's sum does not depend on that, and the
//    extra workgroup keeps the batch-row order of the wave count its own launch takes (outer_bf16_body.h: `vw`);
//  * the reduce blocks use the LO form of reduce_body.h: the eight slab loads of a round requested together whatever the
//    slab count, so that 12 waves keep as many bytes in flight as 20 did with the plain form's one-load tail loop;
//  * every role's LDS scratch overlays the one dynamic allocation.
// The product's workgroups go first in the grid: each lives about as long as the whole launch should.
#include "outer_bf16_body.h"
#include "reduce_body.h"

namespace clv {

constexpr int TL_NW = 4;
static_assert(SR_LDS_FLOATS * 4 <= OD_LDS, "the reduce roles' scratch overlays the product's images");

template <bool XU8>
__global__ __launch_bounds__(64 * TL_NW, XU8 ? 4 : 3) void tail_launch_kernel(ReduceTable t, MeanTerms m, SkinnyRider sr, OuterBf16Args a,
                                                                unsigned n_outer, int vw) {
  extern __shared__ __attribute__((aligned(16))) char tl_lds[];
  if (blockIdx.x < n_outer) { dense_outer_block<TL_NW, XU8>(a, tl_lds, (int)blockIdx.x, vw); return; }
  reduce_launch_block<true>(t, m, sr, blockIdx.x - n_outer, reinterpret_cast<float*>(tl_lds));
}

}  // namespace clv

extern "C" int clv_splitk_reduce_multi_outer_supported(int Bn, int nx, int N, int ldx, int ldg) {
  return clv_dense_outer_bf16_supported(Bn, nx, N, ldx, ldg);
}

extern "C" int clv_splitk_reduce_multi_outer(const clv_reduce_job* jobs, int njobs, const float* const* x, const int* n,
                                             const int* stride, int n_terms, float* means_out,
                                             const clv_skinny_product* riders, int n_riders,
                                             int Bn, int nx, int N, const void* X, int x_u8, int ldx, const float* G, int ldg,
                                             float* out, int ldo, float* colsum, const float* Hact, int ldh, const float* hbias,
                                             float* gdot, void* stream) {
  using namespace clv;
  ReduceTable t;
  MeanTerms m;
  SkinnyRider sr;
  unsigned blocks = 0;
  if (int e = reduce_launch_tables(jobs, njobs, x, n, stride, n_terms, means_out, riders, n_riders, t, m, sr, &blocks)) return e;
  const bool product = Bn != 0 || nx != 0 || N != 0 || X || G || out;
  OuterBf16Args a{};
  unsigned n_outer = 0;
  if (product) {       // the argument rules of clv_dense_outer_bf16
    if (!clv_dense_outer_bf16_supported(Bn, nx, N, ldx, ldg) || !X || !G || !out || ldo < N) return CLV_EINVAL;
    if (((uintptr_t)X) % (x_u8 ? 4 : 16) != 0 || ((uintptr_t)G) % 16 != 0) return CLV_EINVAL;
    if (gdot && (!Hact || !hbias || ldh < N || ldh % 2 != 0 || ((uintptr_t)Hact) % 8 != 0)) return CLV_EINVAL;
    a = OuterBf16Args{Bn, nx, N, ldx, ldg, ldo, X, G, out, colsum, Hact, hbias, gdot, ldh};
    n_outer = (unsigned)((nx + 16 * TL_NW - 1) / (16 * TL_NW)) + ((colsum || gdot) ? 1u : 0u);
  }
  if (blocks + n_outer == 0) return CLV_OK;
  hipStream_t s = (hipStream_t)stream;
  // without a product the launch is the LO reduction alone, with the LDS that needs
  const int lds = product ? OD_LDS : SR_LDS_FLOATS * 4 + reduce_pad_lds();
  ProfScope p("tail_launch", s);
  auto go = [&](auto kern) -> int {
    if (int e = allow_dynamic_lds(reinterpret_cast<const void*>(kern), OD_LDS)) return e;
    hipLaunchKernelGGL(kern, dim3(n_outer + blocks), dim3(64 * TL_NW), lds, s, t, m, sr, a, n_outer, od_own_launch_waves(nx));
    return launch_status();
  };
  return x_u8 ? go(tail_launch_kernel<true>) : go(tail_launch_kernel<false>);
}
