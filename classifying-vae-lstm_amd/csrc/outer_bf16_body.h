// outer_bf16_body.h -- the workgroup body of the dense bf16 kernel gradient dK[j,:] = sum_b X[b,j] G[b,:] (outer_bf16.hip has
// the method).  Shared by the product's own launch (outer_bf16.hip) and the launch that ends a backward pass (tail_launch.hip:
// these workgroups in front of the split-K reduction's).
#pragma once
#include "bf16_images.h"

namespace clv {


typedef float od_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned od_u32x4 __attribute__((ext_vector_type(4)));

// waves per workgroup = row tiles of its inputs: 6 (96 inputs), or 3 (48) where 96 would leave half of the CUs without a
// workgroup (configuration 3: 11264 inputs = 118 or 235 workgroups; every workgroup converts all of G, so fewer, larger ones
// are the better deal once the grid is full)
constexpr int OD_KS = 32;                      // batch rows per stage = one MFMA k-step
constexpr int OD_P = 192;                      // image pitch (bytes): 96 columns
constexpr int OD_IMG = OD_KS * OD_P;           // one image of a stage
constexpr int OD_BUF = 4 * OD_IMG;             // X + three pieces of G
constexpr int OD_LDS = 2 * OD_BUF;

struct OuterBf16Args {
  int Bn, nx, N, ldx, ldg, ldo;
  const void* X;       // float, or uint8 (XU8 kernels: ldx counts bytes)
  const float* G;
  float* out;          // [nx, ldo]
  float* colsum;       // [N] or null
  const float* Hact; const float* hbias; float* gdot; int ldh;      // see SparseOuterArgs
};

typedef __amdgpu_buffer_rsrc_t od_rsrc_t;
constexpr unsigned OD_OOB = 0x80000000u;
__device__ __forceinline__ float od_u2f(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ float4 od_load4(od_rsrc_t r, unsigned voff) {
  const od_u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, 0, 0);
  return make_float4(od_u2f(x[0]), od_u2f(x[1]), od_u2f(x[2]), od_u2f(x[3]));
}
// Frames kept as BYTES (round 6: the training step of the large-batch path never widens its piano-roll frames to float): four
// consecutive inputs are one dword; it travels raw in the .x of the register slot a float4 would take and is widened where
// the slot is consumed (every byte value is exactly a bf16 number).
__device__ __forceinline__ float4 od_load_u8x4(od_rsrc_t r, unsigned voff) {
  return make_float4(od_u2f((unsigned)__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, 0, 0)), 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float4 od_widen(const float4& raw) {
  const float r0 = raw.x;                     // (a scalar copy first: bit_cast of a vector ELEMENT reads element 0, tests/test_host_logic.py)
  const unsigned v = __builtin_bit_cast(unsigned, r0);
  return make_float4((float)(v & 0xffu), (float)((v >> 8) & 0xffu), (float)((v >> 16) & 0xffu), (float)(v >> 24));
}

// waves per workgroup of the product's own launch (clv_dense_outer_bf16 has the reasons)
inline int od_own_launch_waves(int nx) { return (nx + 95) / 96 >= 100 ? 6 : 3; }

// One workgroup of the product: row tile `blk` of the inputs, or (blk >= the number of row tiles) the extra workgroup.
// od_lds: OD_LDS bytes, 16-byte aligned.  The workgroup has OD_NW waves; a row of the kernel gradient does not depend on
// OD_NW (a wave owns its 16 inputs and walks the batch in the same stages).  The extra workgroup's sums do depend on how
// many waves share the batch rows, so that count is an argument of its own, `vw`: OD_NW in the product's own launch; in
// the backward pass's last launch (tail_launch.hip: 4 waves) the count the product's own launch would have used, each
// wave then taking the rows of the virtual waves wave, wave + OD_NW, ...  Same rows, same order, same sums.
template <int OD_NW, bool XU8>
__device__ __forceinline__ void dense_outer_block(const OuterBf16Args& a, char* od_lds, int blk, int vw) {
  constexpr int OD_NT = 64 * OD_NW, OD_JT = 16 * OD_NW;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntile = (a.nx + OD_JT - 1) / OD_JT;
  if (blk >= ntile) {
    // ---- the extra workgroup: colsum[c] = sum_b G[b,c], gdot[c] = sum_b (Hact[b,c] - hbias[c]) G[b,c] -------------------
    float2* red = reinterpret_cast<float2*>(od_lds);     // [2][vw][64]
    const int n2 = a.N / 2;
    for (int w = wave; w < vw; w += OD_NW) {
      float2 cs = make_float2(0.f, 0.f), gd = make_float2(0.f, 0.f);
      if (lane < n2) {
        const float2 hb = a.gdot ? make_float2(a.hbias[2 * lane], a.hbias[2 * lane + 1]) : make_float2(0.f, 0.f);
        for (int b0 = w; b0 < a.Bn; b0 += 8 * vw) {
          float2 hv[8], gv[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) {                    // all loads of a round in flight (clamped rows, masked below)
            const int bb = min(b0 + i * vw, a.Bn - 1);
            gv[i] = *reinterpret_cast<const float2*>(a.G + (size_t)bb * a.ldg + 2 * lane);
            hv[i] = a.gdot ? *reinterpret_cast<const float2*>(a.Hact + (size_t)bb * a.ldh + 2 * lane) : make_float2(0.f, 0.f);
          }
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float mk = b0 + i * vw < a.Bn ? 1.f : 0.f;
            cs.x += gv[i].x * mk; cs.y += gv[i].y * mk;
            gd.x = fmaf((hv[i].x - hb.x) * mk, gv[i].x, gd.x);
            gd.y = fmaf((hv[i].y - hb.y) * mk, gv[i].y, gd.y);
          }
        }
      }
      red[w * 64 + lane] = cs;
      red[(vw + w) * 64 + lane] = gd;
    }
    __syncthreads();
    if (wave == 0 && lane < n2) {
      float2 t = make_float2(0.f, 0.f), u = make_float2(0.f, 0.f);
      for (int w = 0; w < vw; ++w) {
        t.x += red[w * 64 + lane].x; t.y += red[w * 64 + lane].y;
        u.x += red[(vw + w) * 64 + lane].x; u.y += red[(vw + w) * 64 + lane].y;
      }
      if (a.colsum) { a.colsum[2 * lane] = t.x; a.colsum[2 * lane + 1] = t.y; }
      if (a.gdot) { a.gdot[2 * lane] = u.x; a.gdot[2 * lane + 1] = u.y; }
    }
    return;
  }

  // the images' padding (columns N..95 of G, inputs beyond nx) is zeroed once and never written
  for (int i = tid; i < OD_LDS / 16; i += OD_NT) reinterpret_cast<float4*>(od_lds)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  const int j0 = blk * OD_JT;
  const int n4 = a.N / 4;
  // which float4s of a stage this thread moves: X 32 rows x 24, G 32 rows x n4; slot e = tid + 384 i.  Rows beyond the
  // batch fall outside the descriptors (the loads return 0), inputs beyond nx and idle slots get an out-of-range offset.
  constexpr unsigned XE = XU8 ? 1u : 4u;                  // bytes per element of X
  const od_rsrc_t r_x = (od_rsrc_t)__builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.X), 0, (int)(unsigned)((size_t)a.Bn * a.ldx * XE), 0x00020000);
  const od_rsrc_t r_g = (od_rsrc_t)__builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.G), 0, (int)(unsigned)((size_t)a.Bn * a.ldg * 4), 0x00020000);
  constexpr int XC4 = OD_JT / 4;                          // float4 columns of the X tile
  constexpr int XS = OD_KS * XC4 / OD_NT, GS = (OD_KS * 24 + OD_NT - 1) / OD_NT;      // float4 slots per thread: 2, and 2 or 4
  static_assert(XS * OD_NT == OD_KS * XC4, "X slots");
  unsigned xg[XS], gg[GS];
  int xl[XS], gl[GS];
  bool gok[GS];
#pragma unroll
  for (int i = 0; i < XS; ++i) {
    const int e = tid + OD_NT * i;
    const int rx = e / XC4, cx = e - XC4 * rx;
    xg[i] = j0 + 4 * cx < a.nx ? XE * (unsigned)(rx * a.ldx + j0 + 4 * cx) : OD_OOB;
    xl[i] = rx * OD_P + 8 * cx;
  }
#pragma unroll
  for (int i = 0; i < GS; ++i) {
    const int e = tid + OD_NT * i;
    gok[i] = e < OD_KS * n4;
    const int eg = gok[i] ? e : 0, rg = eg / n4, cg = eg - n4 * rg;
    gg[i] = gok[i] ? 4u * (unsigned)(rg * a.ldg + 4 * cg) : OD_OOB;
    gl[i] = rg * OD_P + 8 * cg;
  }
  const int nst = (a.Bn + OD_KS - 1) / OD_KS;
  // FOUR stages of operands in flight per thread (register sets 0..3, set = stage % 4): a stage of 18 MFMAs per wave is a
  // fraction of a trip to HBM, with one stage of lookahead every stage waited for memory.  Every request is unconditional -- a stage beyond the batch lies outside the descriptors and costs
  // nothing -- so the compiler's wait counts stay exact: the body below is four stages, straight-line.
  constexpr int DEPTH = 4;
  float4 xr[DEPTH][XS], gr[DEPTH][GS];
  auto load_stage = [&](float4 (&xq)[XS], float4 (&gq)[GS], int s) {
    const unsigned kx = XE * (unsigned)(s * OD_KS * a.ldx), kg = 4u * (unsigned)(s * OD_KS * a.ldg);
#pragma unroll
    for (int i = 0; i < XS; ++i) {
      const unsigned xo = xg[i] == OD_OOB ? OD_OOB : xg[i] + kx;
      xq[i] = XU8 ? od_load_u8x4(r_x, xo) : od_load4(r_x, xo);
    }
#pragma unroll
    for (int i = 0; i < GS; ++i) gq[i] = od_load4(r_g, gg[i] == OD_OOB ? OD_OOB : gg[i] + kg);
  };
  auto store_stage = [&](const float4 (&xq)[XS], const float4 (&gq)[GS], int s) {
    char* buf = od_lds + (s & 1) * OD_BUF;
#pragma unroll
    for (int i = 0; i < XS; ++i) img_put4<1>(buf + xl[i], 0, XU8 ? od_widen(xq[i]) : xq[i]);
#pragma unroll
    for (int i = 0; i < GS; ++i)
      if (gok[i]) img_put4<3>(buf + OD_IMG + gl[i], OD_IMG, gq[i]);
  };
  __syncthreads();                 // the zeroes are in place
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) load_stage(xr[d], gr[d], d);
  store_stage(xr[0], gr[0], 0);
  load_stage(xr[0], gr[0], DEPTH);
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

  od_f32x4 acc[6];
#pragma unroll
  for (int n = 0; n < 6; ++n) acc[n] = od_f32x4{0.f, 0.f, 0.f, 0.f};
  const int fo = img_frag_lane_offset(OD_P, lane);
  // one stage: the products of stage s out of buffer s & 1; stage s + 1 (set K1) into the other buffer (last read in stage
  // s - 1: every wave has passed that stage's barrier); the request for stage s + 1 + DEPTH into the set that just emptied
  auto stage = [&](int s, float4 (&xq)[XS], float4 (&gq)[GS]) {
    const char* buf = od_lds + (s & 1) * OD_BUF;
    const img_bf16x8 ax = img_frag(buf, OD_P, 16 * wave, fo);
#pragma unroll
    for (int n = 0; n < 6; ++n) {
      img_bf16x8 b[3];
#pragma unroll
      for (int p = 0; p < 3; ++p) b[p] = img_frag(buf + (1 + p) * OD_IMG, OD_P, 16 * n, fo);
#pragma unroll
      for (int p = 2; p >= 0; --p) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax, b[p], acc[n], 0, 0, 0);
    }
    store_stage(xq, gq, s + 1);
    load_stage(xq, gq, s + 1 + DEPTH);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");       // (not __syncthreads: the requests stay in flight)
  };
  for (int s = 0; s < nst; s += DEPTH) {         // (stages beyond nst: zero operands, the accumulators do not move)
    stage(s, xr[1], gr[1]);
    stage(s + 1, xr[2], gr[2]);
    stage(s + 2, xr[3], gr[3]);
    stage(s + 3, xr[0], gr[0]);
  }
  // C/D layout: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
  for (int n = 0; n < 6; ++n)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = j0 + 16 * wave + 4 * (lane >> 4) + r, c = 16 * n + (lane & 15);
      if (j < a.nx && c < a.N) a.out[(size_t)j * a.ldo + c] = acc[n][r];
    }
}

}  // namespace clv
