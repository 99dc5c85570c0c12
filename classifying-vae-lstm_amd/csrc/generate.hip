// generate.hip -- cl_vrnn autoregressive generation as ONE persistent kernel per batch of sequences (gfx950).
//
// cl_vrnn/model.py:9-60 generates a sequence frame by frame: encoder LSTM step on [x_{t-1}, w], z ~ N(mean,
// exp(log_var)) from the latent head, decoder LSTM step on [x_{t-1}, z, w], x_hat = sigmoid(head), x_t ~
// Bernoulli(x_hat), with teacher forcing over the seed frames.  Every frame depends on the previous sample, so
// per-frame launches (14 kernels, even as one hipGraph replay ~100 us) are pure latency.  Here a workgroup owns a
// sequence for its whole length: both recurrent kernels live in registers (the 4-lane k-slice layout of
// lstm_pair.hip), the encoder's input kernel in LDS (the input frame is a handful of notes: its projection is a
// gather of kernel rows), the decoder's input-kernel rows are prefetched from L2 while the encoder runs, the
// noise comes from Philox in place (same values as clv_philox_normal/uniform give for (seed, frame, stream, index)),
// and a frame is four LDS barriers:
//     encoder cell | latent head + z | decoder cell | output head + Bernoulli sample.
#include "lstm_common.h"
#include "philox.h"

namespace clv {

constexpr int GN_NW = 6;                 // waves per role
constexpr int GN_NT = 2 * GN_NW * 64;    // 768 threads: waves 0-5 encoder + head, waves 6-11 decoder
constexpr int GN_LMAX = 16;              // latent dims carried by the encoder's surplus lane groups (2 per group)
constexpr int GN_LWIDE = 32;             // wide-latent variant: one head column per encoder lane group, one more barrier
constexpr int GN_CMAX = 32;

struct GenArgs {
  int N, S, nsteps, L, C, z_prior, has_xp;
  uint32_t k0, k1;              // Philox key (seed)
  const float* x_seed;          // [N,S,88]
  const float* w;               // [N,C]
  const float* Kx_enc;          // [88,352]  rows of encoder_h/kernel that multiply x_{t-1}
  const float* Kw_enc;          // [C,352]
  const float* b_enc;           // [352]
  const float* U_enc;           // [88,352]
  const float* Wz;              // [88,2L]
  const float* bz;              // [2L]
  const float* Kx_dec;          // [88,352] or unused
  const float* Kz;              // [L,352]
  const float* Kw_dec;          // [C,352]
  const float* b_dec;
  const float* U_dec;
  const float* Wo;              // [88,88]
  const float* bo;              // [88]
  float* Xs;                    // [N,nsteps,88]
  float* xhat;                  // [N,S+nsteps,88] or null
  const uint8_t* clamp;         // [N,nsteps,88] (CL instances): row j constrains Xs[n,j], drawn at step S+j
  float inv_T, Tz;              // TP instances: 1 / temperature of the notes, temperature of the latent noise
  const float* w_dec;           // VR instances: [N,C] the decoder's label (w is then the encoder's)
  const float* x0;              // VR instances: [N,88] the frame before x_seed[:, 0], or null (zeros)
  int hist_source;              // VR instances: the decoder's history is the source frame, not the fed-back sample
  float* zout;                  // ZO instances: [3,N,T,L] = (z_mean, z_log_var, z) of every frame
  const float* z_in;            // ZG instances: [N,T,L] the latent path that replaces the encoder's
  const int32_t* noise_rows;    // ZG instances: [N] the row whose uniforms sequence n draws, or null (n itself)
  uint32_t t0;                  // ST instances: the Philox step of local frame 0 (frames, seed frames and rolls stay local)
  const float* state_in;        // ST instances: [N,5,88] rows h_enc, c_enc, h_dec, c_dec, x (the next input); null: zero start
  float* state_out;             // ST instances: the same rows after the last frame, or null; may alias state_in
};

// slice_matvec with half the live registers: the h slice is consumed in two halves of 12 (the kernel is at its
// 168-register budget; a spill inside the frame loop costs far more than the second LDS wait)
__device__ __forceinline__ void slice_matvec_lr(const float* hslice, const f2 (&Ur)[PKK][2], f2 (&acc2)[2]) {
  const float4* hp = reinterpret_cast<const float4*>(hslice);
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    float hv[12];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const float4 v = hp[3 * half + q];
      hv[4 * q] = v.x; hv[4 * q + 1] = v.y; hv[4 * q + 2] = v.z; hv[4 * q + 3] = v.w;
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < 12; ++j) {
      const int kk = 12 * half + j;
      if (kk < PKK) {
        const f2 hh = {hv[j], hv[j]};
        acc2[0] = __builtin_elementwise_fma(hh, Ur[kk][0], acc2[0]);
        acc2[1] = __builtin_elementwise_fma(hh, Ur[kk][1], acc2[1]);
      }
    }
  }
}

// nonzero inputs of the frame in xbuf as two scalar masks (inputs 0..63 / 64..87), values in (x0, x1)
__device__ __forceinline__ void frame_masks(const float* xbuf, int lane, float& x0, float& x1,
                                            unsigned long long& m0, unsigned long long& m1) {
  x0 = xbuf[lane];
  x1 = lane + 64 < LH ? xbuf[lane + 64] : 0.f;
  m0 = __ballot(x0 != 0.f);
  m1 = __ballot(x1 != 0.f);
}

// ZW = false: latent_dim <= 16, the head rides in the surplus lane groups of the encoder's last wave (4 barriers per
// frame).  ZW = true: latent_dim <= 32, every encoder lane group < 2L owns one head column (22 more registers), the
// head's outputs meet in LDS and L lanes draw z (5 barriers per frame).
// CL = true: clamped ancestral sampling: the note drawn at step t >= S is replaced by clamp[n, t-S, u] where that byte is 0
// or 1 (any other byte leaves the draw); the clamped frame is stored and fed back as the next input.  CL = false folds away.
// TP = true: the tempered model: x_hat = sigmoid(fl(logit * inv_T)), z = m + exp(lv / 2) * fl(Tz * eps); both
// factors are wave-uniform kernel arguments.  The draws themselves (keys, streams, steps, indices) are those of TP = false,
// which folds away.
// VR = true (with CL and TP): re-decoding.  S = 0 and x_seed [N,nsteps,88] holds the SOURCE frames: the
// encoder is teacher-forced with source frame t at every step (its writer lanes request frame t+1 a frame early, as seed
// frames are requested), the decoder's input-kernel prefetch reads a second frame buffer (x0, then the fed-back sample or,
// with hist_source, the encoder's previous input), and the two roles form their gate bias from two labels.  clamp may be
// null (every note free).  VR = false folds away.
// ZO = true (with VR): latents out.  The lanes that form z in phase 2 also store (z_mean, z_log_var, z) of the
// frame to zout, at a 32-bit offset from the sequence's uniform base.  ZO = false folds away.
// ZG = true (with VR): latents in, the decode-only loop.  z_t is z_in[n, t, :], requested a frame early by the
// lanes that would have drawn eps and parked in zbuf as it is; the encoder cell, the latent head, the staging of Kx_enc and
// the encoder's label bias fold away (their pointers are null), and the encoder waves keep phase 4.  x_seed holds the given
// HISTORY frames (with hist_source) or is null (the decoder runs on its own samples).  The uniforms are those of row
// noise_rows[n].  Two barriers per frame are left: decoder cell | output head + sample; the z of frame t+1 is parked behind
// the first of them, after the decoder cell of frame t has read zbuf.  ZG = false folds away.
// ST = true (with CL and TP, not VR): resumable generation.  Both LSTMs start from state_in instead of zero,
// the first input is its row x where there is no seed frame, every Philox step is t0 + t, and after the last frame the
// writer lanes store h (from hb), c and xbuf to state_out.  clamp may be null (every note free).  All of it lies outside the
// frame loop but the step's scalar add.  ST = false folds away.
template <int GATE, bool ZW, bool CL, bool TP, bool VR = false, bool ZO = false, bool ZG = false, bool ST = false>
__global__ __launch_bounds__(GN_NT) void vrnn_generate_kernel(GenArgs a) {
  static_assert((!ZO && !ZG) || (VR && CL && TP && !(ZO && ZG)), "ZO and ZG are variants of the VR instances");
  static_assert(!ST || (CL && TP && !VR), "ST is a variant of the clamped, tempered generate instances");
  constexpr bool NR = VR || ST;          // instances whose roll may be null
  constexpr int GN_LQ = (ZW ? GN_LWIDE : GN_LMAX) / PK;
  extern __shared__ __attribute__((aligned(16))) float Kxl[];            // encoder input kernel [88][352], then Wo [88][88]
  float* Wol = ZG ? Kxl : Kxl + LH * LG;                                 // ZG: no encoder, Wo alone
  __shared__ __attribute__((aligned(16))) float hb[2][2][PK * PKP];       // [chain][parity][sliced h]
  __shared__ __attribute__((aligned(16))) float zbuf[GN_LWIDE];
  __shared__ float zargs_l[2 * GN_LWIDE];
  __shared__ float xbuf[128];
  __shared__ float wbuf[GN_CMAX];
  __shared__ float bo_l[CL ? 128 : 1];          // CL: the output bias, read in phase 4 instead of held in a register
  __shared__ uint8_t cbuf[CL ? 128 : 1];        // CL: the constraint byte of the current step, one per writer lane
  __shared__ float xbuf_d[VR ? 128 : 1];        // VR: the decoder's history frame (xbuf is the encoder's input)
  __shared__ float wbuf_d[VR ? GN_CMAX : 1];    // VR: the decoder's label
  // ST with ZW: the step offset and the state's loads cost the wide instances, which sit at the register budget, one more
  // live value than their parents have room for, so they park the gate bias in LDS (as CL parks the output bias): 3 KB,
  // one more LDS read per role and frame, and fewer spilled registers than the parents (PERFLOG.md)
  constexpr bool RBL = ST && ZW;
  __shared__ float rb_l[RBL ? GN_NT : 1];       // RBL: rb of every lane; a lane reads only its own slot
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool enc = wave < GN_NW;
  const int rw = enc ? wave : wave - GN_NW;
  const int s = lane & 3;
  const int u_raw = rw * 16 + (lane >> 2);
  const int u = min(u_raw, LH - 1);
  const int L = a.L, T = a.S + a.nsteps;
  const int n = blockIdx.x;

  // ---- one-time staging ----------------------------------------------------------------------------------------
  if (!ZG) {
    const int nv = LH * LG / 4;
    const float4* src = reinterpret_cast<const float4*>(a.Kx_enc);
    float4* dst = reinterpret_cast<float4*>(Kxl);
    for (int i0 = tid; i0 < nv; i0 += 4 * GN_NT) {
      float4 v[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = src[min(i0 + q * GN_NT, nv - 1)];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        if (i0 + q * GN_NT < nv) dst[i0 + q * GN_NT] = v[q];
    }
  }
  for (int i = tid; i < LH * LH; i += GN_NT) Wol[i] = a.Wo[i];
  for (int i = tid; i < 2 * 2 * PK * PKP; i += GN_NT) {
    float v = 0.f;
    if (ST && a.state_in) {             // parity 0 of each chain: the h row of its LSTM, unit k at hslot(k)
      const int chain = i / (2 * PK * PKP), slot = i % (PK * PKP), r = slot % PKP, k = PKK * (slot / PKP) + r;
      if (((i / (PK * PKP)) & 1) == 0 && r < PKK) v = a.state_in[((size_t)n * 5 + 2 * chain) * LH + k];
    }
    (&hb[0][0][0])[i] = v;
  }
  if (tid < GN_LWIDE) zbuf[tid] = 0.f;
  if (tid < 128) xbuf[tid] = ((VR || a.S > 0) && (!ZG || a.x_seed) && tid < LH) ? a.x_seed[((size_t)n * (VR ? T : a.S)) * LH + tid] : 0.f;
  if (ST && a.state_in && a.S == 0 && tid < LH) xbuf[tid] = a.state_in[((size_t)n * 5 + 4) * LH + tid];      // this lane wrote the 0
  if (!ZG && tid < a.C) wbuf[tid] = a.w[(size_t)n * a.C + tid];
  if (CL && tid < LH) bo_l[tid] = a.bo[tid];
  if (CL && a.S == 0 && tid < LH)               // step 0's row
    cbuf[tid] = (NR && !a.clamp) ? (uint8_t)255 : a.clamp[(size_t)n * a.nsteps * LH + tid];
  if (VR && tid < 128) xbuf_d[tid] = (a.x0 && tid < LH) ? a.x0[(size_t)n * LH + tid] : 0.f;
  if (VR && tid < a.C) wbuf_d[tid] = a.w_dec[(size_t)n * a.C + tid];
  __syncthreads();

  // recurrent kernel slice of this lane's unit (gate pairs), per-sequence bias W.K_w + b of its gate s
  const float* U = (enc && !ZG) ? a.U_enc : a.U_dec;        // ZG: the encoder waves hold no recurrent kernel of their own
  const int zj = u_raw - LH;                                 // encoder role: surplus group index
  const bool is_zl = !ZW && enc && zj >= 0 && 2 * zj < L;    // group carries latents 2zj, 2zj+1
  const bool is_z = !ZG && is_zl;                            // ... and their head columns
  const int lat = 2 * zj + (s & 1);
  const bool lat_ok = is_zl && lat < L;
  auto zcol = [&](int g) { const int l = 2 * zj + (g & 1); return l < L ? (g >> 1) * L + l : -1; };
  f2 Ur[PKK][2];
#pragma unroll
  for (int kk = 0; kk < PKK; ++kk)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int cix = zcol(g);
      const float* src = is_z ? a.Wz + (size_t)(PKK * s + kk) * 2 * L + max(cix, 0)
                              : U + (size_t)(PKK * s + kk) * LG + g * LH + u;
      const float v = *src;
      Ur[kk][g >> 1][g & 1] = (is_z && cix < 0) ? 0.f : v;
    }
  float rb;
  {
    const float* Kw = (enc && !ZG) ? a.Kw_enc : a.Kw_dec;
    const float* wl = (VR && (ZG || !enc)) ? wbuf_d : wbuf;
    float acc = ((enc && !ZG) ? a.b_enc : a.b_dec)[s * LH + u];
    for (int c0 = 0; c0 < a.C; c0 += 8) {
      float kv[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) kv[q] = Kw[(size_t)min(c0 + q, a.C - 1) * LG + s * LH + u];
#pragma unroll
      for (int q = 0; q < 8; ++q) acc = fmaf(c0 + q < a.C ? wl[c0 + q] : 0.f, kv[q], acc);
    }
    rb = acc;
  }
  if (RBL) rb_l[tid] = rb;
  // encoder role also owns the output head: unit u = note u, 4 k-slices
  float bor = 0.f, bzr = 0.f;
  // role registers (one allocation for both roles: a wave uses only its own view): decoder: z rows of its input
  // kernel, lane s takes latents s, s+4, ... -> RR[4q+g]; encoder, ZW: this lane group's head column -> RR[kk]
  constexpr int GN_RR = ZW ? 32 : 16;
  float RR[GN_RR];
  if (enc && ZG) {
#pragma unroll
    for (int kk = 0; kk < GN_RR; ++kk) RR[kk] = 0.f;
  } else if (enc) {
#pragma unroll
    for (int kk = 0; kk < GN_RR; ++kk) {
      const bool own = ZW && kk < PKK && u_raw < 2 * L;
      const float v = a.Wz[(size_t)(PKK * s + min(kk, PKK - 1)) * 2 * L + min(u_raw, 2 * L - 1)];
      RR[kk] = own ? v : 0.f;
    }
  } else {
#pragma unroll
    for (int q = 0; q < GN_LQ; ++q)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int l = s + PK * q;
        const float v = a.Kz[(size_t)min(l, L - 1) * LG + g * LH + u];
        RR[4 * q + g] = l < L ? v : 0.f;
      }
  }
  if (enc && !ZG) {
    if (!CL) bor = a.bo[u];
    const float bzv = a.bz[max(zcol(s), 0)];
    bzr = lat_ok ? bzv : 0.f;
  }
  const int hslot = PKP * (u / PKK) + (u % PKK);
  const int zpos = lat_ok ? (lat % PK) * GN_LQ + lat / PK : 0;
  float c = 0.f;                       // cell state of this lane's unit (its role's LSTM)
  // every lane, also those whose u_raw >= LH was clamped to unit 87: they run that unit's cell too and publish the same h
  if (ST && a.state_in) c = a.state_in[((size_t)n * 5 + (enc ? 1 : 3)) * LH + u];
  const uint32_t t0 = ST ? a.t0 : 0u;  // the Philox step of local frame 0
  const bool writer = s == 0 && u_raw < LH;        // one lane per unit publishes

  // The noise of a frame does not depend on the data: it is drawn one phase (uniform) / one frame (normal) ahead, in
  // slots where its lanes would otherwise wait at a barrier.
  const bool zdraw = ZW ? (tid < L) : (lat_ok && s < 2);            // lanes that own a latent's eps
  const uint64_t zidx = (uint64_t)n * L + (ZW ? tid : lat);
  // ZO / ZG: this sequence's latents, the lane's latent index clamped so that every lane's address is in bounds
  const uint32_t zl = (uint32_t)min(max(ZW ? tid : lat, 0), L - 1), zlast = (uint32_t)T * (uint32_t)L - 1u;
  float* zo_n = ZO ? a.zout + (size_t)n * T * L : nullptr;
  const size_t zo_plane = ZO ? (size_t)a.N * T * L : 0;
  const float* zi_n = ZG ? a.z_in + (size_t)n * T * L : nullptr;
  const int nrow = (ZG && a.noise_rows) ? a.noise_rows[n] : n;             // the row whose uniforms this sequence draws
  float e_cur;
  if (ZG) {
    e_cur = zi_n[zl];                                                       // z of frame 0, as it is
    if (zdraw) zbuf[ZW ? (tid % PK) * GN_LQ + tid / PK : zpos] = e_cur;
    __syncthreads();
  } else {
    e_cur = zdraw ? philox_normal_at(zidx, a.k0, a.k1, 0u, t0) : 0.f;
    if (TP) e_cur = a.Tz * e_cur;
  }
  const uint32_t crow = CL ? ((uint32_t)n * (uint32_t)a.nsteps - (uint32_t)a.S) * (uint32_t)LH : 0u;   // clamp row of step 0
  float seed_carry = 0.f;                         // CL: the constraint byte requested one frame ago
  const float* src_n = VR ? a.x_seed + (size_t)n * T * LH : nullptr;      // VR: this sequence's source frames
  for (int t = 0; t < T; ++t) {
    const int cur = t & 1;
    float x0, x1;
    unsigned long long m0, m1;
    // xbuf = input frame of step t (seed frame or last sample); VR: the source frame for the encoder, xbuf_d for the decoder
    frame_masks((VR && !enc) ? xbuf_d : xbuf, lane, x0, x1, m0, m1);
    float u_cur = 0.f;
    float seed_next = 0.f;                         // teacher forcing: next seed frame, requested a whole frame early
    // CL: the constraint byte of the NEXT sampled step rides in the same register, which holds no seed frame where
    // t+1 >= S; it is requested a whole frame early like the seed, and parked in LDS at the top of that next frame
    // (this lane alone writes and reads cbuf[u]).  32-bit offset from the roll's base
    if (CL && enc && writer && t >= a.S && t > 0) cbuf[u] = (uint8_t)__builtin_bit_cast(uint32_t, seed_carry);
    if (enc && writer && t + 1 < a.S) seed_next = a.x_seed[((size_t)n * a.S + t + 1) * LH + u];
    if (CL && enc && writer && t + 1 >= a.S && t + 1 < T)
      seed_next = __builtin_bit_cast(float, (NR && !a.clamp) ? 255u
                                                : (uint32_t)a.clamp[crow + (uint32_t)(t + 1) * LH + (uint32_t)u]);
    if (CL) seed_carry = seed_next;
    float src_next = 0.f;                          // VR: source frame t+1, the encoder's next input
    // 32-bit offset from this sequence's (uniform) base: no per-lane address pair to keep across the frame
    if (VR && (!ZG || a.x_seed) && enc && writer && t + 1 < T) src_next = src_n[(uint32_t)(t + 1) * (uint32_t)LH + (uint32_t)u];
    // ---- phase 1: encoder cell (enc waves) | decoder input-kernel rows from L2 (dec waves) ------------------------
    float xd = 0.f;
    if (ZG) e_cur = zi_n[min((uint32_t)(t + 1) * (uint32_t)L + zl, zlast)];   // frame t+1's z: unconditional, index clamped
    if (ZG && enc) {
      // no encoder: nothing to do before the decoder cell
    } else if (enc) {
      float xv = RBL ? rb_l[tid] : rb;
      while (m0) {
        const int k = __builtin_ctzll(m0);
        m0 &= m0 - 1;
        const float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x0), k));
        xv = fmaf(v, Kxl[k * LG + s * LH + u], xv);
      }
      while (m1) {
        const int k = __builtin_ctzll(m1);
        m1 &= m1 - 1;
        const float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x1), k));
        xv = fmaf(v, Kxl[(k + 64) * LG + s * LH + u], xv);
      }
      if (!is_z) {
        f2 acc2[2];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc2[g >> 1][g & 1] = (s == g) ? xv : 0.f;
        slice_matvec_lr(&hb[0][cur][PKP * s], Ur, acc2);
        float z[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) z[g] = reduce_slices<PK>(acc2[g >> 1][g & 1]);
        float h, gg;
        lstm_cell<GATE>(z, c, h, gg);
        hb[0][cur ^ 1][hslot] = h;
      }
    } else if (a.has_xp) {
      // rows of the decoder's input kernel for the notes that are on, 4 loads in flight per round: they travel from
      // L2 while the encoder cell and the latent head run
      const unsigned lane_off = (unsigned)(s * LH + u);
      while (m0 | m1) {
        unsigned ko[4];              // 32-bit offsets from the (uniform) kernel base: one register per pending load
        float vv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bool lo = m0 != 0, any = (m0 | m1) != 0;
          const int bit = lo ? __builtin_ctzll(m0) : (m1 ? __builtin_ctzll(m1) : 0);
          const float v = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, lo ? x0 : x1), bit));
          if (lo) m0 &= m0 - 1; else if (m1) m1 &= m1 - 1;
          ko[q] = (unsigned)(any ? bit + (lo ? 0 : 64) : 0) * LG + lane_off;
          vv[q] = any ? v : 0.f;
        }
        float kv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) kv[q] = a.Kx_dec[ko[q]];
#pragma unroll
        for (int q = 0; q < 4; ++q) xd = fmaf(vv[q], kv[q], xd);
      }
    }
    if (!ZG) step_barrier();
    // ---- phase 2: latent head + z ------------------------------------------------------------------------------------
    if (ZG) {
      // the path is given: zbuf already holds z_t
    } else if (!ZW) {          // surplus lane groups of the encoder's last wave
      if (enc && wave == GN_NW - 1) {
        f2 acc2[2];
#pragma unroll
        for (int g = 0; g < 4; ++g) acc2[g >> 1][g & 1] = (s == g) ? bzr : 0.f;
        slice_matvec_lr(&hb[0][cur ^ 1][PKP * s], Ur, acc2);
        float z[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) z[g] = reduce_slices<PK>(acc2[g >> 1][g & 1]);
        if (lat_ok && s < 2) {
          const float m = a.z_prior ? 0.f : ((s & 1) ? z[1] : z[0]);
          const float lv = a.z_prior ? 0.f : ((s & 1) ? z[3] : z[2]);
          const float zv = fmaf(expf(0.5f * lv), e_cur, m);
          zbuf[zpos] = zv;
          if (ZO) {
            const uint32_t zoff = (uint32_t)t * (uint32_t)L + zl;
            zo_n[zoff] = m;
            zo_n[zo_plane + zoff] = lv;
            zo_n[2 * zo_plane + zoff] = zv;
          }
        }
      }
      step_barrier();
    } else {            // one head column per encoder lane group, then L lanes draw z
      if (enc) {
        const float4* hp = reinterpret_cast<const float4*>(&hb[0][cur ^ 1][PKP * s]);
        float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
        for (int q = 0; q < PKP / 4; ++q) {
          const float4 v = hp[q];
          if (4 * q < PKK) acc0 = fmaf(v.x, RR[min(4 * q, GN_RR - 1)], acc0);
          if (4 * q + 1 < PKK) acc1 = fmaf(v.y, RR[min(4 * q + 1, GN_RR - 1)], acc1);
          if (4 * q + 2 < PKK) acc0 = fmaf(v.z, RR[min(4 * q + 2, GN_RR - 1)], acc0);
          if (4 * q + 3 < PKK) acc1 = fmaf(v.w, RR[min(4 * q + 3, GN_RR - 1)], acc1);
        }
        const float za = reduce_slices<PK>(acc0 + acc1);
        if (s == 0 && u_raw < 2 * L) zargs_l[u_raw] = za + a.bz[u_raw];
      }
      step_barrier();
      if (tid < L) {
        const float m = a.z_prior ? 0.f : zargs_l[tid], lv = a.z_prior ? 0.f : zargs_l[L + tid];
        const float zv = fmaf(expf(0.5f * lv), e_cur, m);
        zbuf[(tid % PK) * GN_LQ + tid / PK] = zv;
        if (ZO) {
          const uint32_t zoff = (uint32_t)t * (uint32_t)L + zl;
          zo_n[zoff] = m;
          zo_n[zo_plane + zoff] = lv;
          zo_n[2 * zo_plane + zoff] = zv;
        }
      }
      step_barrier();
    }
    // ---- phase 3: decoder cell ---------------------------------------------------------------------------------------
    if (!enc) {
      f2 acc2[2];
      const float xv = xd + (RBL ? rb_l[tid] : rb);
#pragma unroll
      for (int g = 0; g < 4; ++g) acc2[g >> 1][g & 1] = (s == g) ? xv : 0.f;
      {
#pragma unroll
        for (int q4 = 0; q4 < GN_LQ / 4; ++q4) {      // 4 latents of this lane per LDS word
          const float4 zq = *reinterpret_cast<const float4*>(&zbuf[GN_LQ * s + 4 * q4]);
          const float zl[4] = {zq.x, zq.y, zq.z, zq.w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int q = 4 * q4 + j;
            const f2 zz = {zl[j], zl[j]};
            const f2 k01 = {RR[4 * q], RR[4 * q + 1]}, k23 = {RR[4 * q + 2], RR[4 * q + 3]};
            acc2[0] = __builtin_elementwise_fma(zz, k01, acc2[0]);
            acc2[1] = __builtin_elementwise_fma(zz, k23, acc2[1]);
          }
        }
      }
      slice_matvec_lr(&hb[1][cur][PKP * s], Ur, acc2);
      float z[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) z[g] = reduce_slices<PK>(acc2[g >> 1][g & 1]);
      float h, gg;
      lstm_cell<GATE>(z, c, h, gg);
      hb[1][cur ^ 1][hslot] = h;
    } else {
      // encoder waves are idle here: draw this frame's Bernoulli uniforms and the next frame's latent noise
      if (writer) u_cur = philox_uniform_at((uint64_t)nrow * LH + u, a.k0, a.k1, 1u, t0 + (uint32_t)t);
      // CL: a clamped note's uniform (drawn and discarded) becomes 2 (forced off: never <= p) or -1 (forced on: always
      // <= p, p in [0, 1]), so phase 4 samples the constraint with no extra work; any other byte leaves the draw
      if (CL && writer && t >= a.S) {
        const uint32_t cb = cbuf[u];
        u_cur = cb == 0u ? 2.f : (cb == 1u ? -1.f : u_cur);
      }
      if (!ZG && zdraw) e_cur = philox_normal_at(zidx, a.k0, a.k1, 0u, t0 + (uint32_t)(t + 1));
      if (!ZG && TP) e_cur = a.Tz * e_cur;
    }
    step_barrier();
    // ---- phase 4: output head, Bernoulli sample, next input frame (enc waves) ------------------------------------
    if (enc) {
      // logit_u = sum_k h_dec[k] Wo[k][u]: this lane's k-slice, Wo rows from LDS (consecutive u: conflict-free)
      const float4* hp = reinterpret_cast<const float4*>(&hb[1][cur ^ 1][PKP * s]);
      const float* wo = Wol + (PKK * s) * LH + u;
      float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
      for (int q = 0; q < PKP / 4; ++q) {
        const float4 v = hp[q];
        if (4 * q < PKK) acc0 = fmaf(v.x, wo[(4 * q) * LH], acc0);
        if (4 * q + 1 < PKK) acc1 = fmaf(v.y, wo[(4 * q + 1) * LH], acc1);
        if (4 * q + 2 < PKK) acc0 = fmaf(v.z, wo[(4 * q + 2) * LH], acc0);
        if (4 * q + 3 < PKK) acc1 = fmaf(v.w, wo[(4 * q + 3) * LH], acc1);
      }
      float acc = acc0 + acc1;
      acc = reduce_slices<PK>(acc);
      if (writer) {
        float lg = acc + (CL ? bo_l[u] : bor);
        if (TP) lg = lg * a.inv_T;
        const float p = sigmoidf_(lg);
        const float xs = u_cur <= p ? 1.f : 0.f;
        if (a.xhat) a.xhat[((size_t)n * T + t) * LH + u] = p;
        if (t >= a.S) a.Xs[((size_t)n * a.nsteps + (t - a.S)) * LH + u] = xs;
        // teacher forcing: the next input is the next seed frame while there is one
        if (VR) {
          xbuf_d[u] = a.hist_source ? xbuf[u] : xs;      // this lane alone writes slot u of both buffers
          xbuf[u] = src_next;
        } else {
          xbuf[u] = (t + 1 < a.S) ? seed_next : xs;
        }
      }
      // ZG: park frame t+1's z; the decoder cell of frame t read zbuf before the barrier above
      if (ZG && zdraw) zbuf[ZW ? (tid % PK) * GN_LQ + tid / PK : zpos] = e_cur;
    }
    step_barrier();
  }
  // ST: the state after frame T-1, behind the loop's last barrier: the cells of frame T-1 wrote parity T & 1
  if (ST && a.state_out && writer) {
    // a writer lane has s = 0, so s * LH + u is its u: the offset the frame loop keeps for its kernel rows anyway, formed
    // again here so that nothing new lives across the loop (the kernel is at its register budget)
    const uint32_t su = (uint32_t)(s * LH + u);            // 32-bit offsets from the sequence's (uniform) base
    float* so = a.state_out + (size_t)n * 5 * LH;
    so[(enc ? 0u : 2u) * LH + su] = hb[enc ? 0 : 1][T & 1][PKP * (su / PKK) + (su % PKK)];
    so[(enc ? 1u : 3u) * LH + su] = c;
    if (enc) so[4u * LH + su] = xbuf[su];
  }
}

}  // namespace clv

extern "C" int clv_vrnn_generate_supported(int D, int H, int L, int C) {
  return D == clv::LH && H == clv::LH && L >= 1 && L <= clv::GN_LWIDE && C >= 1 && C <= clv::GN_CMAX;
}

namespace {
using GenKernel = void (*)(clv::GenArgs);
enum class Mode { generate, vary, decode, resume };   // ancestral sampling | re-decoding | a given latent path
                                                      // | ancestral sampling from and to a state

// a runtime flag as a template argument: f(std::true_type) or f(std::false_type)
template <class F>
GenKernel with_bool(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// The one kernel pick.  Every flag becomes a template argument once: first the mode's own tail of (CL, TP, VR, ZO, ZG) --
// generate takes CL and TP as they come, vary and decode are the clamped, tempered VR instances with ZO or ZG, resume is the
// clamped, tempered ST instance -- then the gate and ZW.  (4 + 2 + 1 + 1) tails x 2 gates x 2 widths = the 32 instances, none
// that the kernel's static_asserts forbid.
template <bool... TAIL>
GenKernel pick_gate_width(bool hard, bool wide) {
  return with_bool(hard, [=](auto HARD) { return with_bool(wide, [](auto ZW) -> GenKernel {
    return clv::vrnn_generate_kernel<decltype(HARD)::value ? CLV_GATE_HARD_SIGMOID : CLV_GATE_SIGMOID, decltype(ZW)::value, TAIL...>; }); });
}

GenKernel pick_vrnn_kernel(Mode mode, bool hard, bool wide, bool clamped, bool tempered, bool latents_out) {
  switch (mode) {
    case Mode::generate:
      return with_bool(tempered, [=](auto TP) { return with_bool(clamped, [=](auto CL) {
        return pick_gate_width<decltype(CL)::value, decltype(TP)::value>(hard, wide); }); });
    case Mode::vary:
      return with_bool(latents_out, [=](auto ZO) { return pick_gate_width<true, true, true, decltype(ZO)::value>(hard, wide); });
    case Mode::resume:
      return pick_gate_width<true, true, false, false, false, true>(hard, wide);
    default:                   // Mode::decode
      return pick_gate_width<true, true, true, false, true>(hard, wide);
  }
}

// The one launcher: every refusal of the three entry points, the kernel pick and the launch.  `a` is the call as its entry
// point filled it (vary and decode: S = 0, nsteps = T; absent inputs null; absent temperatures 1.0f, which is exact).
int vrnn_launch(const clv::GenArgs& a, Mode mode, bool tempered, int D, int H, int gate_act, void* stream) {
  using namespace clv;
  const bool decode = mode == Mode::decode;
  // ---- every mode: shapes, gate, temperatures, the decoder half with the head, the roll's 32-bit addressing
  if (!clv_vrnn_generate_supported(D, H, a.L, a.C) || a.N <= 0 || a.S < 0 || a.nsteps < 0 || a.S + a.nsteps <= 0) return CLV_EINVAL;
  if (gate_act != CLV_GATE_HARD_SIGMOID && gate_act != CLV_GATE_SIGMOID) return CLV_EINVAL;
  if (!temper_factor_ok(a.inv_T, false) || !temper_factor_ok(a.Tz, true)) return CLV_EINVAL;
  if (!a.Kz || !a.Kw_dec || !a.b_dec || !a.U_dec || !a.Wo || !a.bo) return CLV_EINVAL;
  const uint64_t frames = (uint64_t)a.N * a.nsteps;                            // the kernel addresses these in 32 bits:
  if ((a.clamp || decode) && frames * LH > UINT32_MAX) return CLV_EINVAL;      // the roll (decode: and the history frames)
  // ---- the modes with an encoder: its label, its half of the weights, Kx_enc staged to LDS in 16-byte pieces
  if (!decode && (!a.w || !a.Kx_enc || !a.Kw_enc || !a.b_enc || !a.U_enc || !a.Wz || !a.bz || ((uintptr_t)a.Kx_enc) % 16 != 0))
    return CLV_EINVAL;
  // ---- each mode's own inputs
  switch (mode) {
    case Mode::resume:         // the kernel draws step t0 + T one frame ahead: it must not wrap
      if ((uint64_t)a.t0 + (uint64_t)a.S + (uint64_t)a.nsteps > UINT32_MAX) return CLV_EINVAL;
      [[fallthrough]];
    case Mode::generate:       // seed frames only if S > 0, samples only if nsteps > 0; a roll constrains at least one step
      if ((a.S > 0 && !a.x_seed) || (a.nsteps > 0 && !a.Xs) || (a.clamp && a.nsteps <= 0)) return CLV_EINVAL;
      break;
    case Mode::vary:           // x_seed: the source frames, a sequence's addressed in 32 bits, as are the latents out
      if (!a.x_seed || !a.w_dec || !a.Xs) return CLV_EINVAL;
      if ((uint64_t)a.nsteps * LH * sizeof(float) > UINT32_MAX || (a.zout && frames * a.L > UINT32_MAX)) return CLV_EINVAL;
      break;
    case Mode::decode:         // x_seed: the history frames, or null; the latents in are addressed in 32 bits
      if (!a.z_in || !a.w_dec || !a.Xs || frames * a.L > UINT32_MAX) return CLV_EINVAL;
      break;
  }
  GenKernel kern = pick_vrnn_kernel(mode, gate_act == CLV_GATE_HARD_SIGMOID, a.L > GN_LMAX, a.clamp != nullptr, tempered, a.zout != nullptr);
  const size_t lds = (size_t)((decode ? 0 : LH * LG) + LH * LH) * sizeof(float);    // Kx_enc (with an encoder) and Wo
  if (!decode)
    // (the wide ST instances hold 3 KB more static LDS: they ask for what they use, so that the sum stays within 160 KB)
    if (int e = allow_dynamic_lds(reinterpret_cast<const void*>(kern), mode == Mode::resume ? (int)lds : 156 * 1024)) return e;
  const char* label = decode ? "vrnn_decode" : mode == Mode::vary ? (a.zout ? "vrnn_vary_latents" : "vrnn_vary")
                      : mode == Mode::resume ? "vrnn_generate_resume"
                      : tempered ? (a.clamp ? "vrnn_generate_tempered_clamped" : "vrnn_generate_tempered")
                                 : (a.clamp ? "vrnn_generate_clamped" : "vrnn_generate");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(label, s);
  hipLaunchKernelGGL(kern, dim3(a.N), dim3(GN_NT), lds, s, a);
  return launch_status();
}

// what every entry point fills alike; everything else starts absent (null, 0) and untempered
clv::GenArgs vrnn_args(int N, int S, int nsteps, int L, int C, uint64_t seed, const uint8_t* clamp, float* Xs, float* xhat) {
  clv::GenArgs a{};
  a.N = N; a.S = S; a.nsteps = nsteps; a.L = L; a.C = C;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  a.clamp = clamp; a.inv_T = 1.f; a.Tz = 1.f; a.Xs = Xs; a.xhat = xhat;
  return a;
}

void set_encoder(clv::GenArgs& a, const float* Kx_enc, const float* Kw_enc, const float* b_enc, const float* U_enc,
                 const float* Wz, const float* bz) {
  a.Kx_enc = Kx_enc; a.Kw_enc = Kw_enc; a.b_enc = b_enc; a.U_enc = U_enc; a.Wz = Wz; a.bz = bz;
}

void set_decoder(clv::GenArgs& a, const float* Kx_dec, const float* Kz, const float* Kw_dec, const float* b_dec,
                 const float* U_dec, const float* Wo, const float* bo) {
  a.has_xp = Kx_dec != nullptr;
  a.Kx_dec = Kx_dec; a.Kz = Kz; a.Kw_dec = Kw_dec; a.b_dec = b_dec; a.U_dec = U_dec; a.Wo = Wo; a.bo = bo;
}
}  // namespace

// One entry point per operation (include/clvae.h): a call from or to a state runs the ST instance, any other call the CL and TP
// instances that its roll and its `tempered` flag name.
extern "C" int clv_vrnn_generate(int N, int S, int nsteps, int D, int H, int L, int C, int gate_act, int z_prior,
                                 uint64_t seed, const float* x_seed, const float* w,
                                 const float* Kx_enc, const float* Kw_enc, const float* b_enc, const float* U_enc,
                                 const float* Wz, const float* bz,
                                 const float* Kx_dec, const float* Kz, const float* Kw_dec, const float* b_dec,
                                 const float* U_dec, const float* Wo, const float* bo, const uint8_t* clamp,
                                 int tempered, float inv_temperature, float z_temperature, uint32_t t0, const float* state_in,
                                 float* state_out, float* Xs, float* xhat, void* stream) {
  if (!tempered && (inv_temperature != 1.0f || z_temperature != 1.0f)) return CLV_EINVAL;
  const bool state = state_in || state_out || t0 != 0;
  clv::GenArgs a = vrnn_args(N, S, nsteps, L, C, seed, clamp, Xs, xhat);
  set_encoder(a, Kx_enc, Kw_enc, b_enc, U_enc, Wz, bz);
  set_decoder(a, Kx_dec, Kz, Kw_dec, b_dec, U_dec, Wo, bo);
  a.z_prior = z_prior; a.x_seed = x_seed; a.w = w; a.inv_T = inv_temperature; a.Tz = z_temperature;
  a.t0 = t0; a.state_in = state_in; a.state_out = state_out;
  return vrnn_launch(a, state ? Mode::resume : Mode::generate, state || tempered, D, H, gate_act, stream);
}

extern "C" int clv_vrnn_vary(int N, int T, int D, int H, int L, int C, int gate_act, int hist_source, uint64_t seed,
                             const float* sources, const float* x0, const float* w_enc, const float* w_dec,
                             const float* Kx_enc, const float* Kw_enc, const float* b_enc, const float* U_enc,
                             const float* Wz, const float* bz,
                             const float* Kx_dec, const float* Kz, const float* Kw_dec, const float* b_dec,
                             const float* U_dec, const float* Wo, const float* bo, const uint8_t* clamp,
                             float inv_temperature, float z_temperature, float* Xs, float* xhat, float* zout,
                             void* stream) {
  clv::GenArgs a = vrnn_args(N, 0, T, L, C, seed, clamp, Xs, xhat);
  set_encoder(a, Kx_enc, Kw_enc, b_enc, U_enc, Wz, bz);
  set_decoder(a, Kx_dec, Kz, Kw_dec, b_dec, U_dec, Wo, bo);
  a.x_seed = sources; a.x0 = x0; a.w = w_enc; a.w_dec = w_dec; a.hist_source = hist_source != 0;
  a.inv_T = inv_temperature; a.Tz = z_temperature; a.zout = zout;
  return vrnn_launch(a, Mode::vary, true, D, H, gate_act, stream);
}

extern "C" int clv_vrnn_decode(int N, int T, int D, int H, int L, int C, int gate_act, uint64_t seed, const float* z_in,
                               const float* x0, const float* history, const float* w_dec, const int32_t* noise_rows,
                               const float* Kx_dec, const float* Kz, const float* Kw_dec, const float* b_dec,
                               const float* U_dec, const float* Wo, const float* bo, const uint8_t* clamp,
                               float inv_temperature, float* Xs, float* xhat, void* stream) {
  clv::GenArgs a = vrnn_args(N, 0, T, L, C, seed, clamp, Xs, xhat);
  set_decoder(a, Kx_dec, Kz, Kw_dec, b_dec, U_dec, Wo, bo);
  a.x_seed = history; a.hist_source = history != nullptr; a.x0 = x0; a.w_dec = w_dec;
  a.z_in = z_in; a.noise_rows = noise_rows; a.inv_T = inv_temperature;
  return vrnn_launch(a, Mode::decode, true, D, H, gate_act, stream);
}
