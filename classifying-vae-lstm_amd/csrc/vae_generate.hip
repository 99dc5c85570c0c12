// vae_generate.hip -- cl_vae autoregressive generation as ONE persistent kernel per batch of sequences (gfx950).
//
// cl_vae/model.py:9-42 (generate_sample) produces a sequence frame by frame:
//     z_mean, z_log_var = z_encoder([x_prev, w])          h = relu([x_prev | w] . K_h + b_h); zargs = h . K_z + b_z
//     z ~ N(z_mean, exp(z_log_var))  (or N(0, 1) under use_z_prior)
//     x_hat = decoder([w, z, x_prev_t])                   h_d = relu([w | x_prev_t | z] . K_d + b_d); sigmoid(h_d . K_o + b_o)
//     x_t ~ Bernoulli(x_hat);  x_prev_t := x_prev;  x_prev := x_t          (the decoder's history lags one frame)
// Every frame depends on the previous sample, so the per-frame launches of the layer chain (a hipGraph replay of ~12
// kernels, ~90 us) are pure latency.  Here a workgroup owns a sequence for its whole length: the frame rows of the two
// hidden kernels sit in LDS (a frame is a handful of notes: its product is a gather of kernel rows), the head and output
// kernels in registers as 4-lane k-slices like the LSTM kernels', the label's contribution to both hidden layers is
// formed once, the noise comes from Philox in place (the values clv_philox_normal / _uniform give for (seed, frame,
// stream, index)), and a frame is four LDS barriers:
//     hidden layer of the z-encoder | latent head + z | hidden layer of the decoder | output layer + Bernoulli sample.
#include "lstm_common.h"
#include "philox.h"

namespace clv {

constexpr int VG_NT = 384;               // 96 output slots x 4 k-slices
constexpr int VG_LMAX = 32;              // latent dims
constexpr int VG_CMAX = 32;

struct VaeGenArgs {
  int N, nsteps, L, C, z_prior, has_xp;
  uint32_t k0, k1;              // Philox key (seed)
  const float* x_seed;          // [N,88]
  const float* w;               // [N,C]
  const float* Kh;              // h/kernel [88 + C, 88]: frame rows, then label rows
  const float* bh;              // [88]
  const float* Kz;              // zargs/kernel [88, 2L] = [z_mean | z_log_var]
  const float* bz;              // [2L]
  const float* Kd;              // decoder_h/kernel [C + (88) + L, 88]: label rows, history rows (has_xp), latent rows
  const float* bd;              // [88]
  const float* Ko;              // x_decoded_mean/kernel [88, 88]
  const float* bo;              // [88]
  float* Xs;                    // [N,nsteps,88]
  float* xhat;                  // [N,nsteps,88] or null
  const uint8_t* clamp;         // [N,nsteps,88] (CL instance): row t constrains frame t
  float inv_T, Tz;              // TP instances: 1 / temperature of the notes, temperature of the latent noise
  const float* w_dec;           // VR instance: [N,C] the decoder's label (w is then the z-encoder's)
  const float* x0;              // VR instance: [N,88] the frame before x_seed[:, 0], or null (zeros)
  int hist_source;              // VR instance: the decoder's history is the source frame, not the fed-back sample
  float* zout;                  // ZO instance: [3,N,T,L] = (z_mean, z_log_var, z) of every frame
  const float* z_in;            // ZG instance: [N,T,L] the latent path that replaces the z-encoder's
  const int32_t* noise_rows;    // ZG instance: [N] the row whose uniforms sequence n draws, or null (n itself)
  uint32_t t0;                  // ST instance: the Philox step of local frame 0 (frames and the roll stay local)
  const float* state_in;        // ST instance: [N,2,88] rows x_in (the last frame), hist (the frame before it); replaces x_seed
  float* state_out;             // ST instance: the same rows after the last frame, or null; may alias state_in
};

// sum over the notes that are on (two scalar masks: inputs 0..63 / 64..87) of row n of an LDS-resident [88][88] kernel,
// column j: every lane walks the same notes (scalar loop), all loads are issued before the first add
__device__ __forceinline__ float gather_rows(const float* Kl, int j, unsigned long long m0, unsigned long long m1) {
  float acc0 = 0.f, acc1 = 0.f;
  while (m0) {
    const int n0 = __builtin_ctzll(m0);
    m0 &= m0 - 1;
    float v1 = 0.f;
    if (m0) { const int n1 = __builtin_ctzll(m0); m0 &= m0 - 1; v1 = Kl[n1 * LH + j]; }
    acc0 += Kl[n0 * LH + j];
    acc1 += v1;
  }
  while (m1) {
    const int n0 = 64 + __builtin_ctzll(m1);
    m1 &= m1 - 1;
    acc0 += Kl[n0 * LH + j];
  }
  return acc0 + acc1;
}

// CL = true: clamped ancestral sampling: the note drawn at frame t is replaced by clamp[n, t, o] where that byte is 0 or 1
// (any other byte leaves the draw); the clamped frame is stored and is the next input.  CL = false folds away.
// TP = true: the tempered model: x_hat = sigmoid(fl(logit * inv_T)), z = mean + exp(lv / 2) * fl(Tz * eps), both
// factors wave-uniform kernel arguments; same draws as TP = false, which folds away.
// VR = true (with CL and TP): re-decoding.  x_seed [N,nsteps,88] holds the SOURCE frames: the z-encoder
// reads source frame t (requested a frame early by the writer lanes), the decoder's history is the frame directly before t
// as in training -- x0, then the fed-back sample or, with hist_source, source frame t-1 -- and the two hidden layers take
// their label share from two labels.  clamp may be null (every note free).  VR = false folds away.
// ZO = true (with VR): latents out: the lanes that form z also store (z_mean, z_log_var, z) of the frame to
// zout, at a 32-bit offset from the sequence's uniform base.  ZO = false folds away.
// ZG = true (with VR): latents in, the decode-only loop.  z_t is z_in[n, t, :], requested a frame early and
// parked in zbuf as it is; the z-encoder's hidden layer and the latent head fold away with their weights (null pointers, no
// LDS copy of K_h).  x_seed holds the given HISTORY frames (with hist_source) or is null (the decoder runs on its own
// samples); the uniforms are those of row noise_rows[n].  Two barriers per frame are left: the decoder's hidden layer |
// output layer + sample; the z of frame t+1 is parked behind the first, after the hidden layer of frame t has read zbuf.
// ST = true (with CL and TP, not VR): resumable generation.  The z-encoder's first input and the decoder's
// first history are the two rows of state_in (a fresh start: both the seed frame), every Philox step is t0 + t, and after
// the last frame the writer lanes store the last two frames to state_out.  clamp may be null.  ST = false folds away.
template <bool CL, bool TP, bool VR = false, bool ZO = false, bool ZG = false, bool ST = false>
__global__ __launch_bounds__(VG_NT) void vae_generate_kernel(VaeGenArgs a) {
  static_assert((!ZO && !ZG) || (VR && CL && TP && !(ZO && ZG)), "ZO and ZG are variants of the VR instance");
  static_assert(!ST || (CL && TP && !VR), "ST is a variant of the clamped, tempered generate instance");
  constexpr bool NR = VR || ST;          // instances whose roll may be null
  extern __shared__ __attribute__((aligned(16))) float vg_lds[];
  float* Khl = vg_lds;                        // [88][88] frame rows of the z-encoder's hidden kernel (ZG: absent)
  float* Kdl = ZG ? vg_lds : Khl + LH * LH;   // [88][88] history rows of the decoder's hidden kernel (has_xp)
  float* Kdz = Kdl + LH * LH;                 // [VG_LMAX][88] latent rows of the decoder's hidden kernel
  __shared__ __attribute__((aligned(16))) float hbuf[2][PK * PKP];      // sliced hidden vectors: z-encoder's, decoder's
  __shared__ float zbuf[VG_LMAX];
  __shared__ float xbuf[2][128];              // [parity]: the frame sampled last (0/1 per note)
  __shared__ float wbuf[VG_CMAX];
  __shared__ float xhis[VR ? 128 : 1];        // VR: the decoder's history frame (x0, then the sample of the frame before)
  __shared__ float wbuf_d[VR ? VG_CMAX : 1];  // VR: the decoder's label
  const int tid = threadIdx.x, lane = tid & 63;
  const int s = tid & 3, o_raw = tid >> 2, o = min(o_raw, LH - 1);       // output slot (unit / note) and k-slice
  const int L = a.L, n = blockIdx.x;
  const bool writer = s == 0 && o_raw < LH;
  const int hslot = PKP * (o / PKK) + (o % PKK);
  // ZO / ZG: this sequence's latents, the slot's latent index clamped so that every lane's address is in bounds
  const uint32_t zl = (uint32_t)min(o_raw >> 1, L - 1), zlast = (uint32_t)a.nsteps * (uint32_t)L - 1u;
  float* zo_n = ZO ? a.zout + (size_t)n * a.nsteps * L : nullptr;
  const size_t zo_plane = ZO ? (size_t)a.N * a.nsteps * L : 0;
  const float* zi_n = ZG ? a.z_in + (size_t)n * a.nsteps * L : nullptr;
  const int nrow = (ZG && a.noise_rows) ? a.noise_rows[n] : n;           // the row whose uniforms this sequence draws

  // ---- one-time staging ---------------------------------------------------------------------------------------------
  for (int i = tid; i < LH * LH; i += VG_NT) {
    if (!ZG) Khl[i] = a.Kh[i];
    Kdl[i] = a.has_xp ? a.Kd[(size_t)a.C * LH + i] : 0.f;
  }
  for (int i = tid; i < VG_LMAX * LH; i += VG_NT)
    Kdz[i] = i < L * LH ? a.Kd[(size_t)(a.C + (a.has_xp ? LH : 0)) * LH + i] : 0.f;
  for (int i = tid; i < 2 * PK * PKP; i += VG_NT) (&hbuf[0][0])[i] = 0.f;
  if (tid < VG_LMAX) zbuf[tid] = (ZG && tid < L) ? zi_n[tid] : 0.f;       // ZG: z of frame 0, as it is
  if (tid < 128) {
    if (ST) xbuf[0][tid] = tid < LH ? a.state_in[(size_t)n * 2 * LH + tid] : 0.f;
    else xbuf[0][tid] = (tid < LH && (!ZG || a.x_seed)) ? a.x_seed[(size_t)n * (VR ? a.nsteps : 1) * LH + tid] : 0.f;
    xbuf[1][tid] = xbuf[0][tid];
    if (VR) xhis[tid] = (a.x0 && tid < LH) ? a.x0[(size_t)n * LH + tid] : 0.f;
  }
  if (!ZG && tid < VG_CMAX) wbuf[tid] = tid < a.C ? a.w[(size_t)n * a.C + tid] : 0.f;
  if (VR && tid < VG_CMAX) wbuf_d[tid] = tid < a.C ? a.w_dec[(size_t)n * a.C + tid] : 0.f;
  // head kernel: slot c < 2L owns column c; the pairs (mean_l, log_var_l) sit in neighbouring slots 2l, 2l+1 so that the
  // log-variance reaches the mean's lanes by one DPP row shift (the kernel's own column order is [means | log-variances])
  const int zc = (o_raw & 1) * L + (o_raw >> 1);          // head column of this slot
  const bool zslot = o_raw < 2 * L;
  float Kzr[PKK], Kor[PKK];
#pragma unroll
  for (int kk = 0; kk < PKK; ++kk) {
    Kzr[kk] = (!ZG && zslot) ? a.Kz[(size_t)(PKK * s + kk) * 2 * L + zc] : 0.f;
    Kor[kk] = a.Ko[(size_t)(PKK * s + kk) * LH + o];
  }
  const float bzr = (!ZG && zslot) ? a.bz[zc] : 0.f, bor = a.bo[o];
  __syncthreads();
  // the label's share of both hidden layers (+ bias): constant over the sequence
  float ch = ZG ? 0.f : a.bh[o], cd = a.bd[o];
  for (int c = 0; c < a.C; ++c) {
    if (!ZG) ch = fmaf(wbuf[c], a.Kh[(size_t)(LH + c) * LH + o], ch);
    cd = fmaf((VR ? wbuf_d : wbuf)[c], a.Kd[(size_t)c * LH + o], cd);
  }
  // notes of the current input frame and of the one before it (the decoder's history lags: cl_vae/model.py:38-40)
  unsigned long long cur0, cur1, his0, his1;
  {
    const float x0 = xbuf[0][lane], x1 = lane + 64 < LH ? xbuf[0][lane + 64] : 0.f;
    cur0 = __ballot(x0 != 0.f); cur1 = __ballot(x1 != 0.f);
    his0 = cur0; his1 = cur1;
    if (VR) {
      const float h0 = xhis[lane], h1 = lane + 64 < LH ? xhis[lane + 64] : 0.f;
      his0 = __ballot(h0 != 0.f); his1 = __ballot(h1 != 0.f);
    }
    if (ST) {             // the decoder's first history: the state's second row
      const float* hs = a.state_in + ((size_t)n * 2 + 1) * LH;
      const float h0 = hs[lane], h1 = lane + 64 < LH ? hs[lane + 64] : 0.f;
      his0 = __ballot(h0 != 0.f); his1 = __ballot(h1 != 0.f);
    }
  }
  const uint32_t t0 = ST ? a.t0 : 0u;    // the Philox step of local frame 0

  for (int t = 0; t < a.nsteps; ++t) {
    // this frame's noise, drawn before anything depends on it
    const float u_cur = writer ? philox_uniform_at((uint64_t)nrow * LH + o, a.k0, a.k1, 1u, t0 + (uint32_t)t) : 2.f;
    // this frame's constraint, requested three barriers before phase 4 uses it (2: free)
    const uint32_t cb = (CL && writer && !(NR && !a.clamp)) ? (uint32_t)a.clamp[((size_t)n * a.nsteps + t) * LH + o] : 2u;
    // VR: source frame t+1, the z-encoder's next input, requested a whole frame before it is published
    const float src_next = (VR && (!ZG || a.x_seed) && writer && t + 1 < a.nsteps) ? a.x_seed[((size_t)n * a.nsteps + t + 1) * LH + o] : 0.f;
    const bool zdraw = s == 0 && zslot && !(o_raw & 1);                 // the mean slot of latent l = o_raw / 2
    float eps;
    if (ZG) {
      eps = zi_n[min((uint32_t)(t + 1) * (uint32_t)L + zl, zlast)];      // frame t+1's z: unconditional, index clamped
    } else {
      eps = zdraw ? philox_normal_at((uint64_t)n * L + (o_raw >> 1), a.k0, a.k1, 0u, t0 + (uint32_t)t) : 0.f;
      if (TP) eps = a.Tz * eps;
    }
    // 1. z-encoder hidden layer: relu(x_prev . K_h[frame rows] + (w . K_h[label rows] + b_h))
    if (!ZG) {
      const float h = fmaxf(ch + gather_rows(Khl, o, cur0, cur1), 0.f);
      if (writer) hbuf[0][hslot] = h;
    }
    if (!ZG) step_barrier();
    // 2. latent head + sample
    if (!ZG) {
      float hv[PKP];
      load_hslice(&hbuf[0][PKP * s], hv);
      float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
      for (int kk = 0; kk < PKK; kk += 2) { acc0 = fmaf(hv[kk], Kzr[kk], acc0); acc1 = fmaf(hv[kk + 1], Kzr[kk + 1], acc1); }
      const float za = reduce_slices<PK>(acc0 + acc1) + bzr;          // mean (even slots) / log-variance (odd slots)
      const float lv = dpp_mov<0x104>(za);                             // row_shl:4: the next slot's value
      if (zdraw) {
        const float mean = a.z_prior ? 0.f : za, lvv = a.z_prior ? 0.f : lv;
        const float zv = fmaf(__expf(0.5f * lvv), eps, mean);
        zbuf[o_raw >> 1] = zv;
        if (ZO) {
          const uint32_t zoff = (uint32_t)t * (uint32_t)L + zl;
          zo_n[zoff] = mean;
          zo_n[zo_plane + zoff] = lvv;
          zo_n[2 * zo_plane + zoff] = zv;
        }
      }
    }
    if (!ZG) step_barrier();
    // 3. decoder hidden layer: relu(w . K_d[label rows] + b_d + x_prev_t . K_d[history rows] + z . K_d[latent rows])
    {
      float acc = cd + (a.has_xp ? gather_rows(Kdl, o, his0, his1) : 0.f);
      float zacc = 0.f;
      for (int l = s; l < L; l += PK) zacc = fmaf(zbuf[l], Kdz[l * LH + o], zacc);      // the 4 lanes of a slot share the latents
      acc += reduce_slices<PK>(zacc);
      if (writer) hbuf[1][hslot] = fmaxf(acc, 0.f);
    }
    step_barrier();
    // 4. output layer, Bernoulli sample
    {
      float hv[PKP];
      load_hslice(&hbuf[1][PKP * s], hv);
      float acc0 = 0.f, acc1 = 0.f;
#pragma unroll
      for (int kk = 0; kk < PKK; kk += 2) { acc0 = fmaf(hv[kk], Kor[kk], acc0); acc1 = fmaf(hv[kk + 1], Kor[kk + 1], acc1); }
      float lg = reduce_slices<PK>(acc0 + acc1) + bor;
      if (TP) lg = lg * a.inv_T;
      if (writer) {
        const float p = sigmoidf_(lg);
        float xs = u_cur <= p ? 1.f : 0.f;
        if (CL && cb <= 1u) xs = (float)cb;         // 0: forced off, 1: forced on, else free (the draw stands)
        if (a.xhat) a.xhat[((size_t)n * a.nsteps + t) * LH + o] = p;
        a.Xs[((size_t)n * a.nsteps + t) * LH + o] = xs;
        xbuf[(t + 1) & 1][o] = VR ? src_next : xs;
        if (VR) xhis[o] = xs;               // read after this frame's last barrier, written again three barriers later
      }
      // ZG: park frame t+1's z; the hidden layer of frame t read zbuf before the barrier above
      if (ZG && zdraw) zbuf[o_raw >> 1] = eps;
    }
    step_barrier();
    {
      const float x0 = xbuf[(t + 1) & 1][lane], x1 = lane + 64 < LH ? xbuf[(t + 1) & 1][lane + 64] : 0.f;
      his0 = cur0; his1 = cur1;
      if (VR && !a.hist_source) {
        const float h0 = xhis[lane], h1 = lane + 64 < LH ? xhis[lane + 64] : 0.f;
        his0 = __ballot(h0 != 0.f); his1 = __ballot(h1 != 0.f);
      }
      cur0 = __ballot(x0 != 0.f); cur1 = __ballot(x1 != 0.f);
    }
  }
  // ST: frame nsteps-1 sits in xbuf[nsteps & 1], behind the loop's last barrier; the other parity holds the frame before
  // it (after one frame: the x_in this call started from)
  if (ST && a.state_out && writer) {
    float* so = a.state_out + (size_t)n * 2 * LH;
    so[o] = xbuf[a.nsteps & 1][o];
    so[LH + o] = xbuf[(a.nsteps + 1) & 1][o];
  }
}

}  // namespace clv

extern "C" int clv_vae_generate_supported(int D, int H, int L, int C) {
  return D == clv::LH && H == clv::LH && L >= 1 && L <= clv::VG_LMAX && C >= 1 && C <= clv::VG_CMAX;
}

namespace {
using VaeKernel = void (*)(clv::VaeGenArgs);
enum class Mode { generate, vary, decode, resume };   // ancestral sampling | re-decoding | a given latent path
                                                      // | ancestral sampling from and to a state

// a runtime flag as a template argument: f(std::true_type) or f(std::false_type)
template <class F>
VaeKernel with_bool(bool b, F f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// The one kernel pick.  Every flag becomes a template argument once: generate takes CL and TP as they come, vary and decode
// are the clamped, tempered VR instances with ZO or ZG, resume is the clamped, tempered ST instance: the 4 + 2 + 1 + 1
// instances, none that the kernel's static_asserts forbid.
VaeKernel pick_vae_kernel(Mode mode, bool clamped, bool tempered, bool latents_out) {
  using namespace clv;
  switch (mode) {
    case Mode::generate:
      return with_bool(tempered, [=](auto TP) { return with_bool(clamped, [](auto CL) -> VaeKernel {
        return vae_generate_kernel<decltype(CL)::value, decltype(TP)::value>; }); });
    case Mode::vary:
      return with_bool(latents_out, [](auto ZO) -> VaeKernel { return vae_generate_kernel<true, true, true, decltype(ZO)::value>; });
    case Mode::resume:
      return vae_generate_kernel<true, true, false, false, false, true>;
    default:                   // Mode::decode
      return vae_generate_kernel<true, true, true, false, true>;
  }
}

// The one launcher: every refusal of the three entry points, the kernel pick and the launch.  `a` is the call as its entry
// point filled it (vary and decode: nsteps = T; absent inputs null; absent temperatures 1.0f, which is exact).
int vae_launch(const clv::VaeGenArgs& a, Mode mode, bool tempered, int D, int H, void* stream) {
  using namespace clv;
  const bool decode = mode == Mode::decode;
  // ---- every mode: shapes, temperatures, the decoder half with the output layer, the samples
  if (!clv_vae_generate_supported(D, H, a.L, a.C) || a.N <= 0 || a.nsteps <= 0) return CLV_EINVAL;
  if (!temper_factor_ok(a.inv_T, false) || !temper_factor_ok(a.Tz, true)) return CLV_EINVAL;
  if (!a.Kd || !a.bd || !a.Ko || !a.bo || !a.Xs) return CLV_EINVAL;
  // ---- the modes with a z-encoder: its frames (x_seed: the seed frame or the sources), its label, its half of the weights
  // (resume: the state's two rows stand for the seed frame)
  if (!decode && (!(mode == Mode::resume ? a.state_in : a.x_seed) || !a.w || !a.Kh || !a.bh || !a.Kz || !a.bz)) return CLV_EINVAL;
  // ---- each mode's own inputs; what the kernel addresses in 32 bits
  const uint64_t frames = (uint64_t)a.N * a.nsteps;
  switch (mode) {
    case Mode::generate:       // nothing more (this family sets no bound on the roll)
      break;
    case Mode::resume:         // the last step drawn is t0 + nsteps - 1; the bound is cl_vrnn's, so that the two agree
      if ((uint64_t)a.t0 + (uint64_t)a.nsteps > UINT32_MAX) return CLV_EINVAL;
      break;
    case Mode::vary:           // the latents out
      if (!a.w_dec || (a.zout && frames * a.L > UINT32_MAX)) return CLV_EINVAL;
      break;
    case Mode::decode:         // x_seed: the history frames, or null; the latents in, the roll and the history frames
      if (!a.z_in || !a.w_dec || frames * a.L > UINT32_MAX || frames * LH > UINT32_MAX) return CLV_EINVAL;
      break;
  }
  VaeKernel kern = pick_vae_kernel(mode, a.clamp != nullptr, tempered, a.zout != nullptr);
  const size_t lds = (size_t)((decode ? 1 : 2) * LH * LH + VG_LMAX * LH) * sizeof(float);   // K_h's frame rows go with the z-encoder
  if (!decode)
    if (int e = allow_dynamic_lds(reinterpret_cast<const void*>(kern), 96 * 1024)) return e;
  const char* label = decode ? "vae_decode" : mode == Mode::vary ? (a.zout ? "vae_vary_latents" : "vae_vary")
                      : mode == Mode::resume ? "vae_generate_resume"
                      : tempered ? (a.clamp ? "vae_generate_tempered_clamped" : "vae_generate_tempered")
                                 : (a.clamp ? "vae_generate_clamped" : "vae_generate");
  hipStream_t s = (hipStream_t)stream;
  ProfScope p(label, s);
  hipLaunchKernelGGL(kern, dim3(a.N), dim3(VG_NT), lds, s, a);
  return launch_status();
}

// what every entry point fills alike; everything else starts absent (null, 0) and untempered
clv::VaeGenArgs vae_args(int N, int nsteps, int L, int C, int use_x_prev, uint64_t seed, const uint8_t* clamp, float* Xs, float* xhat) {
  clv::VaeGenArgs a{};
  a.N = N; a.nsteps = nsteps; a.L = L; a.C = C; a.has_xp = use_x_prev != 0;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32);
  a.clamp = clamp; a.inv_T = 1.f; a.Tz = 1.f; a.Xs = Xs; a.xhat = xhat;
  return a;
}

void set_encoder(clv::VaeGenArgs& a, const float* Kh, const float* bh, const float* Kz, const float* bz) { a.Kh = Kh; a.bh = bh; a.Kz = Kz; a.bz = bz; }
void set_decoder(clv::VaeGenArgs& a, const float* Kd, const float* bd, const float* Ko, const float* bo) { a.Kd = Kd; a.bd = bd; a.Ko = Ko; a.bo = bo; }
}  // namespace

// One entry point per operation (include/clvae.h): a call from or to a state runs the ST instance, any other call the CL and TP
// instances that its roll and its `tempered` flag name.
extern "C" int clv_vae_generate(int N, int nsteps, int D, int H, int L, int C, int use_x_prev, int z_prior, uint64_t seed,
                                const float* x_seed, const float* w, const float* Kh, const float* bh, const float* Kz,
                                const float* bz, const float* Kd, const float* bd, const float* Ko, const float* bo,
                                const uint8_t* clamp, int tempered, float inv_temperature, float z_temperature, uint32_t t0,
                                const float* state_in, float* state_out, float* Xs, float* xhat, void* stream) {
  if (!tempered && (inv_temperature != 1.0f || z_temperature != 1.0f)) return CLV_EINVAL;
  const bool state = state_in || state_out || t0 != 0;
  if (state && x_seed) return CLV_EINVAL;    // the state's two rows stand for the seed frame
  clv::VaeGenArgs a = vae_args(N, nsteps, L, C, use_x_prev, seed, clamp, Xs, xhat);
  set_encoder(a, Kh, bh, Kz, bz);
  set_decoder(a, Kd, bd, Ko, bo);
  a.z_prior = z_prior; a.x_seed = x_seed; a.w = w; a.inv_T = inv_temperature; a.Tz = z_temperature;
  a.t0 = t0; a.state_in = state_in; a.state_out = state_out;
  return vae_launch(a, state ? Mode::resume : Mode::generate, state || tempered, D, H, stream);
}

extern "C" int clv_vae_vary(int N, int T, int D, int H, int L, int C, int use_x_prev, int hist_source, uint64_t seed,
                            const float* sources, const float* x0, const float* w_enc, const float* w_dec, const float* Kh,
                            const float* bh, const float* Kz, const float* bz, const float* Kd, const float* bd,
                            const float* Ko, const float* bo, const uint8_t* clamp, float inv_temperature,
                            float z_temperature, float* Xs, float* xhat, float* zout, void* stream) {
  clv::VaeGenArgs a = vae_args(N, T, L, C, use_x_prev, seed, clamp, Xs, xhat);
  set_encoder(a, Kh, bh, Kz, bz);
  set_decoder(a, Kd, bd, Ko, bo);
  a.x_seed = sources; a.x0 = x0; a.w = w_enc; a.w_dec = w_dec; a.hist_source = hist_source != 0;
  a.inv_T = inv_temperature; a.Tz = z_temperature; a.zout = zout;
  return vae_launch(a, Mode::vary, true, D, H, stream);
}

extern "C" int clv_vae_decode(int N, int T, int D, int H, int L, int C, int use_x_prev, uint64_t seed, const float* z_in,
                              const float* x0, const float* history, const float* w_dec, const int32_t* noise_rows,
                              const float* Kd, const float* bd, const float* Ko, const float* bo, const uint8_t* clamp,
                              float inv_temperature, float* Xs, float* xhat, void* stream) {
  clv::VaeGenArgs a = vae_args(N, T, L, C, use_x_prev, seed, clamp, Xs, xhat);
  set_decoder(a, Kd, bd, Ko, bo);
  a.x_seed = history; a.hist_source = history != nullptr; a.x0 = x0; a.w_dec = w_dec;
  a.z_in = z_in; a.noise_rows = noise_rows; a.inv_T = inv_temperature;
  return vae_launch(a, Mode::decode, true, D, H, stream);
}
