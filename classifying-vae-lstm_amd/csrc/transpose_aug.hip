// transpose_aug.hip -- transposition augmentation: the mini-batch assembly of clv_gather_rows_multi with every
// output row's frames shifted by a random number of semitones, drawn by the launch itself (clv_gather_transposed).
//
// One launch, grid = (work items of a row / (256 TG_IPT), rows, segments + note lists) like the plain gather.  A block
// pays the chain of dependent loads once per row -- step counter -> row list -> allowed mask -> window table -- and draws the
// row's shift from it: every block of a row computes the same Philox value (index = the row's GLOBAL number), so all
// segments of a row, its note lists included, move by the same shift without talking to each other.
//
// Frames.  A work item is 8 aligned bytes of the OUTPUT frame (4 where a segment cannot store 8), bytes p .. = source bytes
// p - s .. of the same frame.  They lie in the three (two) aligned dwords of the source frame from q = p - s down to the
// dword boundary; a dword that is not wholly inside the frame [0, D) is not loaded but taken as zero (D is a multiple of 4, so
// an aligned dword is inside or outside as a whole): no byte of the neighbouring frame is ever read, nothing before the
// store's first or behind its last frame is touched, and the bytes shifted in from outside are the zeros the rule asks for.
// Neighbouring dwords are funnel-shifted by the byte offset of q.  No 64-bit division per element, and the 32-bit one is by
// the constant 88 where D is 88.
//
// Labels.  One thread per output class sums the source classes mapped onto it, in ascending order of the source class.
#include "common.h"
#include "philox.h"

namespace clv {

constexpr uint32_t TRANSPOSE_STREAM = 0xFFFFFFF9u;      // TRANSPOSE_STREAM of trainer.py
constexpr int TG_IPT = 4;                               // work items per thread, 256 apart (GATHER_IPT of pointwise.hip)
constexpr int TG_MAX_K = 12;

struct TransSeg { const unsigned char* src; void* out; const int64_t* table; int64_t row_elems, out_ld, stride, offset;
                  int pieces, bytes_out; unsigned char* notes; };
struct TransArgs { TransSeg seg[4]; int nseg, label_seg, nlist, list_seg[4]; int64_t rows; const int64_t* idx; int64_t row0;
                   const int32_t* step_dev; int32_t step0, period; int64_t cur_stride, cur_offset;      // clv_batch_cursor
                   const uint32_t* allowed; const int32_t* class_map; int K, C, D;
                   uint32_t k0, k1, step; const int32_t* draw_step_dev; uint64_t first_row; int32_t* shift_out; };

__device__ __forceinline__ int64_t trans_base(const TransArgs& a) {
  if (!a.step_dev) return 0;
  int j = (*a.step_dev - a.step0) % a.period;
  j = j < 0 ? j + a.period : j;
  return (int64_t)j * a.cur_stride + a.cur_offset;
}

// the shift of output row r whose source row is sr: the k-th set bit of the row's mask, k uniform over its set bits
__device__ __forceinline__ int trans_shift(const TransArgs& a, int64_t r, int64_t sr, uint32_t step) {
  uint32_t m = a.allowed[sr] & ((2u << (2 * a.K)) - 1u);
  const int n = __popc(m);
  if (n == 0) return 0;
  const float u = philox_uniform_at(a.first_row + (uint64_t)r, a.k0, a.k1, TRANSPOSE_STREAM, step);
  int k = (int)(u * (float)n);
  k = k < n - 1 ? k : n - 1;
  for (int i = 0; i < k; ++i) m &= m - 1u;
  return (__ffs(m) - 1) - a.K;
}

// W = 4 or 8 output bytes from p on (p a multiple of W) of a frame moved up by s notes: W / 4 + 1 aligned dwords of the
// source frame, the last one only when the shift is no multiple of 4
template <int W>
__device__ __forceinline__ void shifted_bytes(const unsigned char* frame, int p, int s, int D, unsigned (&v)[W / 4]) {
  const int q = p - s;
  const int at = q & ~3, sh = q & 3;
  unsigned d[W / 4 + 1];
#pragma unroll
  for (int h = 0; h <= W / 4; ++h) {
    const int x = at + 4 * h;
    d[h] = ((h < W / 4 || sh != 0) && x >= 0 && x < D) ? *reinterpret_cast<const unsigned*>(frame + x) : 0u;
  }
#pragma unroll
  for (int h = 0; h < W / 4; ++h) v[h] = (unsigned)(((((unsigned long long)d[h + 1]) << 32) | d[h]) >> (8 * sh));
}

// gather_note_lists of pointwise.hip over the shifted bytes: a wave per frame, lanes 0..D/4-1 take 4 bytes each
__device__ __forceinline__ void trans_note_lists(const TransArgs& a, const TransSeg& sg, int64_t base, uint32_t step) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int piece = blockIdx.x * 4 + wave;
  if (piece >= sg.pieces) return;
  for (int64_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
    const int64_t sr = a.idx ? a.idx[base + r] : a.row0 + base + r;
    const int s = trans_shift(a, r, sr, step);
    const int64_t tr = sg.table ? sg.table[sr] : sr;
    const unsigned char* frame = sg.src + tr * sg.stride + sg.offset + (int64_t)piece * a.D;
    unsigned v4[1] = {0u};
    if (lane < a.D / 4) shifted_bytes<4>(frame, 4 * lane, s, a.D, v4);
    const unsigned v = v4[0];
    unsigned char* out = sg.notes + ((size_t)r * sg.pieces + piece) * CLV_NOTE_ROW;
    int before = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool on = ((v >> (8 * j)) & 255u) != 0u;
      const unsigned long long m = __ballot(on);
      if (on) out[before + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned char)(4 * lane + j);
      before += __popcll(m);
    }
    for (int p = before + lane; p < CLV_NOTE_ROW; p += 64) out[p] = (unsigned char)CLV_NOTE_NONE;
  }
}

// W: bytes of a work item (8 where every frame segment allows 8-byte stores, else 4); DC: the frame size when it is 88, else 0
template <int W, int DC>
__global__ __launch_bounds__(256) void gather_transposed_kernel(TransArgs a) {
  const int64_t base = trans_base(a);
  const uint32_t step = a.draw_step_dev ? (uint32_t)*a.draw_step_dev : a.step;
  if ((int)blockIdx.z >= a.nseg) {            // the z-slices behind the copies build note lists
    const int li = blockIdx.z - a.nseg;
    int k = a.list_seg[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) k = li == q ? a.list_seg[q] : k;
    TransSeg sg = a.seg[0];
#pragma unroll
    for (int q = 1; q < 4; ++q) if (k == q) sg = a.seg[q];
    trans_note_lists(a, sg, base, step);
    return;
  }
  const int si = blockIdx.z;
  TransSeg sg = a.seg[0];
#pragma unroll
  for (int q = 1; q < 4; ++q) if (si == q) sg = a.seg[q];
  if (si == a.label_seg) {                    // labels: w_out[r, t] = sum over the classes c with map[c] == t of w_src[sr, c]
    if (blockIdx.x != 0) return;
    const float* w_src = reinterpret_cast<const float*>(sg.src);
    float* w_out = reinterpret_cast<float*>(sg.out);
    for (int64_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
      const int64_t sr = a.idx ? a.idx[base + r] : a.row0 + base + r;
      const int s = trans_shift(a, r, sr, step);
      if (si == 0 && threadIdx.x == 0 && a.shift_out) a.shift_out[r] = s;
      const int32_t* map = a.class_map + (int64_t)(s + a.K) * a.C;
      for (int t = threadIdx.x; t < a.C; t += 256) {
        float acc = 0.f;
        for (int c = 0; c < a.C; ++c) if (map[c] == t) acc += w_src[sr * a.C + c];
        w_out[r * a.C + t] = acc;
      }
    }
    return;
  }
  const unsigned D = DC ? (unsigned)DC : (unsigned)a.D;      // (DC: the division below is by a constant)
  unsigned cs[TG_IPT], piece[TG_IPT], within[TG_IPT];
#pragma unroll
  for (int k = 0; k < TG_IPT; ++k) {
    cs[k] = ((blockIdx.x * TG_IPT + k) * 256u + threadIdx.x) * (unsigned)W;
    piece[k] = cs[k] / D;
    within[k] = cs[k] - piece[k] * D;
  }
  const bool first = si == 0 && blockIdx.x == 0 && threadIdx.x == 0;      // (its cs[0] is 0: it never leaves here)
  if ((int64_t)cs[0] >= sg.row_elems) return;
  for (int64_t r = blockIdx.y; r < a.rows; r += gridDim.y) {
    const int64_t sr = a.idx ? a.idx[base + r] : a.row0 + base + r;
    const int s = trans_shift(a, r, sr, step);
    if (first && a.shift_out) a.shift_out[r] = s;
    const int64_t tr = sg.table ? sg.table[sr] : sr;
    const unsigned char* row = sg.src + tr * sg.stride + sg.offset;
    unsigned v[TG_IPT][W / 4];
#pragma unroll
    for (int k = 0; k < TG_IPT; ++k) {
#pragma unroll
      for (int h = 0; h < W / 4; ++h) v[k][h] = 0u;
      if ((int64_t)cs[k] < sg.row_elems) shifted_bytes<W>(row + (size_t)piece[k] * D, (int)within[k], s, (int)D, v[k]);
    }
#pragma unroll
    for (int k = 0; k < TG_IPT; ++k) {
      if ((int64_t)cs[k] >= sg.row_elems) continue;
      const int64_t at = (r * sg.pieces + piece[k]) * sg.out_ld + within[k];
      if (sg.bytes_out) {
        unsigned char* dp = reinterpret_cast<unsigned char*>(sg.out) + at;
        if (W == 8) *reinterpret_cast<uint2*>(dp) = make_uint2(v[k][0], v[k][W / 4 - 1]);
        else *reinterpret_cast<unsigned*>(dp) = v[k][0];
      } else {
#pragma unroll
        for (int h = 0; h < W / 4; ++h)
          *reinterpret_cast<float4*>(reinterpret_cast<float*>(sg.out) + at + 4 * h) =
              make_float4((float)(v[k][h] & 255u), (float)((v[k][h] >> 8) & 255u), (float)((v[k][h] >> 16) & 255u),
                          (float)(v[k][h] >> 24));
      }
    }
  }
}

}  // namespace clv

using namespace clv;

extern "C" int clv_gather_transposed(int64_t rows, const int64_t* idx, int64_t row0, int nseg,
                                     const void* const* src, const int32_t* src_u8, void* const* out,
                                     const int64_t* row_elems, const int64_t* chunk, const int64_t* out_ld,
                                     const int64_t* src_stride, const int64_t* src_offset,
                                     const int64_t* const* src_table, unsigned char* const* notes_out,
                                     const clv_batch_cursor* cursor, const clv_transpose_draw* draw, void* stream) {
  if (rows <= 0 || nseg < 1 || nseg > 4 || !src || !src_u8 || !out || !row_elems || !chunk || !out_ld || !draw) return CLV_EINVAL;
  if (cursor && (!cursor->step_dev || cursor->period < 1)) return CLV_EINVAL;
  if (!draw->allowed || !draw->class_map || draw->K < 0 || draw->K > TG_MAX_K) return CLV_EINVAL;
  const int64_t D = draw->D;
  if (D <= 0 || D % 4 || D > 256 || draw->label_seg >= nseg) return CLV_EINVAL;
  TransArgs a;
  memset(&a, 0, sizeof(a));
  a.nseg = nseg; a.rows = rows; a.idx = idx; a.row0 = row0; a.label_seg = draw->label_seg < 0 ? -1 : draw->label_seg;
  if (cursor) { a.step_dev = cursor->step_dev; a.step0 = cursor->step0; a.period = cursor->period;
                a.cur_stride = cursor->stride; a.cur_offset = cursor->offset; }
  a.allowed = draw->allowed; a.class_map = draw->class_map; a.K = draw->K; a.C = draw->C; a.D = (int)D;
  a.k0 = (uint32_t)draw->seed; a.k1 = (uint32_t)(draw->seed >> 32); a.step = draw->step; a.draw_step_dev = draw->step_dev;
  a.first_row = draw->first_row; a.shift_out = draw->shift_out;
  int64_t maxw = 1, maxl = 0;
  bool wide = D % 8 == 0;                      // 8 output bytes per work item where every frame segment can store them
  for (int k = 0; k < nseg; ++k) {
    if (!src[k] || !out[k] || row_elems[k] <= 0 || row_elems[k] >= (1ll << 31)) return CLV_EINVAL;
    if (k == a.label_seg) {                    // float labels [*, C], whole rows; its source row is the row index itself
      if (src_u8[k] != 0 || draw->C < 1 || row_elems[k] != draw->C || (src_table && src_table[k]) ||
          (notes_out && notes_out[k])) return CLV_EINVAL;
      a.seg[k] = TransSeg{(const unsigned char*)src[k], out[k], nullptr, row_elems[k], 0, 0, 0, 1, 0, nullptr};
      continue;
    }
    if (src_u8[k] == 0) return CLV_EINVAL;     // frames are bytes: a float frame source is refused
    const int bytes_out = src_u8[k] == 2;
    if (chunk[k] > 0 && chunk[k] != D) return CLV_EINVAL;
    const int64_t ld = chunk[k] > 0 ? out_ld[k] : D;
    const int64_t stride = (src_stride && src_stride[k] > 0) ? src_stride[k] : row_elems[k];
    const int64_t offset = src_offset ? src_offset[k] : 0;
    if (row_elems[k] % D || ld < D || ld % 4 || stride % 4 || offset % 4 || ((uintptr_t)src[k]) % 4 ||
        ((uintptr_t)out[k]) % (bytes_out ? 4 : 16)) return CLV_EINVAL;
    a.seg[k] = TransSeg{(const unsigned char*)src[k], out[k], src_table ? src_table[k] : nullptr, row_elems[k], ld, stride, offset,
                        (int)(row_elems[k] / D), bytes_out, notes_out ? notes_out[k] : nullptr};
    if (a.seg[k].notes) {      // byte frames of at most 88 notes, read 4 bytes per lane
      if (D > CLV_NOTE_NONE) return CLV_EINVAL;
      a.list_seg[a.nlist++] = k;
      const int64_t wl = (a.seg[k].pieces + 3) / 4 * 256;      // a wave per frame, 4 frames per block
      maxl = wl > maxl ? wl : maxl;
    }
    wide = wide && (bytes_out ? (ld % 8 == 0 && ((uintptr_t)out[k]) % 8 == 0) : true);
    maxw = row_elems[k] > maxw ? row_elems[k] : maxw;
  }
  maxw = (maxw + (wide ? 7 : 3)) / (wide ? 8 : 4);
  hipStream_t s = (hipStream_t)stream;
  ProfScope p("gather_transposed", s);
  const int64_t gx_copy = (maxw + 256 * TG_IPT - 1) / (256 * TG_IPT), gx_list = (maxl + 255) / 256;
  const dim3 grid((unsigned)(gx_copy > gx_list ? gx_copy : gx_list), (unsigned)(rows < 65535 ? rows : 65535), nseg + a.nlist);
  auto kernel = D == 88 ? (wide ? gather_transposed_kernel<8, 88> : gather_transposed_kernel<4, 88>)
                        : (wide ? gather_transposed_kernel<8, 0> : gather_transposed_kernel<4, 0>);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, a);
  return launch_status();
}
