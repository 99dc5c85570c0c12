"""numpy reference of clv_gather_transposed (csrc/transpose_aug.hip): the mini-batch assembly with a random
transposition per output row.  TEST ORACLE: written from the rule in include/clvae.h, independent of clvae_amd.augment.

Everything is exact (bytes, 0 / 1 floats, integers; the label sums are fp32 adds in ascending order of the source class), so
the GPU tests compare bit for bit.  The uniforms come from oracle/philox.py.
"""
import numpy as np

from oracle import philox as OP

TRANSPOSE_STREAM = 0xFFFFFFF9
NOTE_ROW, NOTE_NONE = 96, 88


def kth_set_bit(m, k):
    """position of the k-th set bit of m (k = 0: the lowest), counted from bit 0"""
    seen = -1
    for j in range(32):
        if (int(m) >> j) & 1:
            seen += 1
            if seen == k:
                return j
    raise ValueError("mask %#x has no set bit number %d" % (int(m), k))


def pick(m, K, u):
    """the shift of a row with mask m and uniform u (float32)"""
    m = int(m) & ((1 << (2 * K + 1)) - 1)
    n = bin(m).count('1')
    if n == 0:
        return 0
    k = min(int(np.float32(u) * np.float32(n)), n - 1)
    return kth_set_bit(m, k) - K


def draw_shifts(masks, K, seed, step, first_row=0):
    """masks: the allowed word of every OUTPUT row (already looked up by its source row); int32 [rows]"""
    masks = np.asarray(masks)
    u = OP.uniform(len(masks), seed, step=step, stream_id=TRANSPOSE_STREAM, first_index=first_row)
    return np.array([pick(m, K, x) for m, x in zip(masks, u)], np.int32)


def shift_frame(frame, s):
    """out[p] = in[p - s] where 0 <= p - s < D, else 0"""
    D = frame.shape[0]
    out = np.zeros_like(frame)
    if s >= 0:
        out[s:] = frame[:D - s]
    else:
        out[:D + s] = frame[-s:]
    return out


def cursor_base(step_value, cursor):
    """cursor = (step0, period, stride, offset) or None"""
    if cursor is None:
        return 0
    step0, period, stride, offset = cursor
    return ((int(step_value) - step0) % period) * stride + offset


def source_rows(rows, idx, row0, base):
    return np.array([int(idx[base + r]) if idx is not None else row0 + base + r for r in range(rows)], np.int64)


def gather_transposed(rows, idx, row0, base, segs, w_src, allowed, class_map, K, seed, step, first_row=0, D=88):
    """segs: a list of (store, row_elems, stride, offset, table) -- store a flat uint8 array, a source row starts at byte
    (table[sr] if table is not None else sr) * stride + offset and is row_elems / D frames of D bytes.  w_src: float32
    [n, C] or None.  Returns (frames per segment: uint8 [rows, pieces, D]; w_out float32 [rows, C] or None; shifts int32 [rows])."""
    sr = source_rows(rows, idx, row0, base)
    shifts = draw_shifts(np.asarray(allowed)[sr], K, seed, step, first_row)
    outs = []
    for store, row_elems, stride, offset, table in segs:
        store = np.asarray(store, np.uint8).reshape(-1)
        pieces = row_elems // D
        out = np.zeros((rows, pieces, D), np.uint8)
        for r in range(rows):
            at = (int(table[sr[r]]) if table is not None else int(sr[r])) * stride + offset
            for p in range(pieces):
                out[r, p] = shift_frame(store[at + p * D: at + (p + 1) * D], int(shifts[r]))
        outs.append(out)
    w_out = None
    if w_src is not None:
        w_src = np.asarray(w_src, np.float32)
        C = w_src.shape[1]
        cmap = np.asarray(class_map).reshape(2 * K + 1, C)
        w_out = np.zeros((rows, C), np.float32)
        for r in range(rows):
            for c in range(C):
                t = int(cmap[int(shifts[r]) + K, c])
                if t >= 0:
                    w_out[r, t] = np.float32(w_out[r, t] + w_src[sr[r], c])
    return outs, w_out, shifts


def note_sets(frames):
    """[rows, pieces, D] -> a list per (row, piece) of the set of sounding notes"""
    f = np.asarray(frames)
    return [[set(np.nonzero(f[r, p])[0].tolist()) for p in range(f.shape[1])] for r in range(f.shape[0])]


def check_note_rows(notes, frames):
    """notes: uint8 [rows * pieces, NOTE_ROW] as the launch wrote them; frames: the reference's [rows, pieces, D].  Every row
    holds its frame's notes once each (any order), then NOTE_NONE up to the end."""
    want = note_sets(frames)
    notes = np.asarray(notes).reshape(len(want), len(want[0]), NOTE_ROW)
    for r, row in enumerate(want):
        for p, s in enumerate(row):
            got = notes[r, p]
            n = len(s)
            assert set(got[:n].tolist()) == s and len(set(got[:n].tolist())) == n, (r, p, got[:n], sorted(s))
            assert (got[n:] == NOTE_NONE).all(), (r, p, got[n:])
