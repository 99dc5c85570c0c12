"""numpy reference of clv_gather_rows_multi (include/clvae.h; csrc/pointwise.hip), the mini-batch assembly as a launch of its
own, and the case tables that tests/test_gather_reference.py (no GPU) and tests/test_gpu_gather.py (-m gpu) both walk.

Written from the header's contract, not from the kernel's structure: a copy, so everything is exact.

  rows      output row r takes source row sr = label_reference.stage_rows(rows, idx, row0, cursor)[r] -- the ONE statement of the
            batch cursor (batch j = (step - step0) mod period, the mathematical modulo) that the label stage, the cl_vae fused
            step and the transposing gather are already held to -- then table[sr] where the segment has a table.
  source    the row starts at element sr * stride + offset of the segment's store and is row_elems long.
  output    `pieces` = row_elems / chunk output rows of out_ld elements per batch row (chunk 0: one piece, out_ld = row_elems); a
            piece fills the first `chunk` columns.  A uint8 source widens to float, or stays bytes in a uint8 output.
  buffer    assemble() returns the WHOLE buffer a segment's output lives in: GUARD rows in front, rows * pieces rows, GUARD rows
            behind, every element the launch must not write -- guards and padding columns -- holding `prefill`.
  notes     per list segment, per output row (= frame) the SET of indices of its nonzero bytes; notes_mismatches() reads the
            launch's rows [*, NOTE_ROW]: the indices in any order, each once, then NOTE_NONE to the end of the row.

A case is plain data (case()/seg()); build() makes its stores, row list and tables from a seed taken from the case's name.
"""
import zlib

import numpy as np

from label_reference import stage_rows

GUARD = 2                       # untouched output rows in front of and behind every output
NOTE_ROW, NOTE_NONE = 96, 88    # CLV_NOTE_ROW / CLV_NOTE_NONE (include/clvae.h)
PREFILL_F32 = -4321.0           # float outputs: no source holds it (labels and float frames are drawn from (-4, 4), bytes are >= 0)
PREFILL_U8 = 0xA5               # uint8 outputs and note rows: byte sources hold 0 .. 0xA4 and 0xC8 only
LOUD = 0xC8                     # the "velocity" byte of the non-binary note cases (200)
INT32_MAX = 2 ** 31 - 1


# ---------------------------------------------------------------------------------------------------------- reference --
def source_rows(rows, idx, row0, cursor, table):
    sr = np.asarray(stage_rows(rows, idx, row0, cursor), np.int64)
    return np.asarray(table, np.int64)[sr] if table is not None else sr


def geometry(s):
    """(chunk, pieces, out_ld, stride) of a segment as the entry point resolves its defaults"""
    chunk = s['chunk'] if s['chunk'] > 0 else s['row_elems']
    ld = s['out_ld'] if s['chunk'] > 0 else s['row_elems']
    stride = s['stride'] if s['stride'] > 0 else s['row_elems']
    return chunk, s['row_elems'] // chunk, ld, stride


def assemble(rows, idx, row0, cursor, segs, prefill=None):
    """segs: dicts with store (flat array), out ('f32' | 'u8'), row_elems, chunk, out_ld, stride, offset, table (or None),
    notes (bool).  Returns (outs, notes): outs[k] the whole expected buffer [GUARD + rows * pieces + GUARD, out_ld] of segment k,
    notes[k] None or the list of note sets of its rows * pieces frames.  prefill: None (PREFILL_F32 / PREFILL_U8 by output type)
    or one value for every output."""
    outs, notes = [], []
    for s in segs:
        chunk, pieces, ld, stride = geometry(s)
        sr = source_rows(rows, idx, row0, cursor, s.get('table'))
        src = np.asarray(s['store'])[(sr * stride + s['offset'])[:, None] + np.arange(s['row_elems'])]
        u8 = s['out'] == 'u8'
        fill = prefill if prefill is not None else (PREFILL_U8 if u8 else PREFILL_F32)
        out = np.full((2 * GUARD + rows * pieces, ld), fill, np.uint8 if u8 else np.float32)
        out[GUARD:GUARD + rows * pieces, :chunk] = src.reshape(rows * pieces, chunk)
        outs.append(out)
        notes.append([set(np.flatnonzero(f).tolist()) for f in src.reshape(rows * pieces, chunk)] if s.get('notes') else None)
    return outs, notes


def notes_expected_shape(rows, s):
    return (2 * GUARD + rows * geometry(s)[1], NOTE_ROW)


def notes_mismatches(got, want, fill=PREFILL_U8):
    """got: the whole note buffer [GUARD + frames + GUARD, NOTE_ROW] (uint8), want: the list of note sets.  Messages."""
    got = np.asarray(got)
    bad = []
    n = len(want)
    if got.shape != (2 * GUARD + n, NOTE_ROW):
        return ["note buffer shape %s" % (got.shape,)]
    if not (got[:GUARD] == fill).all() or not (got[GUARD + n:] == fill).all():
        bad.append("note rows outside the batch written")
    for f, w in enumerate(want):
        row = got[GUARD + f]
        k = len(w)
        head = row[:k].tolist()
        if set(head) != w or len(set(head)) != k:
            bad.append("frame %d: notes %s, want %s" % (f, sorted(head), sorted(w)))
        elif not (row[k:] == NOTE_NONE).all():
            bad.append("frame %d: %d notes, then %s" % (f, k, row[k:].tolist()))
        if len(bad) > 8:
            break
    return bad


def mismatches(got_outs, got_notes, want_outs, want_notes):
    """THE comparison of both test files: every output buffer whole (guards and padding included) with array_equal, every note
    buffer with notes_mismatches.  Returns messages; empty = equal."""
    bad = []
    for k, (g, w) in enumerate(zip(got_outs, want_outs)):
        g = np.asarray(g)
        if g.dtype != w.dtype or g.shape != w.shape:
            bad.append("segment %d: %s %s, want %s %s" % (k, g.dtype, g.shape, w.dtype, w.shape))
        elif not np.array_equal(g, w):
            at = np.argwhere(g != w)
            r, c = at[0]
            bad.append("segment %d: %d elements differ, first at buffer row %d col %d: got %r want %r"
                       % (k, len(at), r, c, g[r, c], w[r, c]))
    for k, (g, w) in enumerate(zip(got_notes, want_notes)):
        if w is not None:
            bad += ["segment %d %s" % (k, m) for m in notes_mismatches(g, w)]
    return bad


# --------------------------------------------------------------------------------------------------------- case tables --
def seg(src, out, row_elems, chunk=0, out_ld=0, stride=0, offset=0, table=None, notes=False, src_mis=0, out_mis=0, fill=None):
    """src / out: 'f32' | 'u8'.  table: None, or 'windows' (n starts into the store with repeated and descending entries).
    src_mis / out_mis: the base pointers sit that many ELEMENTS into a larger (256-byte aligned) tensor.  fill: None (random), or
    'notes' (byte frames of `chunk` bytes with 0, 1, 8, 9, chunk notes in turn), 'loud' (the same, every other note LOUD)."""
    return dict(src=src, out=out, row_elems=row_elems, chunk=chunk, out_ld=out_ld, stride=stride, offset=offset, table=table,
                notes=notes, src_mis=src_mis, out_mis=out_mis, fill=fill)


def case(name, rows, segs, idx=False, row0=0, cursor=None, refused=False):
    """cursor: (step, step0, period, stride, offset).  refused: ops raises and nothing is written."""
    return dict(name=name, rows=rows, segs=segs, idx=idx, row0=row0, cursor=cursor, refused=refused)


LABEL = dict(src='f32', out='f32', row_elems=4)


def label():
    return seg('f32', 'f32', 4)


# the six copy forms at `items` work items per row, every condition of their vector predicate met or (the scalar forms) one broken
FORMS = {
    'f32x4': lambda n: seg('f32', 'f32', 4 * n),
    'f32x1': lambda n: seg('f32', 'f32', n, stride=n + 3, offset=1),
    'u8f32x4': lambda n: seg('u8', 'f32', 4 * n),
    'u8f32x1': lambda n: seg('u8', 'f32', n, stride=n + 3, offset=1),
    'u8x4': lambda n: seg('u8', 'u8', 4 * n, stride=4 * n + 4, offset=4),
    'u8x8': lambda n: seg('u8', 'u8', 8 * n),
}


def _boundary_cases():
    """per vector form: the form itself, then every condition of its predicate broken in turn (M = 4, or 8 for the wide byte
    copy whose broken side stays on 4: the narrower form's result; a byte copy off 4 is refused)"""
    out = []
    for name, src, dst, M, off in (('f32x4', 'f32', 'f32', 4, 1), ('u8f32x4', 'u8', 'f32', 4, 1), ('u8x4', 'u8', 'u8', 4, 1),
                                   ('u8x8', 'u8', 'u8', 8, 4)):
        # base: 2 pieces of 3M in rows of 4M, source rows 7M apart starting M in (u8x4, M = 4: 3M and 7M are off 8, so not wide)
        base = dict(row_elems=6 * M, chunk=3 * M, out_ld=4 * M, stride=7 * M, offset=M)
        refused = name == 'u8x4'
        out.append(case('bound-%s-base' % name, 3, [seg(src, dst, **base), label()], idx=True))
        odd = 2 * M + off if M == 8 else 6          # a chunk off its multiple (on 4 for the wide copy), 4 of them to the row
        breaks = dict(row_elems=dict(row_elems=6 * M + off, chunk=0, out_ld=0),      # one piece: chunk = row_elems is off as well
                      chunk=dict(chunk=odd, row_elems=4 * odd),
                      out_ld=dict(out_ld=4 * M + off), stride=dict(stride=7 * M + off), offset=dict(offset=M + off),
                      src_base=dict(src_mis=off), out_base=dict(out_mis=off))
        for what, ch in breaks.items():
            out.append(case('bound-%s-%s' % (name, what), 3, [seg(src, dst, **dict(base, **ch)), label()], idx=True, refused=refused))
    return out


def _length_cases():
    out = []
    for items in (1, 255, 256, 257, 1023, 1024, 1025, 2049):
        for f, mk in FORMS.items():
            out.append(case('len-%s-%d' % (f, items), 2, [mk(items)], row0=1))
    return out


def _segment_cases():
    out = [case('seg-1', 3, [FORMS['u8f32x4'](2049)])]
    for n in (2, 3, 4):
        for k in range(n):          # the long frame segment at position k, 4-float labels everywhere else
            out.append(case('seg-%d-long-at-%d' % (n, k), 2, [FORMS['u8x8'](2049) if q == k else label() for q in range(n)], idx=True))
    for f in ('f32x4', 'f32x1', 'u8f32x4', 'u8f32x1', 'u8x4'):      # the other forms' long rows beside a segment that leaves early
        for k in (0, 1):
            out.append(case('seg-2-long-%s-at-%d' % (f, k), 2, [FORMS[f](2049) if q == k else label() for q in range(2)], row0=2))
    four = [seg('f32', 'f32', 24, 12, 16, 28, 4), seg('u8', 'f32', 10, 5, 7), seg('u8', 'u8', 48, 24, 32, 56, 8), seg('u8', 'u8', 24, 12, 20, 28, 4)]
    for r in range(4):              # four forms in one launch, in every rotation
        out.append(case('seg-4-forms-rot%d' % r, 5, four[r:] + four[:r], idx=True))
    for k in range(4):              # a uint8 source at position k among float segments
        out.append(case('seg-4-u8-at-%d' % k, 4, [seg('u8', 'f32', 12, 4, 8) if q == k else seg('f32', 'f32', 8, 4, 4) for q in range(4)]))
    return out


def _row_cases():
    out = []
    for rows in (1, 2, 65535, 65536, 65537 + 3):
        for use_idx in (False, True):
            out.append(case('rows-f32-%d-%s' % (rows, 'idx' if use_idx else 'seq'), rows, [seg('f32', 'f32', 4)], idx=use_idx, row0=3))
            out.append(case('rows-u8-%d-%s' % (rows, 'idx' if use_idx else 'seq'), rows, [seg('u8', 'u8', 8)], idx=use_idx, row0=3))
    return out


def _piece_cases():
    out = []
    for f, (src, dst) in dict(f32=('f32', 'f32'), u8f32=('u8', 'f32'), u8=('u8', 'u8')).items():
        out.append(case('pieces-%s-chunk0' % f, 3, [seg(src, dst, 24)], idx=True))
        out.append(case('pieces-%s-one-padded' % f, 3, [seg(src, dst, 24, 24, 32)], idx=True))
        out.append(case('pieces-%s-many-tight' % f, 3, [seg(src, dst, 24, 8, 8)], idx=True))
        out.append(case('pieces-%s-many-padded' % f, 3, [seg(src, dst, 24, 8, 12)], idx=True))
    return out


def _window_cases():
    out = []
    for f, (src, dst) in dict(f32=('f32', 'f32'), u8f32=('u8', 'f32'), u8=('u8', 'u8')).items():
        w = dict(row_elems=5 * 8, chunk=8, out_ld=8, stride=8, offset=8, table='windows')      # 5 frames of 8 from frame start + 1
        out.append(case('win-%s-idx' % f, 6, [seg(src, dst, **w), seg(src, dst, **dict(w, offset=0)), label()], idx=True))
        out.append(case('win-%s-row0' % f, 6, [seg(src, dst, **w), label()], row0=4))
        out.append(case('win-%s-stride-below-row' % f, 6, [seg(src, dst, 40, 8, 12, stride=8, offset=16)], row0=2))
    return out


def _cursor_cases():
    out = []
    P = 3
    for d in (0, 1, P - 1, P, 2 * P + 1, -1, -P - 1):
        for use_idx in (False, True):
            out.append(case('cur-d%d-%s' % (d, 'idx' if use_idx else 'seq'), 4, [seg('u8', 'u8', 16, 8, 8), label()], idx=use_idx,
                            row0=0 if use_idx else 2, cursor=(1000 + d, 1000, P, 4, 0)))
    out.append(case('cur-period-1', 4, [seg('f32', 'f32', 8), label()], idx=True, cursor=(17, 5, 1, 4, 0)))
    for use_idx in (False, True):      # a rank's slice of a global batch: rows 4 .. 7 of every 8
        out.append(case('cur-rank-slice-%s' % ('idx' if use_idx else 'seq'), 4, [seg('u8', 'f32', 8), label()], idx=use_idx,
                        cursor=(12, 7, 3, 8, 4)))
    out.append(case('cur-int32-max-ahead', 4, [seg('u8', 'u8', 8), label()], idx=True, cursor=(INT32_MAX, INT32_MAX - 4, 3, 4, 0)))
    out.append(case('cur-int32-max-behind', 4, [seg('u8', 'u8', 8), label()], idx=True, cursor=(INT32_MAX - 4, INT32_MAX, 3, 4, 0)))
    return out


def _note_cases():
    out = []
    n88 = dict(row_elems=3 * 88, chunk=88, out_ld=88, notes=True, fill='notes')
    out.append(case('notes-float-out', 5, [seg('u8', 'f32', **n88), label()], idx=True))
    out.append(case('notes-float-out-padded', 5, [seg('u8', 'f32', **dict(n88, out_ld=96)), label()], idx=True))
    out.append(case('notes-byte-out', 5, [seg('u8', 'u8', **n88), label()], idx=True))
    out.append(case('notes-two-lists', 5, [seg('u8', 'u8', **n88), seg('u8', 'f32', **dict(n88, row_elems=2 * 88)), label()], idx=True))
    out.append(case('notes-list-after-labels', 5, [label(), label(), seg('u8', 'f32', **n88), seg('u8', 'u8', **n88)], idx=True))
    # 128 frames of 8 bytes: 32 list blocks against one copy block; and one frame next to a 2049-item copy: 1 against 3
    out.append(case('notes-list-grid-larger', 2, [seg('u8', 'u8', 128 * 8, 8, 8, notes=True, fill='notes')], row0=1))
    out.append(case('notes-copy-grid-larger', 2, [seg('u8', 'u8', 88, 88, 88, notes=True, fill='notes'), FORMS['u8x8'](2049)], row0=1))
    for ch in (88, 40, 4):
        out.append(case('notes-chunk-%d' % ch, 3, [seg('u8', 'f32', 10 * ch, ch, ch, notes=True, fill='notes')], idx=True))
        out.append(case('notes-loud-chunk-%d' % ch, 3, [seg('u8', 'u8', 10 * ch, ch, ch + 4, notes=True, fill='loud')], idx=True))
    out.append(case('notes-windows-cursor', 4, [seg('u8', 'u8', 3 * 88, 88, 88, 88, 88, 'windows', True, fill='notes'),
                                               seg('u8', 'u8', 3 * 88, 88, 88, 88, 0, 'windows', True, fill='notes'), label()],
                    idx=True, cursor=(9, 11, 3, 4, 0)))
    out.append(case('notes-chunk-92', 3, [seg('u8', 'f32', 2 * 92, 92, 92, notes=True, fill='notes')], refused=True))
    out.append(case('notes-chunk-6', 3, [seg('u8', 'f32', 12, 6, 6, notes=True, fill='notes')], refused=True))
    out.append(case('notes-float-source', 3, [seg('f32', 'f32', 2 * 88, 88, 88, notes=True)], refused=True))
    return out


CASES = (_boundary_cases() + _length_cases() + _segment_cases() + _row_cases() + _piece_cases() + _window_cases() + _cursor_cases()
         + _note_cases())
assert len({c['name'] for c in CASES}) == len(CASES)


def _note_frames(rng, frames, chunk, loud):
    counts = [0, 1, 8, 9, chunk]
    a = np.zeros((frames, chunk), np.uint8)
    for f in range(frames):
        k = min(counts[f % 5], chunk)
        on = rng.permutation(chunk)[:k]
        a[f, on] = 1
        if loud:
            a[f, on[::2]] = LOUD
    return a


def build(c):
    """The data of a case: dict(idx (int64 array or None), n_list, segs: the case's segment dicts + store (flat, unpadded by the
    misalignment), table (int64 array or None)).  Deterministic in the case's name."""
    rng = np.random.default_rng(zlib.crc32(c['name'].encode()))
    rows, cur = c['rows'], c['cursor']
    n_list = rows if cur is None else (cur[2] - 1) * cur[3] + cur[4] + rows     # entries of the row list the cursor can reach
    n_src = n_list + c['row0'] + 5                                             # rows of the data set (or of the window tables)
    # (3 entries more than the cursor reaches: a model that steps back from the list's start must not land on the right batch)
    idx = rng.integers(0, n_src, n_list + 3).astype(np.int64) if c['idx'] else None
    if idx is not None and n_list > 2:
        idx[1] = idx[0]                                                        # a repeated row
    segs = []
    for s in c['segs']:
        s = dict(s)
        chunk, pieces, ld, stride = geometry(s)
        table = None
        n_rows = n_src                  # source rows the store must hold
        if s['table'] == 'windows':
            n_rows = n_src + 9
            table = rng.integers(0, n_rows, n_src).astype(np.int64)
            table[:4] = [n_rows - 1, n_rows - 2, n_rows - 2, 0][:len(table[:4])]     # descending, repeated, the last and first starts
        size = (n_rows - 1) * stride + s['offset'] + s['row_elems']
        if s['src'] == 'f32':
            store = rng.uniform(-4, 4, size).astype(np.float32)
        elif s['fill'] in ('notes', 'loud'):
            frames = -(-size // chunk)
            store = _note_frames(rng, frames, chunk, s['fill'] == 'loud').reshape(-1)[:size].copy()
        else:
            store = rng.integers(0, PREFILL_U8, size).astype(np.uint8)
        s.update(store=store, table=table)
        segs.append(s)
    return dict(idx=idx, n_list=n_list, segs=segs)


def expected(c, data):
    return assemble(c['rows'], data['idx'], c['row0'], c['cursor'], data['segs'])
