"""No GPU: tests/gather_reference.py, the reference that tests/test_gpu_gather.py holds clv_gather_rows_multi to.

1. assemble() against expectations written out by hand on three tiny cases.
2. A second model of the launch, written the way the kernel works (work items, pieces, a row loop, per-segment geometry) and
   sharing nothing with assemble() but the data: unmutated it gives assemble()'s buffers on every case of the table; with each
   of seven deliberate defects, gather_reference.mismatches -- the comparison the GPU test uses -- must reject it on at least
   one case.  A defect that survives means the case table could not see the same defect in the kernel.
"""
import math

import numpy as np
import pytest

import gather_reference as GR

G, PF, PU = GR.GUARD, GR.PREFILL_F32, GR.PREFILL_U8


def S(store, out, row_elems, chunk=0, out_ld=0, stride=0, offset=0, table=None, notes=False):
    return dict(store=np.asarray(store), out=out, row_elems=row_elems, chunk=chunk, out_ld=out_ld, stride=stride, offset=offset,
                table=table, notes=notes)


# ------------------------------------------------------------------------------------------------- 1. by hand --
def test_chunked_row_with_padding_by_hand():
    outs, notes = GR.assemble(2, None, 0, None, [S(np.arange(12, dtype=np.float32), 'f32', 6, 3, 4)])
    want = np.array([[PF] * 4] * G + [[0, 1, 2, PF], [3, 4, 5, PF], [6, 7, 8, PF], [9, 10, 11, PF]] + [[PF] * 4] * G, np.float32)
    assert outs[0].dtype == np.float32 and np.array_equal(outs[0], want) and notes == [None]


def test_window_table_with_a_repeated_start_by_hand():
    # frames of 2 bytes; a window = 2 frames from one frame behind its start; starts 3, 0, 0 taken in the order 1, 2, 0
    store = np.arange(12, dtype=np.uint8)
    store[4] = 0
    outs, notes = GR.assemble(3, np.array([1, 2, 0]), 99, None, [S(store, 'u8', 4, 2, 2, 2, 2, np.array([3, 0, 0]), True)])
    want = np.array([[PU, PU]] * G + [[2, 3], [0, 5], [2, 3], [0, 5], [8, 9], [10, 11]] + [[PU, PU]] * G, np.uint8)
    assert outs[0].dtype == np.uint8 and np.array_equal(outs[0], want)
    assert notes[0] == [{0, 1}, {1}, {0, 1}, {1}, {0, 1}, {0, 1}]
    widened, _ = GR.assemble(3, np.array([1, 2, 0]), 99, None, [S(store, 'f32', 4, 2, 2, 2, 2, np.array([3, 0, 0]))])
    assert widened[0].dtype == np.float32 and np.array_equal(widened[0][G:-G], want[G:-G].astype(np.float32))


def test_cursor_behind_its_first_step_by_hand():
    # step 3, first bound step 5, 4 batches per epoch: batch (3 - 5) mod 4 = 2; 2 rows a rank out of 2 * 2 + 1 onward
    idx = np.arange(10)[::-1].copy()
    outs, _ = GR.assemble(2, idx, 0, (3, 5, 4, 2, 1), [S(np.arange(20, dtype=np.float32), 'f32', 2)])
    assert np.array_equal(outs[0][G:-G], np.array([[8, 9], [6, 7]], np.float32))      # idx[5], idx[6] = 4, 3
    outs, _ = GR.assemble(2, None, 1, (3, 5, 4, 2, 1), [S(np.arange(20, dtype=np.float32), 'f32', 2)])
    assert np.array_equal(outs[0][G:-G], np.array([[12, 13], [14, 15]], np.float32))  # rows 1 + 5, 1 + 6


# ------------------------------------------------------------------------------------------- 2. the kernel's way --
MUTANTS = ('cursor-no-fixup', 'ld-is-chunk', 'piece-within-swapped', 'last-partial-items-dropped', 'rows-from-65535-unwritten',
           'segment-3-with-geometry-of-0', 'table-before-idx')


def item_width(s):
    """elements per work item: 8 (byte copy, everything on 8), 4 (everything on 4 and the bases on their alignment) or 1"""
    chunk, pieces, ld, stride = GR.geometry(s)
    isz, osz = (1 if s['src'] == 'u8' else 4), (1 if s['out'] == 'u8' else 4)

    def on(M, sal, oal):
        return all(v % M == 0 for v in (s['row_elems'], chunk, ld, stride, s['offset'])) and \
            (s['src_mis'] * isz) % sal == 0 and (s['out_mis'] * osz) % oal == 0
    if s['src'] == 'u8' and s['out'] == 'u8' and on(8, 8, 8):
        return 8
    if s['src'] == 'u8':
        return 4 if on(4, 4, 4 if s['out'] == 'u8' else 16) else 1
    return 4 if on(4, 16, 16) else 1


def take(a, i):
    return np.take(np.asarray(a), i, mode='wrap')      # a defect may index outside: any element will do, as on the device


def launch_model(c, data, mutant=None):
    rows, idx, row0, segs = c['rows'], data['idx'], c['row0'], data['segs']
    base = 0
    if c['cursor'] is not None:
        step, step0, period, cstride, coff = c['cursor']
        j = int(math.fmod(step - step0, period))           # C's remainder: the sign of the dividend
        if j < 0 and mutant != 'cursor-no-fixup':
            j += period
        base = j * cstride + coff
    r = np.arange(rows)
    outs, notes = [], []
    for k, s in enumerate(segs):
        g = segs[0] if (mutant == 'segment-3-with-geometry-of-0' and k == 3) else s
        chunk, pieces, ld, stride = GR.geometry(g)
        own_chunk, own_pieces, own_ld, _ = GR.geometry(s)
        if mutant == 'ld-is-chunk':
            ld = chunk
        table = g['table']
        if mutant == 'table-before-idx' and table is not None and idx is not None:
            sr = take(idx, take(table, base + r))
        else:
            sr = take(idx, base + r) if idx is not None else row0 + base + r
            sr = take(table, sr) if table is not None else sr
        cc = np.arange(g['row_elems'])
        if mutant == 'last-partial-items-dropped':
            W = item_width(s)
            n = g['row_elems'] // W
            cc = cc[cc // W < (n // 256) * 256] if n % 256 else cc
        piece, within = (cc % chunk, cc // chunk) if mutant == 'piece-within-swapped' else (cc // chunk, cc % chunk)
        u8 = s['out'] == 'u8'
        flat = np.full((2 * G + rows * own_pieces) * own_ld, PU if u8 else PF, np.uint8 if u8 else np.float32)
        rr = r[r < 65535] if mutant == 'rows-from-65535-unwritten' else r
        pos = G * own_ld + (rr[:, None] * pieces + piece[None, :]) * ld + within[None, :]
        val = take(s['store'], sr[rr][:, None] * stride + g['offset'] + cc[None, :]).astype(flat.dtype)
        keep = (pos >= 0) & (pos < flat.size)
        flat[pos[keep]] = val[keep]
        outs.append(flat.reshape(-1, own_ld))
        if s['notes']:
            frames = take(s['store'], (sr[:, None] * stride + g['offset'] + np.arange(g['row_elems'])[None, :]))
            sets = [set(np.flatnonzero(f).tolist()) for f in frames.reshape(-1, chunk)][:rows * own_pieces]
            buf = np.full(GR.notes_expected_shape(rows, s), PU, np.uint8)
            for f, w in enumerate(sets):
                buf[G + f] = GR.NOTE_NONE
                buf[G + f, :len(w)] = sorted(w, reverse=True)      # any order will do
            notes.append(buf)
        else:
            notes.append(None)
    return outs, notes


LIVE = [c for c in GR.CASES if not c['refused']]
_DATA = {}


def data_of(c):
    if c['name'] not in _DATA:
        d = GR.build(c)
        _DATA[c['name']] = (d, GR.expected(c, d))
    return _DATA[c['name']]


def test_case_table_covers_what_it_claims():
    names = [c['name'] for c in GR.CASES]
    assert len(names) == len(set(names))
    assert sorted({c['rows'] for c in GR.CASES if c['name'].startswith('rows-')}) == [1, 2, 65535, 65536, 65540]
    assert {len(c['segs']) for c in LIVE} == {1, 2, 3, 4}
    widths = {(s['src'], s['out'], item_width(s)) for c in LIVE for s in c['segs']}
    assert widths == {('f32', 'f32', 4), ('f32', 'f32', 1), ('u8', 'f32', 4), ('u8', 'f32', 1), ('u8', 'u8', 4), ('u8', 'u8', 8)}
    for c in GR.CASES:            # every boundary case sits on the side of the boundary its name says
        if c['name'].startswith('bound-'):
            form, what = c['name'].split('-')[1:3]
            full = dict(f32x4=4, u8f32x4=4, u8x4=4, u8x8=8)[form]
            w = item_width(c['segs'][0])
            assert w == full if what == 'base' else w < full, c['name']
            assert c['refused'] == (form == 'u8x4' and what != 'base')
    for c in GR.CASES:            # a refused byte copy is one that could only go byte by byte
        if c['refused'] and not c['segs'][0]['notes']:
            assert item_width(c['segs'][0]) == 1 and c['segs'][0]['out'] == 'u8'
    for c in LIVE:                # the work items per row that the row-length cases name
        if c['name'].startswith('len-'):
            s = c['segs'][0]
            assert s['row_elems'] // item_width(s) == int(c['name'].split('-')[2]), c['name']
            assert item_width(s) == dict(f32x4=4, f32x1=1, u8f32x4=4, u8f32x1=1, u8x4=4, u8x8=8)[c['name'].split('-')[1]]


def test_no_source_holds_the_prefill():
    for c in LIVE:
        d, _ = data_of(c)
        for s in d['segs']:
            assert not (s['store'] == (PU if s['src'] == 'u8' else PF)).any(), c['name']


def test_the_kernels_way_gives_the_reference_on_every_case():
    for c in LIVE:
        d, (outs, notes) = data_of(c)
        got, got_notes = launch_model(c, d)
        assert GR.mismatches(got, got_notes, outs, notes) == [], c['name']


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_defect_is_rejected_on_some_case(mutant):
    caught = []
    for c in LIVE:
        d, (outs, notes) = data_of(c)
        got, got_notes = launch_model(c, d, mutant)
        if GR.mismatches(got, got_notes, outs, notes):
            caught.append(c['name'])
    print(mutant, "rejected on", len(caught), "cases, e.g.", caught[:4])
    assert caught, "the case table cannot see: " + mutant


def test_the_note_comparison_rejects_wrong_lists():
    want = [{3, 7}, set(), set(range(88))]

    def buf(rows):
        b = np.full((2 * G + 3, GR.NOTE_ROW), PU, np.uint8)
        b[G:G + 3] = GR.NOTE_NONE
        for f, notes in enumerate(rows):
            b[G + f, :len(notes)] = notes
        return b
    good = buf([[7, 3], [], list(range(87, -1, -1))])
    assert GR.notes_mismatches(good, want) == []
    assert GR.notes_mismatches(buf([[3, 3], [], list(range(88))]), want)            # a note twice
    assert GR.notes_mismatches(buf([[3], [], list(range(88))]), want)               # a note missing
    assert GR.notes_mismatches(buf([[3, 7, 9], [], list(range(88))]), want)         # a note too many
    late = good.copy()
    late[G, 95] = 0
    assert GR.notes_mismatches(late, want)                                          # the terminators do not reach the row's end
    guard = good.copy()
    guard[G + 3, 0] = GR.NOTE_NONE
    assert GR.notes_mismatches(guard, want)                                         # a row behind the batch written
    for w in want:
        assert GR.NOTE_ROW - len(w) >= 8
