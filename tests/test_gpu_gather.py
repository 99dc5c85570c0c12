"""-m gpu: clv_gather_rows_multi (csrc/pointwise.hip), the mini-batch assembly as a launch of its own, form by form against the
numpy reference of tests/gather_reference.py over its case table -- the table tests/test_gather_reference.py shows to be
strong enough to reject seven kinds of wrong kernel.

Everything is a copy, so everything is bit for bit.  Every output lives inside a larger buffer that is prefilled with a value
no source holds: GUARD output rows in front of and behind the batch's rows, the padding columns of strided outputs, and the
bytes in front of a deliberately misaligned base and behind the buffer's end.  The WHOLE buffer is compared with array_equal
(gather_reference.mismatches), so a write anywhere it does not belong shows, as does an element never written.  A refused
launch must leave every buffer as it was.

The alignment boundaries (bound-*) cannot observe WHICH of the six copy forms ran, only that both sides of every boundary give
the same bytes; tests/test_gather_reference.py::test_case_table_covers_what_it_claims checks that each case sits on the side
its name says, by the predicate of clv_gather_rows_multi.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gather_reference as GR
from helpers import TAIL

pytestmark = pytest.mark.gpu

G = GR.GUARD


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    return torch.device("cuda:0")


def upload(a, dev, mis=0):
    """a flat array as a device tensor whose base sits `mis` elements into a 256-byte aligned allocation"""
    raw = torch.zeros(mis + a.size + 16, dtype=torch.uint8 if a.dtype == np.uint8 else torch.float32, device=dev)
    assert raw.data_ptr() % 256 == 0
    v = raw[mis:mis + a.size]
    v.copy_(torch.as_tensor(a, device=dev))
    return v


class Guarded:
    """an output of shape [GUARD + n + GUARD, ld] inside a prefilled allocation, `mis` elements behind its 256-byte aligned start
    and TAIL elements in front of its end; `out` is what the launch gets: the row behind the leading guard rows"""

    def __init__(self, dev, shape, u8, mis=0):
        self.fill = GR.PREFILL_U8 if u8 else GR.PREFILL_F32
        self.shape, self.mis, self.n = shape, mis, int(np.prod(shape))
        self.raw = torch.full((mis + self.n + TAIL,), self.fill, dtype=torch.uint8 if u8 else torch.float32, device=dev)
        assert self.raw.data_ptr() % 256 == 0
        self.out = self.raw[mis:mis + self.n].view(*shape)[G:]

    def whole(self):
        """the buffer as the reference shapes it, after checking the canaries on both sides of it"""
        r = self.raw.cpu().numpy()
        assert (r[:self.mis] == self.fill).all() and (r[self.mis + self.n:] == self.fill).all(), "write outside the buffer"
        return r[self.mis:self.mis + self.n].reshape(self.shape)

    def untouched(self):
        return bool((self.raw == self.fill).all().item())


class Launch:
    """the device side of one case: sources, row list, tables, guarded outputs and note buffers, and the step counter"""

    def __init__(self, dev, c):
        from clvae_amd import ops
        self.c, self.ops = c, ops
        self.data = d = GR.build(c)
        self.idx = torch.as_tensor(d['idx'], device=dev) if d['idx'] is not None else None
        self.step = torch.zeros(1, dtype=torch.int32, device=dev)
        self.outs, self.notes, self.segs = [], [], []
        for s in d['segs']:
            chunk, pieces, ld, stride = GR.geometry(s)
            o = Guarded(dev, (2 * G + c['rows'] * pieces, ld), s['out'] == 'u8', s['out_mis'])
            nb = Guarded(dev, GR.notes_expected_shape(c['rows'], s), True) if s['notes'] else None
            table = torch.as_tensor(s['table'], device=dev) if s['table'] is not None else None
            self.segs.append((upload(s['store'], dev, s['src_mis']), o.out, s['row_elems'], s['chunk'], s['out_ld'], s['stride'],
                              s['offset'], table))
            self.outs.append(o)
            self.notes.append(nb)

    def run(self, step=None):
        """one launch (step: the value of the device counter; default the case's own); a cursor case reads the device counter"""
        c, cursor = self.c, None
        if c['cursor'] is not None:
            self.step.fill_(int(c['cursor'][0] if step is None else step))
            cursor = (self.step,) + tuple(c['cursor'][1:])
        notes = [n.out if n is not None else None for n in self.notes] if any(n is not None for n in self.notes) else None
        self.ops.gather_rows_multi(c['rows'], self.idx, self.segs, row0=c['row0'], notes=notes, cursor=cursor)

    def mismatches(self, step=None):
        c = self.c
        cur = c['cursor'] if step is None or c['cursor'] is None else (int(step),) + tuple(c['cursor'][1:])
        want, want_notes = GR.assemble(c['rows'], self.data['idx'], c['row0'], cur, self.data['segs'])
        torch.cuda.synchronize()
        return GR.mismatches([o.whole() for o in self.outs], [n.whole() if n is not None else None for n in self.notes], want, want_notes)

    def untouched(self):
        torch.cuda.synchronize()
        return all(b.untouched() for b in self.outs + [n for n in self.notes if n is not None])


@pytest.mark.parametrize("c", GR.CASES, ids=[c['name'] for c in GR.CASES])
def test_gather_rows_multi_case(dev, c):
    from clvae_amd import _lib
    L = Launch(dev, c)
    if c['refused']:
        with pytest.raises(_lib.ClvError):
            L.run()
        assert L.untouched()
        return
    L.run()
    assert L.mismatches() == []


def test_both_sides_of_every_alignment_boundary_hold_the_same_bytes(dev):
    """a boundary case whose only broken condition is a base pointer reads the SAME store and row list as its form's base case
    would at that geometry: run the aligned twin of every such case and compare the two outputs directly, element for element"""
    for c in GR.CASES:
        if c['name'].startswith('bound-') and c['name'].split('-')[2] in ('src_base', 'out_base') and not c['refused']:
            twin = dict(c, segs=[dict(s, src_mis=0, out_mis=0) for s in c['segs']])       # same name: same seed, same data
            a, b = Launch(dev, c), Launch(dev, twin)
            a.run()
            b.run()
            assert a.mismatches() == [] and b.mismatches() == [], c['name']
            for x, y in zip(a.outs, b.outs):
                assert np.array_equal(x.whole(), y.whole()), c['name']


def test_segment_counts_and_cursors_that_are_refused(dev):
    from clvae_amd import _lib, ops
    c = GR.case('refusals', 4, [GR.seg('u8', 'u8', 8), GR.label()], idx=True, cursor=(3, 0, 3, 4, 0))
    L = Launch(dev, c)
    for segs in ([], L.segs + L.segs + L.segs[:1]):                      # nseg 0 and 5
        with pytest.raises(_lib.ClvError):
            ops.gather_rows_multi(4, L.idx, segs)
    for period in (0, -3):
        with pytest.raises(_lib.ClvError):
            ops.gather_rows_multi(4, L.idx, L.segs, cursor=(L.step, 0, period, 4, 0))

    class NoCounter:
        def data_ptr(self):
            return 0
    with pytest.raises(_lib.ClvError):
        ops.gather_rows_multi(4, L.idx, L.segs, cursor=(NoCounter(), 0, 3, 4, 0))
    with pytest.raises(_lib.ClvError):
        ops.gather_rows_multi(0, L.idx, L.segs)
    assert L.untouched()
    L.run()                                                              # and the same arguments, unbroken, are taken
    assert L.mismatches() == []


@pytest.mark.parametrize("name", ["cur-d0-idx", "cur-rank-slice-seq", "notes-windows-cursor"])
def test_a_captured_launch_follows_the_counter_at_replay(dev, name):
    """one launch captured ONCE; the device counter advanced by clv_i32_add between replays, from two steps before the first bound
    step through two full periods: every replay assembles the batch of the counter's value at replay time, not at capture"""
    from clvae_amd import ops
    c = next(x for x in GR.CASES if x['name'] == name)
    step0, period = c['cursor'][1], c['cursor'][2]
    L = Launch(dev, c)
    first = step0 - 2
    L.step.fill_(first + period)                      # captured while the counter names another batch than any replay's first
    cursor = (L.step,) + tuple(c['cursor'][1:])
    notes = [n.out if n is not None else None for n in L.notes] if any(n is not None for n in L.notes) else None
    torch.cuda.synchronize()
    with ops.Graph() as g:
        ops.gather_rows_multi(c['rows'], L.idx, L.segs, row0=c['row0'], notes=notes, cursor=cursor)
    torch.cuda.synchronize()
    assert L.untouched()                              # a capture runs nothing
    L.step.fill_(first)
    seen = set()
    for it in range(2 * period + 3):
        g.launch()
        assert L.mismatches(step=first + it) == [], it
        assert int(L.step.item()) == first + it
        seen.add((first + it - step0) % period)
        ops.i32_add(L.step, 1)
    assert seen == set(range(period))
