"""-m gpu: the filter stream.  clv_smc_resample_carry against clv_smc_resample, clv_smc_commit and
clv_smc_collapse against the numpy reference (tests/stream_filter_reference.py), and FilterStream of both families against
the one generate_smc call: however the piece is cut, emitted frames + finish() and the evidence are that call's, bit for
bit, and the frames go out on the schedule the one-call ancestor table implies."""
import functools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import filter_reference as FR
import smc_reference as SR
import stream_filter_models as MD
import stream_filter_reference as SF
from helpers import make_synthetic_pickle

pytestmark = pytest.mark.gpu

D = MD.D
NAN = float('nan')


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _t(dev, a):
    return torch.as_tensor(np.ascontiguousarray(a), device=dev)


def _counter(dev, c):
    return torch.full((1,), c, dtype=torch.int32, device=dev)


def _bytes(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint8)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bytes(a), _bytes(b))


# ------------------------------------------------------------------ 1. the carry entry
class _Weights:
    """the buffers of clv_smc_resample for a launch of n steps, filled with values no launch writes"""

    def __init__(self, dev, G, P, n):
        f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
        self.logW, self.logZ, self.ess = torch.full((G * P,), NAN, **f64), torch.full((G,), NAN, **f64), torch.full((G, n), NAN, **f64)
        self.nres, self.flag, self.anc = torch.full((G,), -5, **i32), torch.full((G,), -7, **i32), torch.full((n, G * P), -1, **i32)

    def all(self):
        return self.logW, self.logZ, self.ess, self.nres, self.flag, self.anc


def _script(G, P, n):
    """ell [n, G * P]: the `random` script of filter_reference's last case (300 melodies x 5 particles), its columns dealt
    to G melodies x P particles"""
    i = len(FR.RESAMPLE) - 1
    assert FR.RESAMPLE[i]['script'] == 'random'
    return np.ascontiguousarray(FR.resample_script(i).reshape(FR.RS_STEPS, -1)[:n, :G * P])


@pytest.mark.parametrize("tau", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("P", [1, 5, 64, 65])
@pytest.mark.parametrize("G", [1, 3])
def test_carry_entry_is_the_filter_and_continues_it(dev, G, P, tau):
    from clvae_amd import ops
    n, S, seed, m0 = 6, 2, 77, 5
    ell = _script(G, P, n)
    e = torch.zeros(G * P, dtype=torch.float64, device=dev)

    def run(w, step, nsteps, S, counters, rows):
        for c, row in zip(counters, rows):
            e.copy_(_t(dev, ell[row]))
            step(G, P, nsteps, S, seed, m0, tau, e, *w.all(), _counter(dev, c))

    plain = lambda *a: ops.smc_resample(*a)
    carried = lambda t0, carry: (lambda *a: ops.smc_resample_carry(*a, t0, carry))
    # (a) t0 = 0, carry = 0 is clv_smc_resample: a seed step, the six steps, a step past the end; untouched elements too
    a, b = _Weights(dev, G, P, n), _Weights(dev, G, P, n)
    counters, rows = [S - 1] + list(range(S, S + n)) + [S + n], [0] + list(range(n)) + [0]
    run(a, plain, n, S, counters, rows)
    run(b, carried(0, 0), n, S, counters, rows)
    torch.cuda.synchronize()
    for x, y in zip(a.all(), b.all()):
        assert _same_bits(x, y)
    assert not torch.isnan(a.logW).any() and int((a.anc < 0).sum()) == 0
    if tau == 0.0:
        assert int(a.nres.sum()) == 0
    elif P > 1 and tau == 1.0:
        assert int(a.nres.sum()) > 0
    # (b) the same six steps as 2 + 4: the second launch counts its own steps from 0, its Philox steps on from S + 2
    c1 = _Weights(dev, G, P, 2)
    run(c1, carried(0, 0), 2, S, range(S, S + 2), range(2))
    c2 = _Weights(dev, G, P, 4)
    c2.logW, c2.logZ, c2.nres = c1.logW, c1.logZ, c1.nres
    run(c2, carried(S + 2, 1), 4, 0, range(4), range(2, 6))
    torch.cuda.synchronize()
    assert _same_bits(c2.logW, a.logW) and _same_bits(c2.logZ, a.logZ) and _same_bits(c2.nres, a.nres)
    assert _same_bits(torch.cat([c1.anc, c2.anc]), a.anc) and _same_bits(torch.cat([c1.ess, c2.ess], 1), a.ess)
    assert _same_bits(c2.flag, a.flag)


# ------------------------------------------------------------------ 2. commit and collapse against the numpy reference
class _Store:
    """the pending store on the device, driven through the two entries"""

    def __init__(self, dev, G, P, Dn, cap):
        self.dev, self.G, self.P, self.D, self.cap = dev, G, P, Dn, cap
        i32 = dict(dtype=torch.int32, device=dev)
        self.anc = torch.full((cap, G * P), -3, **i32)
        self.hist = torch.full((cap, G * P, Dn), 9, dtype=torch.uint8, device=dev)
        self.head, self.len = torch.zeros(G, **i32), torch.zeros(G, **i32)

    def commit(self, anc, hist, out_cap=None):
        from clvae_amd import ops
        n = anc.shape[0]
        out_cap = self.cap if out_cap is None else out_cap
        ncommit = torch.full((self.G,), -9, dtype=torch.int32, device=self.dev)
        out = torch.full((self.G, out_cap, self.D), 7, dtype=torch.uint8, device=self.dev)
        ops.smc_commit(self.G, self.P, self.D, n, _t(self.dev, anc.astype(np.int32)), _t(self.dev, hist), self.cap, self.anc,
                       self.hist, self.head, self.len, out_cap, ncommit, out)
        torch.cuda.synchronize()
        return ncommit.cpu().numpy(), out.cpu().numpy()

    def live(self, m):
        """melody m's pending steps, oldest first: (anc [len, P] local, hist [len, P, D])"""
        P, h, n = self.P, int(self.head[m]), int(self.len[m])
        slots = [(h + j) % self.cap for j in range(n)]
        a = self.anc.cpu().numpy()[slots][:, m * P:(m + 1) * P].astype(np.int64) - m * P
        return a.reshape(n, P), self.hist.cpu().numpy()[slots][:, m * P:(m + 1) * P].reshape(n, P, self.D)

    def check(self, ref):
        assert np.array_equal(self.len.cpu().numpy(), ref.pending())
        for m in range(self.G):
            a, h = self.live(m)
            assert np.array_equal(a, ref.anc[m]) and np.array_equal(h, ref.hist[m]), m


SHAPES = [(1, 7), (2, 88), (5, 7), (64, 88)]        # P x D: a melody's step in bytes (7, 35) and in words (176, 5632)


@pytest.mark.parametrize("chunks", SF.CHUNKINGS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("P,Dn", SHAPES)
def test_commit_kernel_against_the_reference(dev, P, Dn, chunks):
    anc, hist = SF.table(P, Dn)
    store, ref = _Store(dev, SF.G, P, Dn, SF.STEPS), SF.Pending(SF.G, P, Dn)
    k = 0
    for n in chunks:
        got, out = store.commit(anc[k:k + n], hist[k:k + n])
        want, frames = ref.feed(anc[k:k + n], hist[k:k + n])
        k += n
        assert np.array_equal(got, want)
        for m in range(SF.G):
            assert np.array_equal(out[m, :want[m]], frames[m]) and np.all(out[m, want[m]:] == 7), m
        store.check(ref)


def _weights(rng, G, P):
    lw = rng.standard_normal((G, P)) * 1.5
    return lw - np.log(np.exp(lw).sum(axis=1, keepdims=True))


@pytest.mark.parametrize("P,Dn", SHAPES)
def test_commit_and_collapse_on_a_ring_of_four_slots(dev, P, Dn):
    """two steps at a time into a store of capacity 4; a melody holding more than two steps is collapsed.  The ring wraps."""
    from clvae_amd import ops
    anc, hist = SF.table(P, Dn, start=1)
    G, cap, seed, m0 = SF.G, 4, 4321, 6
    store, ref = _Store(dev, G, P, Dn, cap), SF.Pending(G, P, Dn)
    rng = np.random.default_rng(P)
    wrapped = collapsed = kept = False
    i32 = dict(dtype=torch.int32, device=dev)
    for k in range(0, SF.STEPS, 2):
        got, out = store.commit(anc[k:k + 2], hist[k:k + 2])
        want, frames = ref.feed(anc[k:k + 2], hist[k:k + 2])
        assert np.array_equal(got, want)
        for m in range(G):
            assert np.array_equal(out[m, :want[m]], frames[m]) and np.all(out[m, want[m]:] == 7)
        store.check(ref)
        head, lens = store.head.cpu().numpy(), store.len.cpu().numpy()
        wrapped |= bool((head + lens > cap).any())
        late = lens > 2
        if P == 1:                              # one particle never holds anything back: collapse one melody anyway
            late = np.arange(G) == (k // 2) % G
        if not late.any():
            continue
        collapsed, kept = True, kept or not late.all()
        lw = _weights(rng, G, P)
        logW, pick_of = _t(dev, lw.reshape(-1)), _t(dev, late.astype(np.int32))
        picks, flag = torch.full((G,), -9, **i32), torch.full((G,), -7, **i32)
        anc_row = torch.full((G * P,), -2, **i32)
        out = torch.full((G, cap, Dn), 7, dtype=torch.uint8, device=dev)
        before = [t.clone() for t in (store.anc, store.hist, store.head)]
        ops.smc_collapse(G, P, Dn, seed, m0, k + 2, False, pick_of, logW, cap, store.anc, store.hist, store.head, store.len,
                         cap, picks, out, anc_row, flag)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, (store.anc, store.hist, store.head)))   # the ring is only read
        out, lw_after = out.cpu().numpy(), logW.cpu().numpy().reshape(G, P)
        for m in range(G):
            rows = slice(m * P, (m + 1) * P)
            if late[m]:
                pick = SF.collapse_pick(lw[m], seed, k + 2, m0 + m)
                assert int(picks[m]) == pick and int(flag[m]) == 1 and int(store.len[m]) == 0
                f = ref.take(m, pick)
                assert np.array_equal(out[m, :len(f)], f) and np.all(out[m, len(f):] == 7)
                assert np.array_equal(anc_row[rows].cpu().numpy(), np.full(P, m * P + pick))
                assert np.all(lw_after[m] == -np.log(float(P)))
            else:                               # not touched at all
                assert int(picks[m]) == -9 and int(flag[m]) == -7 and int(store.len[m]) == lens[m]
                assert np.all(out[m] == 7) and np.all(anc_row[rows].cpu().numpy() == -2)
                assert np.array_equal(lw_after[m].view(np.uint8), lw[m].view(np.uint8))
        store.check(ref)
    assert collapsed and kept and (wrapped or P == 1)


def test_final_pick_is_the_backtracks_draw(dev):
    """final_pick: the particle clv_smc_backtrack draws with n_out = 1 at that step, its lineage, and nothing else written"""
    from clvae_amd import ops
    P, Dn, G, seed, m0, step = 5, 88, SF.G, 99, 3, 14
    anc, hist = SF.table(P, Dn, start=2)
    store = _Store(dev, G, P, Dn, SF.STEPS)
    store.anc.copy_(_t(dev, anc.astype(np.int32)))
    store.hist.copy_(_t(dev, hist))
    store.len.fill_(SF.STEPS)
    lw = _weights(np.random.default_rng(1), G, P)
    logW = _t(dev, lw.reshape(-1))
    picks = torch.full((G,), -9, dtype=torch.int32, device=dev)
    out = torch.full((G, SF.STEPS, Dn), 7, dtype=torch.uint8, device=dev)
    ops.smc_collapse(G, P, Dn, seed, m0, step, True, None, logW, SF.STEPS, store.anc, store.hist, store.head, store.len,
                     SF.STEPS, picks, out)
    Xs = torch.zeros(G, 1, SF.STEPS, Dn, device=dev)
    bp = torch.zeros(G, 1, dtype=torch.int32, device=dev)
    ops.smc_backtrack(G, P, SF.STEPS, Dn, 1, seed, m0, step, logW, store.anc, store.hist, Xs, bp)
    torch.cuda.synchronize()
    want, wp = SR.backtrack(lw, anc, hist, 1, seed, step, m0)
    assert np.array_equal(picks.cpu().numpy(), wp[:, 0]) and torch.equal(picks, bp[:, 0])
    assert np.array_equal(out.cpu().numpy().astype(np.float64), want[:, 0]) and torch.equal(out.float(), Xs[:, 0])
    assert np.array_equal(logW.cpu().numpy(), lw.reshape(-1)) and int(store.len.min()) == SF.STEPS


def test_refusals_and_the_capacity_contract(dev):
    from clvae_amd import _lib, ops
    G, P, Dn, n, cap = 2, 3, 8, 2, 4
    R = G * P
    i32 = dict(dtype=torch.int32, device=dev)
    anc, hist = torch.arange(R, **i32).repeat(n, 1), torch.zeros(n, R, Dn, dtype=torch.uint8, device=dev)
    store = _Store(dev, G, P, Dn, cap)
    ncommit, picks, flag = torch.full((G,), -9, **i32), torch.full((G,), -9, **i32), torch.full((G,), -7, **i32)
    out = torch.full((G, cap, Dn), 7, dtype=torch.uint8, device=dev)
    logW = torch.full((R,), -np.log(3.0), dtype=torch.float64, device=dev)
    anc_row = torch.full((R,), -2, **i32)
    ell = torch.zeros(R, dtype=torch.float64, device=dev)
    w = _Weights(dev, G, P, n)

    def commit(G=G, P=P, Dn=Dn, n=n, anc=anc, hist=hist, cap=cap, panc=store.anc, phist=store.hist, head=store.head,
               length=store.len, out_cap=cap, ncommit=ncommit, out=out):
        ops.smc_commit(G, P, Dn, n, anc, hist, cap, panc, phist, head, length, out_cap, ncommit, out)

    def collapse(G=G, P=P, Dn=Dn, final=False, logW=logW, cap=cap, panc=store.anc, head=store.head, picks=picks, out=out,
                 anc_row=anc_row, flag=flag, out_cap=cap):
        ops.smc_collapse(G, P, Dn, 1, 0, 5, final, None, logW, cap, panc, store.hist, head, store.len, out_cap, picks, out,
                         anc_row, flag)

    def carry(G=G, P=P, n=n, tau=0.5, logW=w.logW, anc=w.anc):
        ops.smc_resample_carry(G, P, n, 0, 1, 0, tau, ell, logW, w.logZ, w.ess, w.nres, w.flag, anc, _counter(dev, 0), 0, 0)

    bad = [lambda: commit(G=0), lambda: commit(P=0), lambda: commit(Dn=0), lambda: commit(n=0), lambda: commit(P=1025),
           lambda: commit(cap=0), lambda: commit(out_cap=0), lambda: commit(anc=None), lambda: commit(hist=None),
           lambda: commit(panc=None), lambda: commit(phist=None), lambda: commit(head=None), lambda: commit(length=None),
           lambda: commit(ncommit=None), lambda: commit(out=None),
           lambda: collapse(G=0), lambda: collapse(P=0), lambda: collapse(Dn=0), lambda: collapse(P=1025),
           lambda: collapse(cap=0), lambda: collapse(out_cap=0), lambda: collapse(logW=None), lambda: collapse(panc=None),
           lambda: collapse(head=None), lambda: collapse(picks=None), lambda: collapse(out=None),
           lambda: collapse(anc_row=None), lambda: collapse(flag=None),
           lambda: carry(G=0), lambda: carry(P=0), lambda: carry(P=1025), lambda: carry(n=0), lambda: carry(tau=1.5),
           lambda: carry(logW=None), lambda: carry(anc=None)]
    for call in bad:
        with pytest.raises(_lib.ClvError, match=r"\(-1\)"):
            call()
    torch.cuda.synchronize()
    assert bool((ncommit == -9).all()) and bool((picks == -9).all()) and bool((out == 7).all()) and bool((store.len == 0).all())
    assert torch.isnan(w.logW).all() and bool((w.anc == -1).all())
    collapse(final=True, anc_row=None, flag=None)       # the final draw needs neither
    # a melody whose pending steps and the chunk do not fit the ring is left alone and says so
    store.len.copy_(torch.tensor([3, 1], **i32))
    before = [t.clone() for t in (store.anc, store.hist, store.head, store.len)]
    commit()
    torch.cuda.synchronize()
    assert ncommit.cpu().tolist()[0] == -1 and ncommit.cpu().tolist()[1] >= 0
    rows0 = slice(0, P)
    assert torch.equal(store.anc[:, rows0], before[0][:, rows0]) and torch.equal(store.hist[:, rows0], before[1][:, rows0])
    assert int(store.head[0]) == int(before[2][0]) and int(store.len[0]) == 3 and bool((out[0] == 7).all())


# ------------------------------------------------------------------ 3. end to end, both families
N, P, T, S = 3, 8, 12, 2
FAMILIES = ('cl_vrnn', 'cl_vae')
MODES = ('plain', 'counted', 'tempered')
SEEDS = {'cl_vrnn': 3, 'cl_vae': 7}                   # chosen on the MI355X: see test_stream_is_the_one_call
# of the clamped notes the share `on` is forced on, at most `most` of a frame (the others off).  cl_vae's tiny model gives
# nearly even weights under a roll that mostly forces notes off and then never coalesces: its roll forces four notes on
ROLLS = {'cl_vrnn': dict(on=0.05, most=3), 'cl_vae': dict(on=1.0, most=4)}
_ENGINES = {}


def _engine(dev, family):
    if family not in _ENGINES:
        _ENGINES[family] = MD.vrnn(dev) if family == 'cl_vrnn' else MD.vae(dev)
    return _ENGINES[family]


@functools.lru_cache(maxsize=None)
def _piece(family):
    """seeds, labels and the roll of the family's piece: about 30 % of the notes clamped, at most ROLLS' `most` of a
    frame forced on (so that a count of 3..4 is feasible)"""
    x, w = MD.inputs(N, S if family == 'cl_vrnn' else None, 10 if family == 'cl_vrnn' else 4, 21)
    roll = MD.roll(np.random.default_rng(22), N, T, frac=0.3, on=ROLLS[family]['on'])
    for n in range(N):
        for t in range(T):
            on = np.nonzero(roll[n, t] == 1)[0]
            roll[n, t, on[ROLLS[family]['most']:]] = 0             # the others are forced off: still about 30 % clamped
    return x, w, roll


def _constraints(family, mode, a=0, b=T):
    from clvae_amd.engine_generate import Constraints
    roll = _piece(family)[2][:, a:b]
    return Constraints.between(3, 4, roll=roll) if mode == 'counted' else roll


def _temper(mode):
    return dict(temperature=0.8, z_temperature=0.5) if mode == 'tempered' else {}


_REFERENCE = {}


def _reference(dev, family, mode, tau=0.5, particles=P):
    """the one generate_smc call over the whole roll, computed once: frames, evidence, ESS and the ancestor table"""
    key = (family, mode, tau, particles)
    if key not in _REFERENCE:
        x, w, _ = _piece(family)
        res, kept = MD.one_call(_engine(dev, family), x, w, T, _constraints(family, mode), particles, resample_threshold=tau,
                                seed=SEEDS[family], **_temper(mode))
        assert len(kept) == 1
        _REFERENCE[key] = dict(Xs=res.Xs[:, 0].cpu().numpy().astype(np.float64), logZ=res.log_evidence.cpu().numpy(),
                               ess=res.ess.cpu().numpy(), anc=kept[0].anc.cpu().numpy().astype(np.int64),
                               nres=res.resamples.cpu().numpy())
    return _REFERENCE[key]


def _stream(dev, family, **kw):
    from clvae_amd.stream import FilterStream
    x, w, _ = _piece(family)
    kw.setdefault('particles', P)
    return FilterStream(MD.model_of(_engine(dev, family)), x, w, kw.pop('particles'), seed=SEEDS[family], **kw)


def schedule_report(dev):
    """the reference schedules of every family and mode (what the seeds were chosen by): lines of text"""
    lines = []
    for family in FAMILIES:
        for mode in MODES:
            ref = _reference(dev, family, mode)
            for chunks in SF.CHUNKINGS:
                lines.append("%s %s seed %d chunks %s: resamples %s counts %s left %s" % (
                    family, mode, SEEDS[family], "x".join(map(str, chunks)), ref['nres'].tolist(),
                    SF.schedule(ref['anc'], P, chunks).tolist(), (T - SF.schedule(ref['anc'], P, chunks).sum(0)).tolist()))
    return lines


@pytest.mark.parametrize("chunks", SF.CHUNKINGS, ids=lambda c: "x".join(map(str, c)))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", FAMILIES)
def test_stream_is_the_one_call(dev, family, mode, chunks):
    """Emitted frames + finish() = generate_smc(...).Xs[:, 0] and log_evidence = its log_evidence, bit for bit, and the counts
    after every advance are those the one-call ancestor table implies (stream_filter_reference.schedule).
    Seeds 3 (cl_vrnn) and 7 (cl_vae) with the rolls of _piece were chosen on the MI355X among seeds 1..12 / 1..10 so that,
    by the one-call table, in every mode at least one melody emits before finish() and at least one still holds frames
    at finish() (asserted below).  Frames emitted before finish() per melody, of 12 (the same for every chunking: what is
    final once all frames are fed does not depend on the cuts), and the resamples:
      cl_vrnn  plain [3, 5, 0] (resamples [4, 4, 3])   counted [2, 5, 5] ([3, 3, 4])   tempered [0, 3, 0] ([4, 4, 3])
      cl_vae   plain [0, 0, 6] ([2, 4, 3])             counted [0, 4, 0] ([2, 3, 2])   tempered [8, 4, 6] ([2, 4, 3])
    schedule_report prints the counts per advance."""
    ref = _reference(dev, family, mode)
    want = SF.schedule(ref['anc'], P, chunks)
    before_finish = want.sum(0)
    assert (before_finish > 0).any() and (before_finish < T).any(), want      # the guard: a condition on the reference
    s = _stream(dev, family)
    k = 0
    for i, n in enumerate(chunks):
        frames, counts = s.advance(_constraints(family, mode, k, k + n), **_temper(mode))
        k += n
        assert np.array_equal(counts, want[i]), (i, counts, want[i])
        assert np.array_equal(s.pending, k - want[:i + 1].sum(0)) and s.t == (S if family == 'cl_vrnn' else 0) + k
        assert np.array_equal(s.ess.view(np.uint8), np.ascontiguousarray(ref['ess'][:, k - n:k]).view(np.uint8))
        assert frames.shape == (N, counts.max(), D)
    frames, counts = s.finish()
    assert np.array_equal(counts, T - before_finish)
    out = np.stack(s.emitted)
    assert out.shape == ref['Xs'].shape and np.array_equal(out, ref['Xs'])
    assert np.array_equal(s.log_evidence.view(np.uint8), ref['logZ'].view(np.uint8))
    assert np.array_equal(s.collapses, np.zeros(N))
    with pytest.raises(ValueError):
        s.advance(_constraints(family, mode, 0, 1))


@pytest.mark.parametrize("family", FAMILIES)
def test_without_resampling_nothing_is_final_before_the_end(dev, family):
    ref = _reference(dev, family, 'plain', tau=0.0)
    assert int(ref['nres'].sum()) == 0
    s = _stream(dev, family, resample_threshold=0.0)
    for k in range(0, T, 4):
        frames, counts = s.advance(_constraints(family, 'plain', k, k + 4))
        assert np.array_equal(counts, np.zeros(N)) and np.array_equal(s.pending, np.full(N, k + 4))
    frames, counts = s.finish()
    assert np.array_equal(counts, np.full(N, T)) and np.array_equal(np.stack(s.emitted), ref['Xs'])
    assert np.array_equal(s.log_evidence.view(np.uint8), ref['logZ'].view(np.uint8))


@pytest.mark.parametrize("family", FAMILIES)
def test_one_particle_is_the_clamped_stream(dev, family):
    """P = 1: every lineage is the only one, every advance emits all its frames, and they are Stream.advance(clamp=...)'s"""
    from clvae_amd.stream import Stream
    x, w, roll = _piece(family)
    s = _stream(dev, family, particles=1)
    plain = Stream(MD.model_of(_engine(dev, family)), x, w, seed=SEEDS[family])
    for a, b in ((0, 5), (5, 6), (6, 12)):
        frames, counts = s.advance(roll[:, a:b])
        assert np.array_equal(counts, np.full(N, b - a)) and np.array_equal(s.pending, np.zeros(N))
        assert np.array_equal(frames, plain.advance(b - a, clamp=roll[:, a:b]))
        assert s.t == plain.t
    frames, counts = s.finish()
    assert np.array_equal(counts, np.zeros(N)) and frames.shape == (N, 0, D)


# ------------------------------------------------------------------ 4. collapse and max_lag
def _honoured(frames, roll):
    c = roll <= 1
    return np.array_equal(frames[c], roll[c].astype(np.float64))


@pytest.mark.parametrize("family", FAMILIES)
def test_collapse_restarts_a_melody_from_one_particle(dev, family):
    x, w, roll = _piece(family)
    s = _stream(dev, family)
    s.advance(roll[:, :5])
    st = s.state
    lens = s.pending.copy()
    lw = st.logW.cpu().numpy().reshape(N, P).copy()
    rows = [b.clone() for b in st.buffers()]
    store = _Store(dev, N, P, D, st.cap)
    store.anc, store.hist, store.head, store.len = st.pend_anc.clone(), st.pend_hist.clone(), st.head.clone(), st.len.clone()
    logZ, t = s.log_evidence, s.t
    which = [0, 2]
    frames, counts = s.collapse(which)
    assert s.state.t == t and np.array_equal(s.log_evidence.view(np.uint8), logZ.view(np.uint8))
    assert np.array_equal(s.collapses, [1, 0, 1]) and np.array_equal(s.pending, [0, lens[1], 0])
    assert np.array_equal(counts, [lens[0], 0, lens[2]])
    lw_after = s.state.logW.cpu().numpy().reshape(N, P)
    for m in range(N):
        mine = slice(m * P, (m + 1) * P)
        if m in which:
            pick = SF.collapse_pick(lw[m], SEEDS[family], t, m)
            assert s.picks[m] == pick
            a, h = store.live(m)
            assert np.array_equal(frames[m, :counts[m]], SF.lineage_frames(a, h, pick).astype(np.float64))
            for now, was in zip(s.state.buffers(), rows):       # all P rows hold the picked row's state
                assert _same_bits(now[mine], was[m * P + pick].expand(P, -1))
            assert np.all(lw_after[m] == -np.log(float(P)))
        else:
            assert s.picks[m] == -1
            for now, was in zip(s.state.buffers(), rows):
                assert _same_bits(now[mine], was[mine])
            assert np.array_equal(lw_after[m].view(np.uint8), lw[m].view(np.uint8))
    frames, counts = s.advance(roll[:, 5:])                     # the next advance runs
    s.finish()
    out = np.stack(s.emitted)
    assert out.shape == (N, T, D) and _honoured(out, roll) and set(np.unique(out)) <= {0.0, 1.0}
    # the melody that was not collapsed still returns the one call's frames
    assert np.array_equal(out[1], _reference(dev, family, 'plain')['Xs'][1])


@pytest.mark.parametrize("tau", [0.0, 0.5])
@pytest.mark.parametrize("family", FAMILIES)
def test_max_lag_bounds_what_is_held_back(dev, family, tau):
    x, w, roll = _piece(family)
    s = _stream(dev, family, resample_threshold=tau, max_lag=2)
    forced, real = np.zeros(N, np.int64), s.collapse

    def spy(index=None):
        forced[np.asarray(index)] += 1
        return real(index)
    s.collapse = spy
    total = np.zeros(N, np.int64)
    for k in range(0, T, 2):
        frames, counts = s.advance(roll[:, k:k + 2])
        total += counts
        assert (s.pending <= 2).all() and np.array_equal(total + s.pending, np.full(N, k + 2))
    frames, counts = s.finish()
    out = s.emitted
    assert all(o.shape == (T, D) for o in out) and _honoured(np.stack(out), roll)
    assert np.array_equal(s.collapses, forced)
    if tau == 0.0:                      # nothing ever coalesces: every second advance forces every melody
        assert np.array_equal(forced, np.full(N, 3))


# ------------------------------------------------------------------ 5. the state's round trip
@pytest.mark.parametrize("family", FAMILIES)
def test_state_round_trip_continues_bit_for_bit(dev, family, tmp_path):
    from clvae_amd.engine_generate import FilterState
    x, w, roll = _piece(family)
    eng = _engine(dev, family)
    kw = dict(particles=P, seed=SEEDS[family])
    first = eng.filter_advance(None, x, w, roll[:, :5], **kw)
    np.savez(str(tmp_path / "state.npz"), **first.state.to_numpy())
    back = FilterState.from_numpy(np.load(str(tmp_path / "state.npz")), dev)
    ends = []
    for state in (first.state, back):
        nxt = eng.filter_advance(state, None, w, roll[:, 5:], **kw)
        fin = eng.filter_collapse(nxt.state, final=True, seed=SEEDS[family])
        torch.cuda.synchronize()
        ends.append((nxt.frames, torch.as_tensor(nxt.counts), nxt.ess, fin.frames, torch.as_tensor(fin.counts),
                     torch.as_tensor(fin.picks), *nxt.state.buffers(), *[getattr(nxt.state, k) for k in ('logW', 'logZ', 'nres')]))
    assert len(ends[0]) == len(ends[1]) and all(_same_bits(a, b) for a, b in zip(*ends))
    assert first.state.t == (S if family == 'cl_vrnn' else 0) + T


# ------------------------------------------------------------------ 6. the sample tools with --live
@pytest.mark.parametrize("which", FAMILIES)
def test_live_cli_writes_the_files_of_the_one_call(dev, tmp_path, capsys, which):
    import importlib
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, HARMONIZE_FLAGS, LIVE_FLAGS, parser_for
    SM = importlib.import_module('clvae_amd.%s.sample' % which)
    TR = importlib.import_module('clvae_amd.%s.train' % which)
    data = make_synthetic_pickle(str(tmp_path / "syn.pickle"), n_songs=(10, 4, 4), seed=1)
    mdir = str(tmp_path / "models")
    os.makedirs(mdir)
    extra = ['--latent_dim', '4', '--batch_size', '50'] if which == 'cl_vae' else ['--seq_length', '8', '--batch_size', '20']
    np.random.seed(0)
    TR.train(TR.build_parser().parse_args(['m', '--use_x_prev', '--num_epochs', '2', '--patience', '0', '--train_file', data,
                                           '--model_dir', mdir] + extra))
    parser = parser_for('%s.sample' % which, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS + LIVE_FLAGS)

    def run(name, flags):
        sdir = str(tmp_path / name)
        os.makedirs(sdir)
        args = parser.parse_args(['h', '-n', '3', '-t', '8', '--seed', '4', '-i', os.path.join(mdir, 'm.h5'), '--train_file', data,
                                  '--sample_dir', sdir, '--harmonize', 'top', '--particles', '8'] + flags)
        np.random.seed(3)
        capsys.readouterr()
        rolls = SM.sample(args)
        files = {f: open(os.path.join(sdir, f), 'rb').read() for f in sorted(os.listdir(sdir))}
        return rolls, files, capsys.readouterr().out

    rolls, files, printed = run('whole', [])
    live_rolls, live_files, live_printed = run('live', ['--live', '4'])
    assert len(files) >= 6 and files == live_files
    assert all(np.array_equal(a, b) for a, b in zip(rolls, live_rolls))
    evidence = lambda text: [line for line in text.splitlines() if 'log p(voice) per frame' in line]
    assert len(evidence(printed)) == 3 and evidence(printed) == evidence(live_printed)
    assert sum(line.startswith('live chunk') for line in live_printed.splitlines()) == 2
    lag_rolls, lag_files, lag_printed = run('lag', ['--live', '4', '--max_lag', '2'])
    lines = [line for line in lag_printed.splitlines() if line.startswith('live chunk')]
    assert len(lines) == 2 and all('emitted' in line and 'pending' in line for line in lines)
    assert all(max(int(v) for v in line.split('pending')[1].split()) <= 2 for line in lines)
    assert sorted(lag_files) == sorted(files) and all(r.shape == (8, 88) for r in lag_rolls)
