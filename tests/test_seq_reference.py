"""tests/seq_reference.py without a GPU: (a) the reference is the oracle's LSTM; (b) an honest fp32 evaluation of every GPU
case stays below half of every bound, local and running, in three summation orders with and without fma; (c) every planted
fault is rejected by the comparison functions the GPU test uses; (d) the case tables reach the dispatch edges they are there
for; (e) nothing but the tie case is flagged; (f) what the three entry points refuse on the host.

Large batches go through the fp32 evaluation with their first and last four rows (S.sub_rows): rows are independent."""
import numpy as np
import pytest

import clvae_amd  # noqa: F401
from clvae_amd import _lib
from oracle import clvae_oracle as O
import seq_reference as S

f32, f64 = np.float32, np.float64
HALF = 0.5


def small(c, inp):
    rows = S.sub_rows(c['B'])
    return S.take_rows(inp, rows), rows


@pytest.fixture(scope="module")
def fwd_runs():
    """(table, case, inputs of the evaluated rows, the default fp32 evaluation's records), computed once, left unchanged"""
    out = []
    for table in ('fwd88', 'bwd88', 'any'):
        for c in S.CASES[table]:
            inp, rows = small(c, S.forward_inputs(c))
            out.append((table, c, inp, rows, S.f32_forward(inp)))
    return out


def bwd_args(c, inp, rows):
    d = S.backward_inputs(c)
    return d['dhs'][rows], d.get('Kz')


# ------------------------------------------------------------------------------------------------ (a) the oracle itself --
@pytest.mark.parametrize("gate_act", (S.HARD, S.LOGISTIC))
def test_the_reference_is_the_oracle(gate_act):
    c = dict(H=9, B=3, T=4, gate_act=gate_act, rowbias=1, h0=1, c0=1)
    inp = S.forward_inputs(c)
    H = c['H']
    x = inp['xproj'].astype(f64) + inp['rowbias'].astype(f64)[:, None]
    Uw, h0, c0 = (inp[k].astype(f64) for k in ('U', 'h0', 'c0'))
    hs, cache = O.lstm_forward(x, np.eye(4 * H), Uw, np.zeros(4 * H), h0, c0, S.GATE_NAME[gate_act])
    free = S.forward_free(inp)
    gates = cache['Z'].copy()
    gates[:, :, 2 * H:3 * H] = np.tanh(gates[:, :, 2 * H:3 * H])
    for got, want in ((free['hs'][0], hs), (free['cs'][0], cache['C']), (free['gates'][0], gates), (free['hT'][0], hs[:, -1]),
                      (free['cT'][0], cache['C'][:, -1])):
        assert np.abs(got - want).max() <= 1e-12
    # the backward on fp32 records; the oracle recomputes g from z_c, so it gets artanh of the stored g
    rec = S.f32_forward(inp)
    dhs = S.backward_inputs(c)['dhs']
    Z = rec['gates'].astype(f64)
    Z[:, :, 2 * H:3 * H] = np.arctanh(Z[:, :, 2 * H:3 * H])
    cache = dict(Z=Z, C=rec['cs'].astype(f64), H=rec['hs'].astype(f64), xs=np.zeros((3, 4, 1)), h0=None, c0=c0,
                 gate_act=S.GATE_NAME[gate_act], in_masks=None)
    dz = O.lstm_backward(dhs.astype(f64), cache, np.zeros((1, 4 * H)), Uw)[4]
    for tie in ('separate', 'fma'):
        ref = S.backward(rec, dhs, inp['U'], inp['c0'], gate_act, tie=tie)['dz']
        assert np.abs(ref[0] - dz).max() <= 1e-12 and not ref[2].any()
    assert np.abs(S.backward(rec, dhs, inp['U'], None, gate_act)['dz'][0] - dz).max() > 1e-3      # c0 matters


def test_the_two_roundings_of_the_kink_differ_at_minus_2p5_only():
    """every float32 within 2^-10 of +-2.5: the derivative rule under separate rounding and under fma"""
    for base in (2.5, -2.5):
        lo, hi = f32(base - 2.0 ** -10), f32(base + 2.0 ** -10)
        z = np.arange(lo.view(np.uint32), hi.view(np.uint32) + 1, dtype=np.int64) if base > 0 else \
            np.arange(hi.view(np.uint32), lo.view(np.uint32) + 1, dtype=np.int64)
        z = z.astype(np.uint32).view(f32)
        assert z.min() == min(lo, hi) and z.max() == max(lo, hi) and len(z) > 8000
        fl = S.tie_flags(z)
        assert sorted(z[fl].tolist()) == ([-2.5] if base < 0 else [])
    assert S.hard_y32(f32(-2.5), 'separate') == 0 and S.hard_y32(f32(-2.5), 'fma') < 0
    up = np.nextafter(f32(2.5), f32(9))
    for tie in ('separate', 'fma'):
        assert S.hard_y32(f32(2.5), tie) <= 1 and S.hard_y32(up, tie) <= 1 and S.hard_y32(np.nextafter(up, f32(9)), tie) > 1
    assert S.DEVICE_TIE in ('separate', 'fma')


# ------------------------------------------------------------------------------------- (b) fp32 stays below half a bound --
def worst(rep):
    return max(rep.values()) if rep else 0.0


def test_fp32_forward_stays_below_half_of_every_bound(fwd_runs):
    top = {}
    for table, c, inp, rows, _ in fwd_runs:
        for order, fma in S.VARIANTS:
            rep = S.judge_forward("%s %r %s fma=%d" % (table, c, order, fma), inp,
                                  S.outputs_of(c, S.f32_forward(inp, order, fma, save=c.get('save', 1))))
            for k, v in rep.items():
                top[k] = max(top.get(k, 0.0), v)
    for c in S.STEP_CASES:
        inp = S.forward_inputs(c)
        for order, fma in S.VARIANTS:
            rep = S.judge_forward("step %r" % (c,), inp, S.f32_forward(inp, order, fma, save=False))
            top['step'] = max(top.get('step', 0.0), worst(rep))
    print("\nfp32 forward, worst error / bound:", ", ".join("%s %.3g" % kv for kv in sorted(top.items())))
    assert max(top.values()) <= HALF, top


def test_fp32_impulse_probes_are_exact():
    for c in S.IMPULSE_88 + S.IMPULSE_ANY:
        if c['B'] > 100:
            continue                                        # the same rows again (b mod H), or H^2 work
        for scale in S.IMPULSE_SCALES:
            inp = S.impulse_inputs(c, scale)
            for order, fma in S.VARIANTS:
                rep = S.judge_impulse("impulse %r x %g" % (c, scale), inp, S.f32_forward(inp, order, fma), scale)
                assert rep['g'] <= HALF
                S.judge_forward("impulse %r" % (c,), inp, S.outputs_of(c, S.f32_forward(inp, order, fma)))


def backward_cases(fwd_runs):
    """(name, case, records, dhs, U, c0, gate, Kz, sum_terms) of every backward the GPU test runs, on the fp32 records"""
    for table, c, inp, rows, rec in fwd_runs:
        if table == 'fwd88':
            continue
        dhs, Kz = bwd_args(c, inp, rows)
        yield "%s %r" % (table, c), c, rec, dhs, inp['U'], inp['c0'], c['gate_act'], Kz, True
    for c in S.CRAFTED:
        rows = S.sub_rows(c['B'])
        rec, dhs, c0 = S.crafted_records(c)
        rec = {k: v[rows] for k, v in rec.items()}
        yield "crafted %r" % (c,), c, rec, dhs[rows], S.make_U(np.random.default_rng(5), 88), None if c0 is None else c0[rows], \
            c['gate_act'], None, True
    for c in S.SELECT_BWD:
        rows = S.sub_rows(c['B'])
        rec, dhs, Uw, _ = S.select_bwd_inputs(c)
        yield "select %r" % (c,), c, {k: v[rows] for k, v in rec.items()}, dhs[rows], Uw, None, c['gate_act'], None, False


def test_fp32_backward_stays_below_half_of_every_bound(fwd_runs):
    top = {}
    for name, c, rec, dhs, Uw, c0, gate_act, Kz, sum_terms in backward_cases(fwd_runs):
        for order, fma in S.VARIANTS:
            got = S.f32_backward(rec, dhs, Uw, c0, gate_act, Kz, order, fma)
            rep, flags = S.judge_backward("%s %s fma=%d" % (name, order, fma), rec, dhs, Uw, c0, gate_act, got, Kz,
                                          sum_terms=sum_terms)
            assert not flags.any(), name                    # (e) only the tie case is flagged
            for k, v in rep.items():
                key = ('select ' if not sum_terms else '') + k
                top[key] = max(top.get(key, 0.0), v)
            if c.get('dh0'):
                assert not got['dz'].any() and not got['dzsum'].any()
    print("\nfp32 backward, worst error / bound:", ", ".join("%s %.3g" % kv for kv in sorted(top.items())))
    assert max(top.values()) <= HALF, top


def test_fp32_selection_probes():
    """dZ of a 0/1 Kz is a column of dz; dh_0 of a selection U picks single entries of dz_1"""
    for c in S.SELECT_Z:
        if c['B'] > 8:
            continue
        rec, dhs, _ = S.crafted_records(dict(H=88, B=c['B'], T=c['T'], gate_act=c['gate_act'], c0=0, dh0=0, plain=1))
        Kz, sel = S.select_z(c)
        for order, fma in S.VARIANTS:
            got = S.f32_backward(rec, dhs, S.make_U(np.random.default_rng(5), 88), None, c['gate_act'], Kz, order, fma)
            assert np.array_equal(got['dZ'], got['dz'][:, :, sel])
    assert sorted(set(np.concatenate([S.select_z(c)[1] for c in S.SELECT_Z]).tolist())) == list(range(352))


# ----------------------------------------------------------------------------------------------- (c) planted faults --
def rejected(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def test_every_forward_fault_is_rejected(fwd_runs):
    caught = {f: 0 for f in S.FWD_FAULTS}
    for table, c, inp, rows, _ in fwd_runs:
        if table != 'fwd88' or c['T'] > 4:
            continue
        for fault in S.FWD_FAULTS:
            got = S.outputs_of(c, S.f32_forward(inp, fault=fault, save=c['save']))
            caught[fault] += rejected(lambda: S.judge_forward("fault", inp, got))
    print("\nforward faults, rejecting cases:", caught)
    assert all(caught.values()), caught
    # a lost term is also what the impulse probe makes exact
    c = S.IMPULSE_88[0]
    inp = S.impulse_inputs(c, 1.0)
    for fault in ('k_lost', 'slice_lost', 'if_swapped', 'zc_stored', 'h0_ignored'):
        assert rejected(lambda: S.judge_impulse("fault", inp, S.f32_forward(inp, fault=fault), 1.0)), fault


def test_every_backward_fault_is_rejected(fwd_runs):
    caught = {f: 0 for f in S.BWD_FAULTS + S.BWDZ_FAULTS}
    for name, c, rec, dhs, Uw, c0, gate_act, Kz, sum_terms in backward_cases(fwd_runs):
        if c['H'] > 128:
            continue
        for fault in S.BWD_FAULTS + (S.BWDZ_FAULTS if Kz is not None else ()):
            got = S.f32_backward(rec, dhs, Uw, c0, gate_act, Kz, fault=fault)
            caught[fault] += rejected(lambda: S.judge_backward("fault", rec, dhs, Uw, c0, gate_act, got, Kz, sum_terms=sum_terms))
    print("\nbackward faults, rejecting cases:", caught)
    assert all(caught.values()), caught
    # the selection probe rejects a lost 22-column slice exactly: g = 0 puts the ones of U into the columns 0..87
    c = S.SELECT_BWD[0]
    rec, dhs, Uw, _ = S.select_bwd_inputs(c)
    got = S.f32_backward(rec, dhs, Uw, None, c['gate_act'], fault='slice_lost')
    assert rejected(lambda: S.judge_backward("fault", rec, dhs, Uw, None, c['gate_act'], got, sum_terms=False))
    # and a wrong tie setting is rejected by the tie case, in the flagged elements, once the flags are off
    c = S.TIE_CASES[0]
    rec, dhs, c0 = S.crafted_records(c)
    Uw = S.make_U(np.random.default_rng(5), 88)
    got = S.f32_backward(rec, dhs, Uw, c0, S.HARD, tie='separate')
    want, bound, flags = S.backward(rec, dhs, Uw, c0, S.HARD, tie='fma')['dz']
    assert flags.any() and rejected(lambda: S.check("tie", got['dz'], want, bound, 88))
    S.check("tie", got['dz'], want, bound, 88, flags)


# ------------------------------------------------------------------------------------------------- (d) table edges --
def test_the_tables_reach_their_edges():
    assert [S.rows_per_wg(B) for B in S.B88] == [1, 1, 1, 1, 2, 1, 2, 4]
    assert [S.rows_per_wg(B) for B in (88, 352, 528, 2, 5)] == [1, 2, 4, 1, 1]
    fwd = S.CASES['fwd88']
    assert {(S.rows_per_wg(c['B']), c['gate_act'], c['save']) for c in fwd} == {(r, g, s) for r in (1, 2, 4) for g in (0, 1) for s in (0, 1)}
    assert {c['T'] for c in fwd} == {0, 1, 2, 3, 4, 33} and {c['B'] for c in fwd} == set(S.B88)
    for k in ('rowbias', 'h0', 'c0', 'hT', 'cT'):
        assert {c[k] for c in fwd} == {0, 1}, k
    assert any(c['h0'] and not c['c0'] for c in fwd) and any(c['alias'] and c['hT'] and c['h0'] for c in fwd)
    assert {c['own'] for c in fwd if c['save']} == {0, 1}
    assert any(c['T'] == 0 and c['hT'] and c['h0'] for c in fwd) and any(c['T'] == 0 and c['cT'] for c in fwd)
    bwd = S.CASES['bwd88']
    assert {(S.rows_per_wg(c['B']), c['gate_act']) for c in bwd} == {(r, g) for r in (1, 2, 4) for g in (0, 1)}     # each with and without latents
    assert {c['T'] for c in bwd} == {0, 1, 2, 3, 4, 5} and {c['nz'] for c in bwd} == set(S.NZ) and {c['pad'] for c in bwd} == {0, 3}
    assert {c['c0'] for c in bwd} == {0, 1} and {c['B'] for c in bwd} == set(S.B88)
    assert {S.latent_group(nz) for nz in S.NZ} == {(1, 1), (1, 3), (1, 4), (2, 1), (2, 4), (3, 1), (8, 4), (10, 3), (10, 4)}
    anyc = [c for c in S.CASES['any'] if not c['force']]
    assert {c['H'] for c in anyc} >= set(S.H_ANY) and any(c['force'] and c['H'] == 88 for c in S.CASES['any'])
    assert [S.la_slices(H) for H in (1, 16, 17, 32, 33, 64, 65, 128, 129, 1024)] == [8, 8, 8, 8, 4, 4, 2, 2, 1, 1]
    assert [S.la_units_per_thread(H) for H in (1, 256, 257, 512, 513, 768, 769, 1024)] == [1, 1, 2, 2, 3, 3, 4, 4]
    assert {(S.la_slices(c['H']), c['gate_act']) for c in anyc} == {(k, g) for k in (1, 2, 4, 8) for g in (0, 1)}
    assert {(S.la_units_per_thread(c['H']), c['gate_act']) for c in anyc} == {(k, g) for k in (1, 2, 3, 4) for g in (0, 1)}
    assert {c['T'] for c in anyc} == {0, 1, 2, 3}
    # the crafted records: every ladder point in every gate block at unit 0, at unit 87 and in between; g = +-1; |c|
    pts = S.ladder_points()
    assert len(set(pts.tolist())) == 13 and f32(-2.5) not in pts and f32(2.5) in pts
    seen = {(k, u): set() for k in (0, 1, 3) for u in (0, 12, 75, 87)}
    for c in S.CRAFTED:
        rec, dhs, c0 = S.crafted_records(c)
        for (k, u) in seen:
            seen[(k, u)] |= set(rec['gates'][:min(c['B'], 16), :, k * 88 + u].ravel().tolist())
        assert set(rec['gates'][:, :, 2 * 88 + 20:2 * 88 + 22].ravel().tolist()) == {1.0, -1.0}
        assert set(np.abs(rec['cs'][:, :, 30:37]).ravel().tolist()) == {0.0, 1.0, 20.0, 100.0}
        assert bool(c['dh0']) == (not dhs.any()) and (c0 is None) == (not c['c0'])
    for key, vals in seen.items():
        assert vals >= set(pts.tolist()), key
    assert {c['T'] for c in S.CRAFTED} == {1, 2, 3} and {S.rows_per_wg(c['B']) for c in S.CRAFTED} == {1, 2, 4}
    assert {(S.rows_per_wg(c['B']), c['force']) for c in S.TIE_CASES} == {(1, 0), (2, 0), (4, 0), (1, 1)}
    assert [S.rows_per_wg(c['B']) for c in S.IMPULSE_88] == [1, 2, 4] and [c['H'] for c in S.IMPULSE_ANY] == [7, 33, 100, 257, 600]
    assert {(S.rows_per_wg(c['B']), c['g']) for c in S.SELECT_BWD if c['H'] == 88} == {(r, g) for r in (1, 2, 4) for g in range(4)}


# -------------------------------------------------------------------------------------------------------- (e) flags --
def test_only_the_tie_case_is_flagged():
    near = S.near_kink                                      # within 8 ulp of +-2.5
    for table in ('bwd88', 'any'):
        for c in S.CASES[table]:
            inp = S.forward_inputs(c)
            z = S.f32_forward(inp)['gates']
            H = c['H']
            for k in (0, 1, 3):
                assert not near(z[:, :, k * H:(k + 1) * H]).any(), (table, c)
    for c in S.CRAFTED:
        rec, _, _ = S.crafted_records(c)
        assert not S.tie_flags(rec['gates']).any()
    for c in S.TIE_CASES:
        rec, dhs, c0 = S.crafted_records(c)
        fl = S.backward(rec, dhs, S.make_U(np.random.default_rng(5), 88), c0, S.HARD)['dz'][2]
        cols = sorted(k * 88 + u for k in (0, 1, 3) for u in S.TIE_UNITS)
        assert fl.all(0).all(0).nonzero()[0].tolist() == cols and fl.sum() == c['B'] * len(cols)


# ---------------------------------------------------------------------------------------------------- (f) refusals --
EINVAL = -1
_buffer = np.zeros(64, np.float32)
BUF = _buffer.ctypes.data + (-_buffer.ctypes.data) % 16          # never dereferenced: every call below is refused on the host


def test_what_the_entry_points_refuse():
    L = _lib.lib()
    P = BUF

    def fwd(B=2, T=3, H=88, gate_act=0, xproj=P, U=P, hs=P, cs=P, gates=P):
        return L.clv_lstm_seq_fwd(B, T, H, gate_act, xproj, None, U, None, None, hs, cs, gates, None, None, None)

    def bwd(B=2, T=3, H=88, gate_act=0, U=P, dhs=P, cs=P, gates=P, dzsum=P):
        return L.clv_lstm_seq_bwd(B, T, H, gate_act, U, dhs, cs, None, gates, dzsum, None)

    def bwd_z(B=2, T=3, H=88, gate_act=0, U=P, dhs=P, cs=P, gates=P, dzsum=P, Kz=P, nz=4, dZ=P, lddz=4):
        return L.clv_lstm_seq_bwd_z(B, T, H, gate_act, U, dhs, cs, None, gates, dzsum, Kz, nz, dZ, lddz, None)

    for f in (fwd, bwd, bwd_z):
        for kw in (dict(H=0), dict(H=-3), dict(H=1025), dict(B=0), dict(B=-1), dict(T=-1), dict(gate_act=2), dict(gate_act=-1),
                   dict(U=None), dict(cs=None) if f is not fwd else dict(hs=None)):
            assert f(**kw) == EINVAL, (f.__name__, kw)
    assert fwd(xproj=None) == EINVAL and fwd(cs=None) == EINVAL            # gates without cs
    for kw in (dict(dhs=None), dict(gates=None), dict(dzsum=None)):
        assert bwd(**kw) == EINVAL and bwd_z(**kw) == EINVAL, kw
    for kw in (dict(H=87), dict(H=89), dict(H=100), dict(nz=0), dict(nz=-1), dict(nz=41, lddz=41), dict(nz=8, lddz=7),
               dict(Kz=None), dict(dZ=None)):
        assert bwd_z(**kw) == EINVAL, kw
