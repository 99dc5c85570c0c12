"""CPU: tests/mx_reference.py, the fp64 reference of the lstm_mx kernels, against itself and a finite difference -- and the
sensitivity of the comparisons tests/test_gpu_mx.py makes (the same functions, the same constants, the same inputs), so that
the GPU test is known to catch a lost piece pair, a lost or stale note, a shifted step, a stray clone row, a missing store."""
import numpy as np
import pytest

import mx_reference as MR

H, G4 = MR.H, MR.G4


def _outputs(c, **kw):
    """(hs [B*T,H], coef, aux) of the reference forward of case c with some inputs replaced"""
    a = dict(X=c['X'], Kx=c['Kx'], Z=c['Z'], Kz=c['Kz'], rb=c['rb'], U=c['U'])
    a.update(kw)
    r = MR.forward(c['B'], c['T'], a['X'], a['Kx'], a['Z'], a['Kz'], a['rb'], a['U'], c['gate_act'])
    return [r['hs'].reshape(-1, H), r['coef'], r['aux']]


@pytest.fixture(scope="module")
def ladder():
    return MR.ladder_case(88, 'f32', 3)


@pytest.fixture(scope="module")
def zcase():
    c = MR.case('hs-z32-f32-T9')
    c['bwd'] = MR.backward_coef(c['ref']['coef'], c['ref']['aux'], c['dhs'], c['U'], c['Kz'])
    return c


# ---- the reference itself --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ['hs-z32-f32-T9', 's-z16-f32-T4', 'hs-none-T12'])
def test_record_bptt_is_the_oracle_bptt(cid):
    """(b) fed the reference's own records is (a): the backward check on the kernel's records rests on this"""
    c = MR.case(cid)
    a = MR.backward_oracle(c['ref'], c['dhs'], c['U'], c['Kz'])
    b = MR.backward_coef(c['ref']['coef'], c['ref']['aux'], c['dhs'], c['U'], c['Kz'])
    for k in ('dz', 'dzsum', 'dZ'):
        if a[k] is not None:
            np.testing.assert_allclose(b[k], a[k], rtol=1e-10, atol=1e-14, err_msg=k)
    assert (a['dZ'] is None) == (c['nz'] == 0)


def test_record_layouts_round_trip():
    rng = np.random.default_rng(0)
    B, T = 3, 2
    gates, aux_pair = rng.standard_normal((B, T, G4)), rng.standard_normal((B * T, 2, H))
    coef, aux = MR.to_records(gates, aux_pair)
    assert coef.shape == (B * T, H, 4) and aux.shape == (B * T, H, 2)
    # unit-major: [row][unit][ki, kf, kg, ko] and [row][unit][kcarry, kc]
    assert coef[4, 17, 2] == gates[2, 0, 2 * H + 17] and aux[5, 80, 1] == aux_pair[5, 1, 80]
    g2, a2 = MR.from_records(coef, aux, B, T)
    assert np.array_equal(g2, gates) and np.array_equal(a2, aux_pair)


def test_gradient_is_the_finite_difference():
    """dZ, dzsum (= d/d rowbias) and dz . Kx^T (= d/dX) of sum(hs * R) on a tiny sigmoid case"""
    c = MR.make_case(2, 3, 4, 2, 'sigmoid', seed=3)
    R = c['dhs']
    g = MR.backward_oracle(c['ref'], R, c['U'], c['Kz'])
    dX = g['dz'].reshape(-1, G4) @ c['Kx'].T

    def loss(**kw):
        a = dict(X=c['X'], Z=c['Z'], rb=c['rb'])
        a.update(kw)
        return float((MR.forward(2, 3, a['X'], c['Kx'], a['Z'], c['Kz'], a['rb'], c['U'], 'sigmoid')['hs'] * R).sum())

    e = 1e-6
    for key, grad, idx in (('Z', g['dZ'], [(0, 0), (2, 1), (5, 0)]), ('rb', g['dzsum'], [(0, 5), (1, H + 7), (1, 3 * H + 80)]),
                           ('X', dX, [(0, 1), (3, 2), (5, 3)])):
        for i in idx:
            hi, lo = c[key].copy(), c[key].copy()
            hi[i] += e
            lo[i] -= e
            fd = (loss(**{key: hi}) - loss(**{key: lo})) / (2 * e)
            assert abs(fd - grad[i]) <= 1e-8 + 1e-6 * abs(grad[i]), (key, i, fd, grad[i])


def test_bf16_pieces():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(4096) * np.exp(rng.standard_normal(4096) * 3)).astype(np.float32)
    p = MR.split3(x)
    assert np.array_equal(p[0].astype(np.float64) + p[1].astype(np.float64) + p[2].astype(np.float64), x.astype(np.float64))
    assert not (p.view(np.uint32) & 0xFFFF).any()                   # bf16 values
    # ties to even: 1 + 2^-8 lies between 1 and 1 + 2^-7 and goes to the even 1; 1 + 3 * 2^-8 goes up to 1 + 2^-6
    assert MR.bf16_round(np.float32(1 + 2.0 ** -8)) == 1.0 and MR.bf16_round(np.float32(1 + 3 * 2.0 ** -8)) == 1 + 2.0 ** -6
    a, W = MR.f32(rng.standard_normal((3, 40))), MR.f32(rng.standard_normal((40, 5)))
    assert np.abs(MR.piece_product(a, W) - a @ W).max() < 1e-5
    assert np.abs(MR.piece_product(a, W, [(0, 0)]) - a @ W).max() > 1e-3       # bf16 x bf16 alone


# ---- the kink condition of every hard-sigmoid GPU case ---------------------------------------------------------------
@pytest.mark.parametrize("cid", [k for k, v in MR.CASES.items() if v[4] == MR.HS])
def test_kink_caps_hold_for_the_gpu_cases(cid):
    c = MR.case(cid)
    ex = MR.kink_exclusions(c['ref']['pre'], MR.HS)          # asserts the share and the per-(row, step) cap
    assert not MR.PR.kink_mask(c['ref']['pre'], MR.HS, MR.FLIP_GUARD).any()
    print("%s: %d of %d coefficients within %.0e of a kink" % (cid, ex.sum(), ex.size, MR.DELTA))


@pytest.mark.parametrize("kind", ['f32', 'u8'])
@pytest.mark.parametrize("nx", MR.LADDER_NX)
def test_kink_caps_hold_for_the_ladder(nx, kind):
    seen = set()
    for rot in range(len(MR.ladder_counts(nx))):
        c = MR.ladder_case(nx, kind, rot)
        MR.kink_exclusions(c['ref']['pre'], MR.HS)
        assert not MR.PR.kink_mask(c['ref']['pre'], MR.HS, MR.FLIP_GUARD).any()
        n = c['counts'].reshape(MR.LADDER_B, MR.LADDER_T)
        assert (n == (c['X'] != 0).sum(1).reshape(n.shape)).all()        # -0.0 is off
        seen |= {(int(n[b, t]), b, t) for b in range(MR.LADDER_B) for t in range(MR.LADDER_T)}
    # every count at every step (0, 1, 2, 3, T - 2, T - 1 among them) of every row (the four positions of a workgroup and
    # the single row of the last one)
    assert seen == {(k, b, t) for k in MR.ladder_counts(nx) for b in range(MR.LADDER_B) for t in range(MR.LADDER_T)}
    assert sorted(MR.ladder_order(nx)) == MR.ladder_counts(nx)
    assert set(MR.ladder_counts(88)) == {0, 1, 4, 5, 8, 9, 12, 15, 16, 17, 19, 20, 87, 88}


@pytest.mark.parametrize("kind", ['f32', 'u8'])
@pytest.mark.parametrize("nx", [n for n in MR.LADDER_NX if n > MR.MX_PAD])
def test_ladder_puts_a_real_note_behind_every_padded_tail(nx, kind):
    """the padded tail (16 notes or more, no multiple of four) is visible only if something stands where the padding
    belongs: for every such frame from step 2 on, each padded slot below nx -- each that a list can fill -- holds a note of
    the list written to the same buffer two steps earlier, with a value that is not zero; 17 and 19 notes meet that at
    every step from 2 on in every row"""
    padded = [k for k in MR.ladder_counts(nx) if len(MR.padded_slots(k))]
    assert {17, 19, nx - 1} <= set(padded)
    seen = set()
    for rot in range(len(MR.ladder_counts(nx))):
        c = MR.ladder_case(nx, kind, rot)
        for f in range(c['B'] * c['T']):
            k, t = int(c['counts'][f]), f % c['T']
            if k in padded and t >= 2:
                stale = MR.stale_notes(c, f)
                assert list(stale) == list(MR.padded_slots(k)) and len(stale) == -k % 4
                for slot, note in stale.items():
                    if slot < nx:
                        assert note is not None and note[1] != 0 and c['X'][f - 2, note[0]] == note[1], (rot, f, slot)
                    else:
                        assert note is None and nx == 95 and slot == 95
                seen.add((k, f // c['T'], t))
    assert seen == {(k, b, t) for k in padded for b in range(MR.LADDER_B) for t in range(2, MR.LADDER_T)}


# ---- planted faults: each must fail the GPU test's comparison --------------------------------------------------------
def _frame_with(c, counts, min_t=0):
    """the first frame with one of these counts at step min_t or later; from step 2 on (where the list buffer held the list
    of the same row's frame f - 2) only behind a frame that was not empty"""
    T = c['T']
    return next(f for f in range(c['B'] * T) if c['counts'][f] in counts and f % T >= min_t
                and (f % T < 2 or c['counts'][f - 2] > 0))


def _drop_note(c, pos):
    f = _frame_with(c, (17, 19, 20))
    X = c['X'].copy()
    X[f, np.flatnonzero(X[f] != 0)[pos]] = 0.0
    return _outputs(c, X=X)


def _stale_entry(c):
    """a frame of 17 or 19 notes whose padding was not written: the consumer's last round adds the entry that the list of
    two steps earlier (the same buffer) really holds at position `count`: MR.stale_notes"""
    f = _frame_with(c, (17, 19), min_t=2)
    col, v = MR.stale_notes(c, f)[int(c['counts'][f])]
    X = c['X'].copy()
    X[f, col] += v
    return _outputs(c, X=X)


def _next_frame_at_the_end(c):
    B, T = c['B'], c['T']
    X = c['X'].copy()
    for b in range(B):
        X[b * T + T - 1] = c['X'][(b * T + T) % (B * T)]
    return _outputs(c, X=X)


def _clone_row(c):
    """rows beyond B write what they computed from other inputs (no row bias) into row B - 1"""
    B, T = c['B'], c['T']
    rb = c['rb'].copy()
    rb[B - 1] = 0.0
    bad, out = _outputs(c, rb=rb), _outputs(c)
    for o, b in zip(out, bad):
        o[(B - 1) * T:] = b[(B - 1) * T:]
    return out


def _z_shifted(c):
    B, T = c['B'], c['T']
    Z = c['Z'].reshape(B, T, -1)
    return _outputs(c, Z=np.concatenate([Z[:, 1:], Z[:, -1:]], 1).reshape(B * T, -1))


def _aux_swapped(c):
    out = _outputs(c)
    out[2][:, 40] = out[2][:, 40, ::-1]
    return out


def _wave7_unit(c):
    """unit 86 multiplies unit 85's columns of U"""
    U = c['U'].copy()
    U[:, 86::H] = U[:, 85::H]
    return _outputs(c, U=U)


FWD_FAULTS = [
    ("the note at list position 8 dropped", 'ladder', lambda c: _drop_note(c, 8)),
    ("the note at list position 16 dropped", 'ladder', lambda c: _drop_note(c, 16)),
    ("a stale list entry read behind 17 or 19 notes", 'ladder', _stale_entry),
    ("frame t + 1 used for frame t at t = T - 1", 'ladder', _next_frame_at_the_end),
    ("the clone rows of a partial workgroup write into row B - 1", 'ladder', _clone_row),
    ("z_{t+1} used for z_t", 'zcase', _z_shifted),
    ("kcarry and kc swapped for one unit", 'zcase', _aux_swapped),
    ("one unit of wave 7 wrong", 'zcase', _wave7_unit),
]


@pytest.mark.parametrize("k", range(len(FWD_FAULTS)), ids=[f[0] for f in FWD_FAULTS])
def test_forward_check_rejects_planted_faults(request, k):
    name, fix, make = FWD_FAULTS[k]
    c = request.getfixturevalue(fix)
    MR.check_forward(c['ref'], *[MR.f32(o) for o in _outputs(c)])           # fp32 rounding of the right answer passes
    with pytest.raises(AssertionError, match=r"(row|step|unit|slot|gate)") as e:
        MR.check_forward(c['ref'], *make(c))
    print(name, '->', e.value)


def _dz0_not_stored(c, b):
    dz = b['dz'].copy()
    dz[:, 0] = c['ref']['coef'].reshape(c['B'], c['T'], G4)[:, 0]           # the forward record is still there
    return dz, b['dzsum'], b['dZ']


def _dz_stored_and_summed_wrong(c, b):
    dz = b['dz'].copy()
    dz[:, 2, 3 * H:] *= 1 + 1e-3
    return dz, dz.sum(1), b['dZ']


BWD_FAULTS = [
    ("dz_0 not stored for odd T", _dz0_not_stored),
    ("dzsum missing its last step", lambda c, b: (b['dz'], b['dzsum'] - b['dz'][:, 0], b['dZ'])),
    ("one step's gate block stored and summed wrong alike", _dz_stored_and_summed_wrong),
    ("dZ_0 from the image of step 1", lambda c, b: (b['dz'], b['dzsum'], np.concatenate(
        [b['dZ'].reshape(c['B'], c['T'], -1)[:, 1:2], b['dZ'].reshape(c['B'], c['T'], -1)[:, 1:]], 1))),
]


@pytest.mark.parametrize("k", range(len(BWD_FAULTS)), ids=[f[0] for f in BWD_FAULTS])
def test_backward_check_rejects_planted_faults(zcase, k):
    c, b = zcase, zcase['bwd']
    assert c['T'] % 2 == 1
    MR.check_backward(b, MR.f32(b['dz']), MR.f32(b['dzsum']), MR.f32(b['dZ']), Kz=c['Kz'])
    with pytest.raises(AssertionError, match=r"(row|step|unit|gate|latent)") as e:
        MR.check_backward(b, *BWD_FAULTS[k][1](c, b), Kz=c['Kz'])
    print(BWD_FAULTS[k][0], '->', e.value)


def _probe(kind):
    if kind == 'hU':         # the CPU's stand-in for the kernel's h_0: the fp64 h_0 of the probe's step-0 frames, as fp32
        X, Kx = MR.exact_fwd_step0()
        h0 = MR.f32(MR.forward(MR.EXACT_B, 2, X, Kx, None, None, None, np.zeros((H, G4)), MR.HS)['hs'][:, 0])
        return h0, MR.exact_probe(kind, h0[0])[1]
    return MR.exact_probe(kind)


@pytest.mark.parametrize("kind", sorted(MR.EXACT_BOUND))
def test_exactness_bounds_are_the_emulation_and_catch_every_lost_pair(kind):
    """EXACT_BOUND[kind] is EXACT_MARGIN x the error of the nine-pair fp32-accumulated product on the probe's inputs; every
    dropped second-order pair is beyond it by 2x or more, and so is every single lost MFMA of the weights' third piece
    (k-step s, q = 2: all the kernel can lose in one line without a first-order error)"""
    a, W = _probe(kind)
    kb = MR.EXACT_KBLOCK[kind]
    readback = MR.EXACT_READBACK if kind in ('hU', 'zKz') else 0.0
    emul = MR.assert_exact(kind, MR.piece_product(a, W, kblock=kb), a, W)
    assert 0.9 * MR.EXACT_BOUND[kind] <= MR.EXACT_MARGIN * emul <= 1.1 * MR.EXACT_BOUND[kind], (kind, emul)
    assert readback < 0.05 * MR.EXACT_BOUND[kind]
    faults = [("pair %s" % (pair,), dict(pairs=[p for p in MR.ALL_PAIRS if p != pair])) for pair in MR.SECOND_ORDER]
    faults += [("MFMA (s = %d, q = 2)" % s, dict(lost=(s, 2))) for s in range(-(-a.shape[1] // kb))]
    for name, kw in faults:
        got = MR.piece_product(a, W, kblock=kb, **kw)
        err = np.abs(got - a @ W).max()
        assert err >= 2 * (MR.EXACT_BOUND[kind] + readback), (kind, name, err)
        with pytest.raises(AssertionError, match=r"row \d+, column \d+"):
            MR.assert_exact(kind, got, a, W, readback=readback > 0)
        print("%s without %s: %.2e, bound %.2e, emulation %.2e" % (kind, name, err, MR.EXACT_BOUND[kind], emul))
