"""fp64 reference of the large-batch LSTM pass (include/clvae.h: clv_lstm_mx_fwd / clv_lstm_mx_bwd).

Written from the header's contract, not from the kernels' structure, out of oracle/clvae_oracle.py and tests/pair_reference.py:

  forward   xs = X[:, :nx] . Kx + Z[:, :nz] . Kz + rowbias, O.lstm_forward from zero state, and the backward coefficients
            (PR.coefficients) as the kernels' UNIT-major records: coef [B*T,H,4] = (ki, kf, kg, ko), aux [B*T,H,2] =
            (kcarry, kc); the pre-activations come along for PR.kink_mask.
  backward  (a) the oracle's BPTT end to end, (b) PR.bptt_from_coefficients from GIVEN records (the kernel's own):
            dz [B,T,4H] gate-major (what the kernel writes over coef), dzsum [B,4H], dZ = dz . Kz^T [B*T,nz].
  bf16      round to nearest even, split3 (x = p0 + p1 + p2, the kernels' three pieces) and piece_product: a product from a
            chosen subset of the nine piece pairs, accumulated in fp32 -- what the matrix cores are meant to compute, and,
            with a pair left out, what they compute when one MFMA is lost.

check_forward / check_backward / assert_exact are the comparisons of tests/test_gpu_mx.py; tests/test_mx_reference.py feeds
them planted faults on the CPU.  The builders of the GPU test's inputs (make_case, ladder_frames, exact_*) live here for the
same reason: the CPU test shows the faults on the very inputs the kernels get.
"""
import numpy as np

from oracle import clvae_oracle as O
import pair_reference as PR

H, G4 = PR.H, PR.G4
WAVE_UNITS = 12         # forward wave w owns the units 12 w .. 12 w + 11 (wave 7: 84 .. 87)
NBLK = 8
DELTA = 1e-4            # hard-sigmoid coefficients whose fp64 pre-activation is this close to a kink are left out ...
KINK_SHARE = 1e-3       # ... at most this share of a case's coefficients
KINK_PER_SLICE = 4      # ... and at most this many of one (row, step)
FLIP_GUARD = 1e-5       # no case has an fp64 pre-activation this close to a kink: an fp32 pre-activation (about 100 terms of
                        # magnitude below 10, each rounding 6e-7 at most, 2e-6 as a random walk) stays on its fp64 side
SLICE_RTOL, SLICE_ATOL = PR.SLICE_RTOL, PR.SLICE_ATOL

MX_FAST, MX_PAD, MX_NXMAX, MX_NZMAX = 8, 16, 96, 32
LADDER = (0, 1, 4, 5, 8, 9, 12, 15, 16, 17, 19, 20)       # + nx - 1 and nx: every path of the note-list consumer


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


# ---- records ---------------------------------------------------------------------------------------------------------
def to_records(gates, aux_pair):
    """gates [B,T,4H] gate-major, aux_pair [B*T,2,H]  ->  coef [B*T,H,4], aux [B*T,H,2]"""
    BT = aux_pair.shape[0]
    return (np.ascontiguousarray(gates.reshape(BT, 4, H).transpose(0, 2, 1)),
            np.ascontiguousarray(aux_pair.transpose(0, 2, 1)))


def from_records(coef, aux, B, T):
    """coef [B*T,H,4], aux [B*T,H,2]  ->  gates [B,T,4H] gate-major, aux_pair [B*T,2,H]"""
    coef, aux = np.asarray(coef, np.float64).reshape(B * T, H, 4), np.asarray(aux, np.float64).reshape(B * T, H, 2)
    return coef.transpose(0, 2, 1).reshape(B, T, G4), np.ascontiguousarray(aux.transpose(0, 2, 1))


# ---- forward / backward ------------------------------------------------------------------------------------------------
def forward(B, T, X, Kx, Z, Kz, rowbias, U, gate_act):
    """X [B*T,nx] or None, Kx [nx,4H]; Z [B*T,nz] or None, Kz [nz,4H]; rowbias [B,4H] or None; U [H,4H]"""
    xs = np.zeros((B * T, G4))
    if X is not None:
        xs = xs + np.asarray(X, np.float64) @ Kx
    if Z is not None:
        xs = xs + np.asarray(Z, np.float64) @ Kz
    xs = xs.reshape(B, T, G4)
    if rowbias is not None:
        xs = xs + rowbias[:, None, :]
    hs, cache = O.lstm_forward(xs, np.eye(G4), U, np.zeros(G4), gate_act=gate_act)
    gates, aux_pair = PR.coefficients(cache, gate_act)
    coef, aux = to_records(gates, aux_pair)
    return dict(hs=hs, coef=coef, aux=aux, gates=gates, aux_pair=aux_pair, pre=cache['Z'], cache=cache, gate_act=gate_act)


def _backward(dz, Kz):
    return dict(dz=dz, dzsum=dz.sum(1), dZ=None if Kz is None else dz.reshape(-1, G4) @ Kz.T)


def backward_oracle(fwd, dhs, U, Kz=None):
    """(a): the oracle's BPTT from the reference forward's own pre-activations"""
    return _backward(O.lstm_backward(dhs, fwd['cache'], np.eye(G4), U)[4], Kz)


def backward_coef(coef, aux, dhs, U, Kz=None):
    """(b): BPTT from given records coef [B*T,H,4], aux [B*T,H,2] and dL/dh [B,T,H]"""
    B, T, _ = dhs.shape
    gates, aux_pair = from_records(coef, aux, B, T)
    return _backward(PR.bptt_from_coefficients(gates, aux_pair, U, dhs), Kz)


# ---- bf16 pieces -------------------------------------------------------------------------------------------------------
def bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def split3(x):
    """x = p0 + p1 + p2 exactly, each a bf16 (csrc/common.h); returns [3, ...] fp32"""
    x = np.asarray(x, np.float32)
    p0 = bf16_round(x)
    r1 = x - p0
    p1 = bf16_round(r1)
    return np.stack([p0, p1, bf16_round(r1 - p1)])


ALL_PAIRS = tuple((p, q) for p in range(3) for q in range(3))       # (piece of the activation, piece of the weight)
SECOND_ORDER = ((1, 1), (0, 2), (2, 0))                               # about 2^-16 of the product each


def piece_product(a, W, pairs=ALL_PAIRS, kblock=32, lost=None):
    """a [M,K] . W [K,N] from the given piece pairs: every bf16 x bf16 product is exact in fp32; one fp32 accumulator per
    activation piece (the pieces of the activation sit in different columns of the MFMA), k in blocks of `kblock` (what one
    k-step of the kernel holds of this product) with the weight pieces inside a block as the kernels issue them, every
    single addition rounded to fp32 (an MFMA rounds no more often than that), the three accumulators summed at the end like
    the butterfly does.  lost = (s, q): the one MFMA of k-step s and weight piece q is skipped."""
    ap, Wp = split3(a), split3(W)
    M, K = ap.shape[1:]
    acc = np.zeros((3, M, W.shape[1]), np.float32)
    for p in range(3):
        for k0 in range(0, K, kblock):
            for q in range(3):
                if (p, q) not in pairs or lost == (k0 // kblock, q):
                    continue
                for k in range(k0, min(k0 + kblock, K)):
                    acc[p] = acc[p] + ap[p][:, k, None] * Wp[q][None, k, :]
    return ((acc[0] + acc[1]) + acc[2]).astype(np.float64)


def _pieces_with_signs(rng, shape, lo, hi, s0, s1, s2):
    """fp32 values of magnitude lo..hi whose three pieces carry the signs s0, s1, s2 (broadcast over shape); the second and
    third piece sit at 0.40 .. 0.48 of the ulp above them: as large as a piece gets without coming near a tie"""
    p0 = bf16_round((rng.uniform(lo, hi, shape) * s0).astype(np.float32))
    ulp0 = 2.0 ** (np.floor(np.log2(np.abs(p0.astype(np.float64)))) - 7)
    p1 = bf16_round((rng.uniform(0.40, 0.48, shape) * ulp0 * s1).astype(np.float32))
    ulp1 = 2.0 ** (np.floor(np.log2(np.abs(p1.astype(np.float64)))) - 7)
    p2 = rng.uniform(0.40, 0.48, shape) * ulp1 * s2
    return f32(p0.astype(np.float64) + p1.astype(np.float64) + p2)


def _sgn(x):
    return np.where(np.asarray(x) < 0, -1.0, 1.0)


def coherent_weights(rng, a_row, N, lo, hi):
    """W [K,N] for the activation row a_row [K]: the second-order terms of a_row . W all have one sign per pair
    (piece 1 of W follows piece 1 of a, piece 2 of W piece 0 of a, piece 0 of W piece 2 of a), so a lost pair shows as a
    SUM of K terms and not as their random walk; the first-order products keep random signs."""
    p = split3(a_row)
    return _pieces_with_signs(rng, (a_row.shape[0], N), lo, hi, _sgn(p[2])[:, None], _sgn(p[1])[:, None], _sgn(p[0])[:, None])


def crafted_activations(rng, M, K, lo, hi, alternate=False):
    """a [M,K] whose piece signs depend on k only: coherent_weights(a[0]) is then coherent for every row.  alternate: the
    third piece's sign is the first's for even k and its opposite for odd k; coherent_weights gives W's first piece the
    sign of a's third, so the first-order products a . W then alternate in sign along k and their partial sums -- what an
    fp32 accumulator rounds on -- stay near one term's size, while the second-order sums still grow with K."""
    s = [np.where(rng.random(K) < 0.5, -1.0, 1.0)[None, :] for _ in range(3)]
    if alternate:
        s[2] = s[0] * np.where(np.arange(K) % 2, -1.0, 1.0)[None, :]
    return _pieces_with_signs(rng, (M, K), lo, hi, *s)


# ---- the exactness probes (tests/test_gpu_mx.py, f) --------------------------------------------------------------------
# Bounds on |kernel's product - fp64 product| for the probes below: EXACT_MARGIN x the error of piece_product (nine pairs,
# fp32 accumulation, k in the blocks of EXACT_KBLOCK) against fp64 on the same inputs, measured on the CPU
# (test_mx_reference.py re-measures it and shows that every dropped second-order pair, and every single lost MFMA of the
# weights' third piece, exceeds the bound by 2x or more).  The margin is for the summation order inside an MFMA and the
# butterfly.  Measured emulation errors (products of magnitude up to 4.4 / 5.5 / 2.3 / 2.2): hU 2.10e-6 (with the CPU's
# stand-in for the kernel's h_0: the fp64 h_0 rounded to fp32), zKz 3.01e-6, dzUT 8.5e-7, dzKzT 6.5e-7.  A dropped
# second-order pair moves these products by 3.1e-5 .. 6.4e-5 / 8.6e-5 .. 1.0e-4 / 2.7e-4 / 2.6e-4 .. 2.7e-4, one lost MFMA
# (k-step s, weight piece 2) by 2.0e-5 .. 2.9e-5 / 8.6e-5 / 2.5e-5 .. 2.9e-5 / 2.5e-5 .. 3.1e-5.
# Margins of those faults over the bounds: a dropped pair 3.7x .. 7.7x / 7.1x .. 8.3x / 79x / 101x, one lost MFMA 2.3x ..
# 3.5x / 7.1x / 7.4x .. 8.4x / 9.5x .. 11.8x.  None of the four bounds was measured on a GPU or adjusted to a GPU's result:
# they are the CPU emulation's errors x EXACT_MARGIN; test_gpu_mx.py prints each probe's largest error next to its bound.
EXACT_MARGIN = 4
EXACT_BOUND = {'hU': 8.4e-6, 'zKz': 1.2e-5, 'dzUT': 3.4e-6, 'dzKzT': 2.6e-6}
# what one k-step (one MFMA per weight piece) holds of a probe's reduction index: 32 units of h or 32 latents in the
# forward pass; in the backward pass k = 4 unit + gate and the probes' dz has the input gate only: 8 units
EXACT_KBLOCK = {'hU': 32, 'zKz': 32, 'dzUT': 8, 'dzKzT': 8}
# the forward probes read z_f back from kcarry = fl(0.2f z + 0.5): half an ulp of kcarry < 1 is 2^-25, times 5; z itself is
# fl(product + bias) with |z| < 2.5: half an ulp of that is 2^-23; and 0.2f - 0.2 = 3e-9 on |z| < 2.5, times 5
EXACT_READBACK = 2.0 ** -23 + 5 * 2.0 ** -25 + 5 * 2.5 * abs(float(np.float32(0.2)) - 0.2)
EXACT_B = 5             # one full workgroup and one with a single row


def exact_probe(kind, a_row0=None, seed=11):
    """(a [EXACT_B,K], W [K,N]) of one probe.  hU: a is the h_0 the caller has (the kernel's; on the CPU a stand-in), W =
    U's forget block, about 16 x an orthogonal matrix's entries; the other three craft a as well."""
    rng = np.random.default_rng(seed + sorted(EXACT_BOUND).index(kind))
    if kind == 'hU':
        return None, coherent_weights(rng, np.asarray(a_row0, np.float32), H, 0.65, 1.3)
    if kind == 'zKz':
        a = crafted_activations(rng, EXACT_B, MX_NZMAX, 0.5, 1.0)
        return a, coherent_weights(rng, a[0].astype(np.float32), H, 0.5, 1.0)
    # backward: the accumulators start at zero (the forward ones carry the cancelling bias), so alternating first-order
    # terms of like magnitude keep them small, and with them the rounding the bound has to allow
    a = crafted_activations(rng, EXACT_B, H, 0.75, 1.0, alternate=True)
    return a, coherent_weights(rng, a[0].astype(np.float32), H if kind == 'dzUT' else MX_NZMAX, 0.75, 1.0)


def cancelling(rng, prod, spread):
    """the input that cancels prod up to a random rest below `spread`: -fp32(prod) + rest"""
    return f32(-f32(prod) + rng.uniform(-spread, spread, prod.shape))


def assert_exact(kind, got, a, W, readback=False):
    """|got - a . W| <= EXACT_BOUND[kind] (+ EXACT_READBACK) for every element; returns the largest error"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(a, np.float64) @ np.asarray(W, np.float64))
    bound = EXACT_BOUND[kind] + (EXACT_READBACK if readback else 0.0)
    assert np.isfinite(err).all(), "%s: non-finite product" % kind
    if err.max() > bound:
        r, c = np.unravel_index(int(err.argmax()), err.shape)
        raise AssertionError("%s: product of row %d, column %d off by %.3e, bound %.3e (%d of %d elements beyond it)"
                             % (kind, r, c, err.max(), bound, int((err > bound).sum()), err.size))
    return float(err.max())


def exact_fwd_step0(seed=5):
    """step-0 float frames and their kernel for the hU probe: h_0 depends on them alone (zero state: the forget gate's
    pre-activation does not reach h_0, and the row bias of the probe is zero outside the forget block)"""
    rng = np.random.default_rng(seed)
    nx = 24
    X = np.zeros((EXACT_B, 2, nx))
    for b in range(EXACT_B):
        X[b, 0, rng.permutation(nx)[:6]] = f32(rng.standard_normal(6))
    return X.reshape(EXACT_B * 2, nx), f32(rng.standard_normal((nx, G4)) * 0.7)


# ---- comparisons ---------------------------------------------------------------------------------------------------------
def _blocks(a):
    """[..., H] -> [..., 8, 12]: the unit blocks of the forward waves (zeros / False behind unit 87)"""
    a = np.asarray(a)
    pad = np.zeros(a.shape[:-1] + (NBLK * WAVE_UNITS - H,), a.dtype)
    return np.concatenate([a, pad], -1).reshape(a.shape[:-1] + (NBLK, WAVE_UNITS))


def sliced(got, ref, names, name, exclude=None):
    """PR.assert_close_sliced over every axis of got [..., H] with the unit axis cut into wave blocks"""
    ref = np.asarray(ref, np.float64)
    try:
        return PR.assert_close_sliced(_blocks(np.asarray(got, np.float64)), _blocks(ref), tuple(range(len(names))),
                                      SLICE_ATOL * max(np.abs(ref).max(), 1e-30), SLICE_RTOL,
                                      exclude=None if exclude is None else _blocks(exclude), name=name)
    except AssertionError as e:
        raise AssertionError("%s [axes: %s]" % (e, ", ".join("%d = %s" % (i, n) for i, n in enumerate(names))))


def elementwise(got, want, tol, names, name, exclude=None):
    """|got - want| <= tol per element (tol broadcasts); the message names the first element beyond it"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bad = ~(np.abs(got - want) <= np.broadcast_to(tol, got.shape))         # NaN is bad
    if exclude is not None:
        bad &= ~exclude
    if bad.any():
        idx = np.unravel_index(int(np.flatnonzero(bad)[0]), got.shape)
        raise AssertionError("%s: %d element(s) off, first at %s: got %r, want %r" % (
            name, int(bad.sum()), ", ".join("%s %d" % (n, i) for n, i in zip(names, idx)), got[idx], want[idx]))


def kink_exclusions(pre, gate_act):
    """PR.kink_mask at DELTA, [B,T,4H] -- within the caps, or the case is no fair test of the coefficients"""
    ex = PR.kink_mask(pre, gate_act, DELTA)
    B, T, _ = pre.shape
    per = ex.reshape(B * T, G4).sum(1)
    assert ex.sum() <= KINK_SHARE * ex.size, "kinks: %d of %d coefficients left out" % (ex.sum(), ex.size)
    assert per.max() <= KINK_PER_SLICE, "kinks: %d coefficients of (row %d, step %d) left out" % (
        per.max(), per.argmax() // T, per.argmax() % T)
    return ex


FWD_AXES = ('row', 'step', 'gate', 'unit block')


def check_forward(ref, hs, coef, aux, name=''):
    """hs [B*T,H], coef [B*T,H,4], aux [B*T,H,2] of one forward launch against forward()'s result: per element at the pair
    test's bounds, per slice (row, step, gate / record slot, wave's unit block).  Returns the kink-excluded count."""
    B, T, _ = ref['pre'].shape
    hs = np.asarray(hs, np.float64).reshape(B, T, H)
    elementwise(hs, ref['hs'], 5e-6, ('row', 'step', 'unit'), name + 'hs')
    sliced(hs, ref['hs'], ('row', 'step', 'unit block'), name + 'hs')
    got = np.asarray(coef, np.float64).reshape(B, T, H, 4).transpose(0, 1, 3, 2)
    want = ref['gates'].reshape(B, T, 4, H)
    ex = kink_exclusions(ref['pre'], ref['gate_act']).reshape(B, T, 4, H)
    elementwise(got, want, 2e-5 * (1 + np.abs(want)), ('row', 'step', 'gate', 'unit'), name + 'coef', exclude=ex)
    nex = sliced(got, want, FWD_AXES, name + 'coef', exclude=ex)
    ga = np.asarray(aux, np.float64).reshape(B, T, H, 2).transpose(0, 1, 3, 2)
    wa = ref['aux_pair'].reshape(B, T, 2, H)
    elementwise(ga[:, :, 0], wa[:, :, 0], 5e-6, ('row', 'step', 'unit'), name + 'kcarry')
    elementwise(ga[:, :, 1], wa[:, :, 1], 1e-5, ('row', 'step', 'unit'), name + 'kc')
    sliced(ga, wa, ('row', 'step', 'slot', 'unit block'), name + 'aux')
    return nex


def check_backward(ref, dz, dzsum, dZ, Kz=None, name='', exclude=None, slices=True):
    """dz [B*T,4H] (gate-major), dzsum [B,4H], dZ [B*T,nz] (valid columns) of one backward launch against backward_*():
    dz per element at the pair test's bound; dzsum and dZ per element at what that bound lets through the sum over the steps
    and the product with Kz; everything per slice.  Those two element bounds are worst cases and loose (dZ at nz = 32: some
    4e-3 on values near 2), so for dzsum and dZ the slice checks -- 1e-4 of a (row), (step), (gate) or (latent) slice's
    largest value -- are what binds: one wrong element that is small beside the largest of each of its slices passes.  slices=False, exclude [B,T,4H]: form (a), the end-to-end comparison,
    is per element only, as in the pair test, and with hard-sigmoid gates leaves out dz near a kink (and with it the sums
    over such elements: dzsum and dZ are compared under (b))."""
    B, T, _ = ref['dz'].shape
    want = ref['dz'].reshape(B, T, 4, H)
    dz = np.asarray(dz, np.float64).reshape(B, T, 4, H)
    ex = None if exclude is None else exclude.reshape(B, T, 4, H)
    elementwise(dz, want, 3e-5 * (1 + np.abs(want)), ('row', 'step', 'gate', 'unit'), name + 'dz', exclude=ex)
    if slices:
        sliced(dz, want, FWD_AXES, name + 'dz', exclude=ex)
    if ex is not None:
        return
    ws = ref['dzsum'].reshape(B, 4, H)
    ds = np.asarray(dzsum, np.float64).reshape(B, 4, H)
    elementwise(ds, ws, 3e-5 * (T + np.abs(want).sum(1)), ('row', 'gate', 'unit'), name + 'dzsum')
    if slices:
        sliced(ds, ws, ('row', 'gate', 'unit block'), name + 'dzsum')
    if Kz is not None:
        nz = Kz.shape[0]
        wz = ref['dZ'].reshape(B, T, nz)
        gz = np.asarray(dZ, np.float64).reshape(B, T, nz)
        tol = 3e-5 * ((1 + np.abs(ref['dz'])).reshape(B * T, G4) @ np.abs(Kz).T).reshape(B, T, nz)
        elementwise(gz, wz, tol, ('row', 'step', 'latent'), name + 'dZ')
        if slices:
            PR.assert_close_sliced(gz, wz, (0, 1, 2), SLICE_ATOL * max(np.abs(wz).max(), 1e-30), SLICE_RTOL,
                                   name=name + 'dZ [axes: 0 = row, 1 = step, 2 = latent]')


# ---- inputs of the GPU test's cases ------------------------------------------------------------------------------------
def frame_values(rng, n, kind):
    """n values of notes that are on: float frames take negative and fractional ones, byte frames 1 .. 255"""
    if kind == 'u8':
        return rng.integers(1, 256, n).astype(np.float64)
    v = f32(rng.standard_normal(n) * 1.2)
    return np.where(np.abs(v) < 0.05, 0.75, v)


def ladder_counts(nx):
    return sorted(set(min(c, nx) for c in LADDER + (nx - 1, nx)))


def padded_slots(count):
    """the list slots behind `count` notes that the producer pads and the consumer's last round of four reads"""
    return range(count, (count + 3) & ~3) if count >= MX_PAD else range(0)


def ladder_order(nx):
    """the ladder's counts in the order a row meets them step after step (cyclically).  A step's list lies in the buffer
    that held the list of two steps earlier, so wherever lists can be padded (nx > MX_PAD) the even places run
    nx, nx - 1, 17, 20, 19: two steps before every frame whose tail is padded stands a frame with more notes, and each
    padded slot that a list of this nx can fill at all holds a real note of it -- a producer that shortens or drops the
    padding then adds that note's kernel row, and does not depend on what the CU held before the launch.  (Slot 95 behind
    94 or 95 notes at nx = 95 is the one no list fills.)"""
    counts = ladder_counts(nx)
    if nx <= MX_PAD:
        return counts
    chain = [nx, nx - 1, 17, 20, 19]
    rest = [c for c in counts if c not in chain]
    order = []
    for c in chain:
        order += [c, rest.pop(0)]
    return order + rest


def ladder_frames(rng, B, T, nx, kind, rot):
    """X [B*T,nx]: frame (b, t) holds exactly order[(5 b + t + rot) % len] notes at random columns, order = ladder_order(nx);
    over rot = 0 .. len - 1 every (row, step) sees every count.  Float frames: the notes that are off are 0.0 or -0.0."""
    order = ladder_order(nx)
    X = np.zeros((B * T, nx))
    if kind != 'u8':
        X[rng.random(X.shape) < 0.5] = -0.0
    n = np.empty(B * T, int)
    for b in range(B):
        for t in range(T):
            n[b * T + t] = order[(5 * b + t + rot) % len(order)]
            X[b * T + t, rng.permutation(nx)[:n[b * T + t]]] = frame_values(rng, n[b * T + t], kind)
    return X, n


def note_list(frame):
    """the note list the producer makes of one frame: (column, value) of the notes that are on, by column"""
    cols = np.flatnonzero(frame != 0)
    return [(int(k), float(frame[k])) for k in cols]


def stale_notes(c, f):
    """for frame f (= b T + t, t >= 2) of a ladder case: {padded slot: the (column, value) that the list of frame f - 2, the
    last one written to the same buffer, holds there, or None where that list is shorter}"""
    assert f % c['T'] >= 2
    before = note_list(c['X'][f - 2])
    return {s: before[s] if s < len(before) else None for s in padded_slots(int(c['counts'][f]))}


def make_case(B, T, nx, nz, gate_act, kind='f32', seed=0, rowbias=True, u_scale=1.5, density=0.08, X=None, search=False):
    """inputs (fp32 values) of one forward / backward pair and the fp64 reference forward.  kind: 'f32' float frames with
    values other than 1, 'u8' byte frames.  The kernel rows are scaled so that a full frame stays inside the gates' range.
    Hard-sigmoid gates: no fp64 pre-activation may lie within FLIP_GUARD of a kink, so that the end-to-end backward
    comparison (a) does not hang on which side an fp32 pre-activation falls.  A seed that does not meet this is an error;
    with search=True (the ladder's many launches) the seed moves on by 7919 until one does.  c['seed'] is the seed used."""
    while True:
        c = _make_case(B, T, nx, nz, gate_act, kind, seed, rowbias, u_scale, density, X)
        if not PR.kink_mask(c['ref']['pre'], gate_act, FLIP_GUARD).any():
            return c
        assert search, "seed %d: an fp64 pre-activation within %.0e of a kink; choose another seed" % (seed, FLIP_GUARD)
        seed += 7919


def _make_case(B, T, nx, nz, gate_act, kind, seed, rowbias, u_scale, density, X):
    rng = np.random.default_rng(seed)
    c = dict(B=B, T=T, nx=nx, nz=nz, gate_act=gate_act, kind=kind, seed=seed)
    c['U'] = f32(O.orthogonal(rng, (H, G4), np.float64) * u_scale)
    vmag = 100.0 if kind == 'u8' else 1.0
    c['Kx'] = f32(rng.standard_normal((max(nx, 1), G4)) * 1.6 / (vmag * max(1.0, np.sqrt(density * nx)))) if nx else None
    c['Kz'] = f32(rng.standard_normal((nz, G4)) * 0.4) if nz else None
    if nx and X is None:
        X = np.zeros((B * T, nx))
        on = rng.random(X.shape) < density
        X[on] = frame_values(rng, int(on.sum()), kind)
    c['X'] = X if nx else None
    c['Z'] = f32(rng.standard_normal((B * T, nz))) if nz else None
    c['rb'] = f32(rng.standard_normal((B, G4)) * (0.5 if nx or nz else 2.0)) if rowbias else None
    c['dhs'] = f32(rng.standard_normal((B, T, H)))
    c['ref'] = forward(B, T, c['X'], c['Kx'], c['Z'], c['Kz'], c['rb'], c['U'], gate_act)
    return c


# id: (B, T, nx, nz, gate, frames, rowbias, scale of U, seed).  The twelve forward instances <GATE, HASZ, XMODE>, T = 1 .. 5 (the
# lookahead clamps), one long odd T, B = 1 .. 5 and 9, 258 workgroups with a single row in the last, nx = 1, 5, 7, 95,
# nz = 0, 1, 15, 16, 17, 31, 32 (the backward dispatch flips at 16 | 17).  T = 131 takes the pair test's U (its bounds are
# known to hold over 128 steps of an orthogonal U; 1.5 x that amplifies a rounding error from step to step).
HS, SG = 'hard_sigmoid', 'sigmoid'
CASES = {
    'hs-f32-T1':     (1, 1, 88, 0, HS, 'f32', True, 1.5, 1000),
    'hs-z1-u8-T2':   (2, 2, 95, 1, HS, 'u8', True, 1.5, 1003),
    'hs-z15-T3':     (3, 3, 0, 15, HS, None, True, 1.5, 1004),
    's-z16-f32-T4':  (4, 4, 7, 16, SG, 'f32', True, 1.5, 1010),
    's-z17-u8-T5':   (5, 5, 5, 17, SG, 'u8', False, 1.5, 1011),
    's-z31-T8':      (9, 8, 0, 31, SG, None, True, 1.5, 1012),
    'hs-z32-f32-T9': (9, 9, 1, 32, HS, 'f32', True, 1.5, 1006),
    's-u8-T131':     (4, 131, 88, 0, SG, 'u8', True, 1.0, 1009),
    'hs-u8-B1029':   (1029, 2, 96, 0, HS, 'u8', True, 1.5, 80192),
    'hs-none-T12':   (3, 12, 0, 0, HS, None, True, 1.5, 1001),
    's-none-T2':     (5, 2, 0, 0, SG, None, True, 1.5, 1008),
    's-f32-T9':      (2, 9, 60, 0, SG, 'f32', False, 1.5, 1007),
    'hs-z32-T2':     (6, 2, 0, 32, HS, None, False, 1.5, 8924),
}
LADDER_NX = (1, 5, 6, 7, 88, 95, 96)
LADDER_B, LADDER_T = 9, 7           # three workgroups, the last with one real row; steps 0, 1, 2, 3, T - 2, T - 1 and one more


def case(cid):
    B, T, nx, nz, gate, kind, rowbias, u_scale, seed = CASES[cid]
    return make_case(B, T, nx, nz, gate, kind or 'f32', seed=seed, rowbias=rowbias, u_scale=u_scale)


def ladder_case(nx, kind, rot):
    """one launch of the note-count ladder: hard-sigmoid gates, a latent input on the odd rotations"""
    rng = np.random.default_rng(nx * 1000 + rot * 2 + (kind == 'u8'))
    X, counts = ladder_frames(rng, LADDER_B, LADDER_T, nx, kind, rot)
    c = make_case(LADDER_B, LADDER_T, nx, 3 * (rot & 1), HS, kind, seed=nx * 77 + rot, density=0.12, X=X, search=True)
    c['counts'] = counts
    return c
