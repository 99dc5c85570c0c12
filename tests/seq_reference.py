"""fp64 reference of clv_lstm_seq_fwd / clv_lstm_seq_bwd / clv_lstm_seq_bwd_z (csrc/lstm.hip, csrc/lstm_any.hip) with a bound
for every element, the probes that make a misplaced term exact, the case tables that tests/test_seq_reference.py (no GPU),
tests/test_gpu_seq.py and tests/seq_worker.py share, and an fp32 evaluation of the same contract in which faults can be planted.

Written from the contract of include/clvae.h and from oracle/clvae_oracle.py (O.lstm_forward / O.lstm_backward):
  z_t = xproj[b,t] + rowbias[b] + h_{t-1} . U;  i, f, o = gate_act(z_i, z_f, z_o);  g = tanh(z_c);  c_t = f c_{t-1} + i g;
  h_t = o tanh(c_t);  gates = (z_i, z_f, g, z_o);  the backward turns gates into dz and writes dzsum = sum_t dz.

forward     forward_local(records, inputs): every step on its own, from the DEVICE's stored h_{t-1}, c_{t-1}; the error of a
            step does not grow with T and a stale state shows at the step where it happens.  forward_free(inputs): the oracle's
            recurrence end to end with a running first-order bound (eh_0 = 0; ez_t = local + eh_{t-1} . |U|; the gates by
            their Lipschitz constants 0.2 / 0.25 / 1; c and h by the product rule).
backward    backward(records, dhs, U, c0, gate_act, Kz): a pure function of the fp32 records it is given (the device
            forward's or crafted ones), so every hard-sigmoid kink is decided exactly as the kernel must decide it: the
            derivative is 0.2 where the FLOAT32 value y = 0.2 z + 0.5 lies in [0, 1].  `tie` says how that float32 y is
            rounded: 'separate' (product, then sum) or 'fma'; the two differ at z = -2.5 only (separate: y = 0, passes; fma:
            y = -7.45e-9, clipped), which is flagged.  DEVICE_TIE is what the compiled kernels do.
            dzsum and dZ are judged against the fp64 sum / product of the device's OWN stored dz.
bounds      U_ = 2^-24.  A pre-activation is a sum of n = H + 2 terms in any order, fused or not: (n + 1) U_ sum |terms|.
            Elementwise stages are counted in ulps: an ordinary operation OP = 2 U_ of its result (pointwise_reference.py);
            hard sigmoid: the constant 0.2f (U_ |0.2 z|), the product and the sum (OP each); logistic:
            pointwise_reference._sigmoid_bound (v_exp_f32, v_rcp_f32); fast_tanh(x) = 1 - 2 rcp(1 + 2^(x c)), c = 2 log2 e:
              x c    the constant and the product, 3 U_ relative -> e = 2^(x c) moves by 2 |x| 3 U_, v_exp_f32 adds OP
              1 + e  OP of it;  v_rcp_f32  OP;  so r = 1 / (1 + e) is off by r (e r (6 |x| + 2) U_ + 2 OP)
              1 - 2r one fma, or a product and a difference: OP (2 r + |tanh x|)
            -- 2 r times the first plus the second: an ABSOLUTE 7 U_ at x = 0, where 1 - 2 r cancels.
            The backward's bounds run through dh_{t-1} = dz_t . U^T ((4H + 1) U_ sum |terms|) and the dc carry.
scale of U  uniform in +-U_SCALE / H with U_SCALE = 1.5: sum_k |U[k, j]| ~ 0.75, so the running forward bound grows by
            less than 0.75 per step even through tanh (Lipschitz 1) and stays a check at T = 33, and dz . U^T (4H terms,
            ~3 times the gate derivatives of at most 0.25) does not grow either.  With it the honest fp32 evaluation stays
            below 0.5 of every bound (tests/test_seq_reference.py, condition b).
"""
import zlib

import numpy as np

import pointwise_reference as P
from oracle import clvae_oracle as O

U_ = P.U
OP = P.OP
f32, f64 = np.float32, np.float64
A = np.abs
HARD, LOGISTIC = 0, 1                  # CLV_GATE_HARD_SIGMOID, CLV_GATE_SIGMOID
GATE_NAME = {HARD: 'hard_sigmoid', LOGISTIC: 'sigmoid'}
BLOCKS = ('z_i', 'z_f', 'g', 'z_o')
U_SCALE = 1.5
DEVICE_TIE = 'fma'                     # tests/test_gpu_seq.py::test_the_tie_at_minus_2p5 reads it off the device
ORDERS = P.ORDERS
VARIANTS = tuple((o, fma) for o in ORDERS for fma in (False, True))


def r64(a):
    return None if a is None else np.asarray(a, f32).astype(f64)


# ------------------------------------------------------------------------------------------------------------ checker --
def where(shape, i, H):
    """(row, step, gate, unit) of flat-per-shape index i: [B,T,4H] -> gate block and unit; [B,T,H], [B,H], [B,4H]"""
    i = tuple(int(x) for x in i)
    last = i[-1]
    wide = shape[-1] == 4 * H and H > 0
    gate, unit = (BLOCKS[last // H], last % H) if wide else ('-', last)
    return "(row %d, step %s, gate %s, unit %d)" % (i[0], i[1] if len(i) == 3 else '-', gate, unit)


def check(name, got, want, bound, H, flags=None):
    """every element of got within its bound of want (flagged ones must only be finite); returns the worst error / bound and
    raises with the first offending (row, step, gate, unit)"""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (name, got.shape, want.shape)
    bound = np.broadcast_to(np.asarray(bound, f64), want.shape)
    err = A(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isfinite(got), np.nan_to_num(ratio, nan=np.inf), np.inf)
    if flags is not None:
        ratio = np.where(np.broadcast_to(flags, want.shape) & np.isfinite(got), 0.0, ratio)
    bad = np.argwhere(ratio > 1.0)
    if bad.size:
        i = tuple(int(x) for x in bad[0])
        raise AssertionError("%s %s: got %.9g, expected %.9g, error %.3g = %.3g x its bound %.3g (%d of %d elements off)"
                             % (name, where(want.shape, i, H), got[i], want[i], err[i], ratio[i], bound[i], len(bad), want.size))
    return float(ratio.max()) if ratio.size else 0.0


def check_bits(name, got, want, H):
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (name, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    if bad.size:
        i = tuple(int(x) for x in bad[0])
        raise AssertionError("%s %s: got %r, expected %r bit for bit (%d of %d elements off)"
                             % (name, where(want.shape, i, H), got[i], want[i], len(bad), want.size))
    return 0.0


# ------------------------------------------------------------------------------------------------- elementwise stages --
def tanh_cost(x):
    """absolute error budget of fast_tanh(x): see the module's docstring"""
    e = np.exp(np.clip(2.0 * x, -700.0, 700.0))
    r = 1.0 / (1.0 + e)
    return 2 * r * (e * r * (6 * A(x) + 2) * U_ + 2 * OP) + OP * (2 * r + A(np.tanh(x)))


def gate(z, ez, gate_act):
    """gate value and its bound from a pre-activation and its bound"""
    if gate_act == HARD:
        lin = 0.2 * z
        return np.clip(lin + 0.5, 0.0, 1.0), 0.2 * ez + U_ * A(lin) + OP * (A(lin) + A(lin + 0.5))
    y = O.sigmoid(np.asarray(z, f64))
    return y, 0.25 * ez + P._sigmoid_bound(y, np.clip(z, -30.0, 30.0))


def hard_y32(z32, tie):
    """the float32 value 0.2f z + 0.5f, product and sum rounded separately or fused"""
    z32 = np.asarray(z32, f32)
    if tie == 'separate':
        return f32(0.2) * z32 + f32(0.5)
    assert tie == 'fma', tie
    return (f64(f32(0.2)) * z32.astype(f64) + 0.5).astype(f32)


def gate_grad(z32, y, ey, gate_act, tie):
    """derivative of the gate at the fp32 record z32, and its bound"""
    if gate_act == HARD:
        y32 = hard_y32(z32, tie)
        d = np.where((y32 >= 0) & (y32 <= 1), 0.2, 0.0)
        return d, U_ * d                       # the constant 0.2f
    d = y * (1 - y)
    return d, ey * A(1 - 2 * y) + OP * (A(1 - y) * y + d)


def tie_flags(z32):
    """where the two roundings of y decide the kink differently"""
    a, b = hard_y32(z32, 'separate'), hard_y32(z32, 'fma')
    return ((a >= 0) & (a <= 1)) != ((b >= 0) & (b <= 1))


# ------------------------------------------------------------------------------------------------------------ forward --
def _step(x, rb, Uw, hp, cp, ehp, ecp, gate_act):
    """one step in fp64 from (h, c) of the step before and their bounds; returns {name: (value, bound)}"""
    H = Uw.shape[0]
    aU = A(Uw)
    z = x + rb + hp @ Uw
    ez = (H + 3) * U_ * (A(x) + A(rb) + A(hp) @ aU) + ehp @ aU
    zs, es = [z[:, k * H:(k + 1) * H] for k in range(4)], [ez[:, k * H:(k + 1) * H] for k in range(4)]
    (i, ei), (f, ef), (o, eo) = (gate(zs[k], es[k], gate_act) for k in (0, 1, 3))
    g, eg = np.tanh(zs[2]), es[2] + tanh_cost(zs[2])
    c = f * cp + i * g
    ec = ef * A(cp) + f * ecp + ei * A(g) + i * eg + OP * (A(f * cp) + A(i * g) + A(c))
    tc = np.tanh(c)
    h = o * tc
    eh = eo * A(tc) + o * (ec + tanh_cost(c)) + OP * A(h)
    gates = np.concatenate([zs[0], zs[1], g, zs[3]], 1)
    egates = np.concatenate([es[0], es[1], eg, es[3]], 1)
    return dict(gates=(gates, egates), cs=(c, ec), hs=(h, eh))


def _parts(inp):
    x, Uw = r64(inp['xproj']), r64(inp['U'])
    B, T, G4 = x.shape
    H = G4 // 4
    rb = np.zeros((B, G4)) if inp.get('rowbias') is None else r64(inp['rowbias'])
    h0 = np.zeros((B, H)) if inp.get('h0') is None else r64(inp['h0'])
    c0 = np.zeros((B, H)) if inp.get('c0') is None else r64(inp['c0'])
    return x, rb, Uw, h0, c0, B, T, H


def forward_local(records, inp):
    """{gates, cs, hs: (want, bound)} of every step, each from the stored fp32 state of the step before"""
    x, rb, Uw, h0, c0, B, T, H = _parts(inp)
    hs, cs = r64(records['hs']), r64(records['cs'])
    hp = np.concatenate([h0[:, None], hs[:, :-1]], 1)[:, :T].reshape(B * T, H)
    cp = np.concatenate([c0[:, None], cs[:, :-1]], 1)[:, :T].reshape(B * T, H)
    zero = np.zeros((B * T, H))
    r = _step(x.reshape(B * T, 4 * H), np.repeat(rb, T, 0), Uw, hp, cp, zero, zero, inp['gate_act'])
    return {k: (v.reshape(B, T, v.shape[1]), e.reshape(B, T, v.shape[1])) for k, (v, e) in r.items()}


def forward_free(inp):
    """the oracle's LSTM end to end with running bounds; also hT, cT (T = 0: the initial state, exact)"""
    x, rb, Uw, h0, c0, B, T, H = _parts(inp)
    out = {k: (np.zeros((B, T, w)), np.zeros((B, T, w))) for k, w in (('gates', 4 * H), ('cs', H), ('hs', H))}
    h, c, eh, ec = h0, c0, np.zeros((B, H)), np.zeros((B, H))
    for t in range(T):
        r = _step(x[:, t], rb, Uw, h, c, eh, ec, inp['gate_act'])
        for k in r:
            out[k][0][:, t], out[k][1][:, t] = r[k]
        (h, eh), (c, ec) = r['hs'], r['cs']
    out['hT'], out['cT'] = (h, eh), (c, ec)
    return out


def judge_forward(name, inp, got):
    """every output of one forward call.  got: hs, and cs + gates of a saving call, hT / cT where the call asked for them,
    xproj_after where gates went to a buffer of their own.  Returns {output: worst error / bound}."""
    x, rb, Uw, h0, c0, B, T, H = _parts(inp)
    save = 'gates' in got
    free = forward_free(inp)
    rep = {}
    if save:
        local = forward_local(got, inp)
        for k in ('gates', 'cs', 'hs'):
            rep[k] = check(name + ' ' + k, got[k], *local[k], H)
            rep[k + ' (free)'] = check(name + ' ' + k + ' against the free recurrence', got[k], *free[k], H)
    else:
        assert 'cs' not in got
        rep['hs (free)'] = check(name + ' hs', got['hs'], *free['hs'], H)
    if 'hT' in got:
        rep['hT'] = check_bits(name + ' hT', got['hT'], got['hs'][:, T - 1] if T > 0 else h0, H)
    if 'cT' in got:
        if T == 0:
            rep['cT'] = check_bits(name + ' cT', got['cT'], c0, H)
        elif save:
            rep['cT'] = check_bits(name + ' cT', got['cT'], got['cs'][:, T - 1], H)
        else:
            rep['cT (free)'] = check(name + ' cT', got['cT'], *free['cT'], H)
    if 'xproj_after' in got:
        rep['xproj'] = check_bits(name + ' xproj (gates have a buffer of their own)', got['xproj_after'], inp['xproj'], H)
    return rep


# ----------------------------------------------------------------------------------------------------------- backward --
def backward(records, dhs, Uw, c0, gate_act, Kz=None, tie=None, sum_terms=True):
    """dz of every step from the fp32 records (gates, cs), with running bounds and the flags of the tie.
    sum_terms=False: U is a selection matrix, dz . U^T picks single entries and costs nothing (the selection probe)."""
    tie = tie or DEVICE_TIE
    z32 = np.asarray(records['gates'], f32)
    G, C, dH, Uw = r64(z32), r64(records['cs']), r64(dhs), r64(Uw)
    B, T, H = C.shape
    c0 = np.zeros((B, H)) if c0 is None else r64(c0)
    aUt = A(Uw).T
    dz, edz = np.zeros((B, T, 4 * H)), np.zeros((B, T, 4 * H))
    flags = np.zeros((B, T, 4 * H), bool)
    dhrec, edhrec, dc, edc = (np.zeros((B, H)) for _ in range(4))
    later = np.zeros(B, bool)                    # a flagged element in a later step reaches every earlier one of its row
    for t in range(T - 1, -1, -1):
        zi, zf, g, zo = (G[:, t, k * H:(k + 1) * H] for k in range(4))
        zi32, zf32, zo32 = (z32[:, t, k * H:(k + 1) * H] for k in (0, 1, 3))
        (i, ei), (f, ef), (o, eo) = (gate(v, 0.0, gate_act) for v in (zi, zf, zo))
        (gi, egi), (gf, egf), (go, ego) = (gate_grad(v32, y, ey, gate_act, tie)
                                          for v32, y, ey in ((zi32, i, ei), (zf32, f, ef), (zo32, o, eo)))
        cp = C[:, t - 1] if t > 0 else c0
        tc, etc = np.tanh(C[:, t]), tanh_cost(C[:, t])
        dh = dH[:, t] + dhrec
        edh = edhrec + OP * A(dh)
        kc = o * (1 - tc * tc)
        ekc = eo * A(1 - tc * tc) + o * (2 * A(tc) * etc + OP * (tc * tc + A(1 - tc * tc))) + OP * A(kc)
        dc = dc + dh * kc
        edc = edc + edh * A(kc) + A(dh) * ekc + OP * (A(dh * kc) + A(dc))
        ki, kf, kg, ko = g * gi, cp * gf, i * (1 - g * g), tc * go
        eki, ekf = A(g) * egi + OP * A(ki), A(cp) * egf + OP * A(kf)
        ekg = ei * A(1 - g * g) + i * OP * (g * g + A(1 - g * g)) + OP * A(kg)
        eko = etc * go + A(tc) * ego + OP * A(ko)
        dzt = np.concatenate([dc * ki, dc * kf, dc * kg, dh * ko], 1)
        # two products each, in either order: (dc g) gi or dc (g gi)
        edzt = np.concatenate([edc * A(ki) + A(dc) * eki, edc * A(kf) + A(dc) * ekf, edc * A(kg) + A(dc) * ekg,
                               edh * A(ko) + A(dh) * eko], 1) + 2 * OP * A(dzt)
        dz[:, t], edz[:, t] = dzt, edzt
        if gate_act == HARD:
            fl = np.concatenate([tie_flags(zi32), tie_flags(zf32), np.zeros((B, H), bool), tie_flags(zo32)], 1)
            flags[:, t] = fl | later[:, None]
            later = later | fl.any(1)
        edc = edc * f + A(dc) * ef + OP * A(dc * f)
        dc = dc * f
        dhrec = dzt @ Uw.T
        edhrec = edzt @ aUt + ((4 * H + 1) * U_ * (A(dzt) @ aUt) if sum_terms else 0.0)
    return dict(dz=(dz, edz, flags))


def dzsum_ref(dz_dev):
    """fp64 sum over the steps of the device's own dz; T + 1 for any order"""
    d = r64(dz_dev)
    return d.sum(1), (d.shape[1] + 1) * U_ * A(d).sum(1)


def dZ_ref(dz_dev, Kz):
    """dz_t . Kz^T of the device's own dz: 4H terms in any order"""
    d, K = r64(dz_dev), r64(Kz)
    return d @ K.T, (d.shape[2] + 1) * U_ * (A(d) @ A(K).T)


def judge_backward(name, records, dhs, Uw, c0, gate_act, got, Kz=None, tie=None, sum_terms=True):
    """got: dz, dzsum and, with Kz, dZ [B,T,nz].  Returns ({output: ratio}, flags of dz)."""
    H = np.asarray(Uw).shape[0]
    ref = backward(records, dhs, Uw, c0, gate_act, Kz, tie, sum_terms)
    rep = dict(dz=check(name + ' dz', got['dz'], *ref['dz'][:2], H, ref['dz'][2]))
    rep['dzsum'] = check(name + ' dzsum', got['dzsum'], *dzsum_ref(got['dz']), H)
    if Kz is not None:
        rep['dZ'] = check(name + ' dZ', got['dZ'], *dZ_ref(got['dz'], Kz), H)
    return rep, ref['dz'][2]


# ------------------------------------------------------------------------------------------- fp32 evaluation, faults --
def _mv32(extra, h, Uw, order, fma, keep=None):
    """sum(extra) + h . Uw in fp32, the terms taken in `order`; fma: a product is not rounded before it is added.
    keep [K]: 0 drops the term of that k (planted faults)"""
    h64, U64 = np.asarray(h, f32).astype(f64), np.asarray(Uw, f32).astype(f64)
    K = U64.shape[0]
    keep = np.ones(K) if keep is None else keep
    if order == 'pairwise':
        terms = np.concatenate([np.asarray(e, f64)[:, None, :] for e in extra] + [h64[:, :, None] * (U64 * keep[:, None])[None]], 1)
        if fma:                                  # a pair: one fused product-sum
            if terms.shape[1] % 2:
                terms = np.concatenate([terms, np.zeros_like(terms[:, :1])], 1)
            terms = terms[:, 0::2] + terms[:, 1::2]
        return P.sum32(terms.astype(f32), axis=1, order='pairwise')
    seq = [('e', e) for e in extra] + [('k', k) for k in range(K) if keep[k]]
    if order == 'reversed':
        seq.reverse()
    acc = np.zeros((h64.shape[0], U64.shape[1]), f32)
    for kind, v in seq:
        term = np.asarray(v, f64) if kind == 'e' else h64[:, v:v + 1] * U64[v]
        if kind == 'k' and not fma:
            term = term.astype(f32).astype(f64)
        acc = (acc.astype(f64) + term).astype(f32)
    return acc


def tanh32(x):
    """fast_tanh step by step in fp32: every operation correctly rounded"""
    x = np.asarray(x, f32)
    with np.errstate(over='ignore'):
        a = x * f32(2.885390082)
        e = np.exp2(a.astype(f64)).astype(f32)
        return f32(1) - f32(2) * (f32(1) / (e + f32(1)))


def gate32(z, gate_act, fma):
    z = np.asarray(z, f32)
    if gate_act == HARD:
        return np.clip(hard_y32(z, 'fma' if fma else 'separate'), f32(0), f32(1))
    return f32(1) / (f32(1) + P.exp32(-np.clip(z, f32(-30), f32(30))))


def _mad32(a, b, c, fma):
    """a b + c"""
    if fma:
        return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)
    return np.asarray(a, f32) * np.asarray(b, f32) + np.asarray(c, f32)


FWD_FAULTS = ('h_stale', 'k_lost', 'slice_lost', 'if_swapped', 'zc_stored', 'rowbias_neighbour', 'h0_ignored', 'c0_ignored',
              'hT_stale', 'cT_stale')
BWD_FAULTS = ('c0_ignored', 'f_wrong_step', 'no_1mg2', 'dzo_from_dc', 'slice_lost', 'dzsum_no_t0', 'kink_hi', 'kink_lo')
BWDZ_FAULTS = ('dZ_shift', 'dZ0_missing', 'Kz_leak')


def f32_forward(inp, order='forward', fma=False, fault=None, save=True):
    """the contract in fp32; returns hs, cs, gates, hT, cT (an inference call: drop what it does not store)"""
    assert fault is None or fault in FWD_FAULTS, fault
    x, Uw = np.asarray(inp['xproj'], f32), np.asarray(inp['U'], f32)
    B, T, G4 = x.shape
    H = G4 // 4
    gate_act = inp['gate_act']
    zero = np.zeros((B, H), f32)
    rb = np.zeros((B, G4), f32) if inp.get('rowbias') is None else np.asarray(inp['rowbias'], f32)
    h0 = zero if inp.get('h0') is None or fault == 'h0_ignored' else np.asarray(inp['h0'], f32)
    c0 = zero if inp.get('c0') is None or fault == 'c0_ignored' else np.asarray(inp['c0'], f32)
    if fault == 'rowbias_neighbour':
        rb = rb[np.arange(B) ^ 1 if B % 2 == 0 else np.arange(B)]
    keep = np.ones(H)
    if fault == 'k_lost':
        keep[H // 2] = 0
    if fault == 'slice_lost':
        keep[(H + 3) // 4:2 * ((H + 3) // 4)] = 0
    hs, cs, gates = np.zeros((B, T, H), f32), np.zeros((B, T, H), f32), np.zeros((B, T, G4), f32)
    h, c, hold = h0, c0, h0
    for t in range(T):
        hin = hold if fault == 'h_stale' else h
        z = _mv32([x[:, t], rb], hin, Uw, order, fma, keep)
        zi, zf, zc, zo = (z[:, k * H:(k + 1) * H] for k in range(4))
        if fault == 'if_swapped':
            zi, zf = zf, zi
        i, f, o = (gate32(v, gate_act, fma) for v in (zi, zf, zo))
        g = tanh32(zc)
        c = _mad32(f, c, i * g, fma)
        hold, h = h, o * tanh32(c)
        hs[:, t], cs[:, t] = h, c
        gates[:, t] = np.concatenate([zi, zf, zc if fault == 'zc_stored' else g, zo], 1)
    hT = h if T > 0 else np.asarray(inp['h0'], f32) if inp.get('h0') is not None else zero
    cT = c
    if fault == 'hT_stale':
        hT = hs[:, T - 2] if T > 1 else h0
    if fault == 'cT_stale':
        cT = cs[:, T - 2] if T > 1 else c0
    out = dict(hs=hs, hT=hT, cT=cT)
    if save:
        out.update(cs=cs, gates=gates)
    return out


def f32_backward(records, dhs, Uw, c0, gate_act, Kz=None, order='forward', fma=False, fault=None, tie=None):
    """BPTT in fp32 from the records; returns dz, dzsum and, with Kz, dZ [B,T,nz]"""
    assert fault is None or fault in BWD_FAULTS + BWDZ_FAULTS, fault
    tie = tie or DEVICE_TIE
    G, C, dH, Uw = (np.asarray(a, f32) for a in (records['gates'], records['cs'], dhs, Uw))
    B, T, H = C.shape
    c0 = np.zeros((B, H), f32) if c0 is None or fault == 'c0_ignored' else np.asarray(c0, f32)
    one = f32(1)

    def grad(z, y):
        if gate_act != HARD:
            return y * (one - y)
        y32 = hard_y32(z, tie)
        ok = (y32 >= 0) & (y32 <= 1)
        if fault == 'kink_hi':
            ok = ok | (z == np.nextafter(np.nextafter(f32(2.5), f32(9)), f32(9)))
        if fault == 'kink_lo':
            ok = ok | (z == np.nextafter(f32(-2.5), f32(-9)))
        return np.where(ok, f32(0.2), f32(0))

    dz = np.zeros((B, T, 4 * H), f32)
    dhrec, dc = np.zeros((B, H), f32), np.zeros((B, H), f32)
    keep = np.ones(4 * H)
    if fault == 'slice_lost':
        keep[22:44] = 0
    for t in range(T - 1, -1, -1):
        zi, zf, g, zo = (G[:, t, k * H:(k + 1) * H] for k in range(4))
        i, f, o = (gate32(v, gate_act, fma) for v in (zi, zf, zo))
        cp = C[:, t - 1] if t > 0 else c0
        tc = tanh32(C[:, t])
        dh = dH[:, t] + dhrec
        dc = _mad32(dh, o * (one - tc * tc), dc, fma)
        omg = one if fault == 'no_1mg2' else one - g * g
        dzt = np.concatenate([dc * (g * grad(zi, i)), dc * (cp * grad(zf, f)), dc * (i * omg),
                              (dc if fault == 'dzo_from_dc' else dh) * (tc * grad(zo, o))], 1)
        dz[:, t] = dzt
        fc = gate32(G[:, max(t - 1, 0), H:2 * H], gate_act, fma) if fault == 'f_wrong_step' else f
        dc = dc * fc
        dhrec = _mv32([], dzt, Uw.T, order, fma, keep)
    out = dict(dz=dz, dzsum=P.sum32(dz[:, 1:] if fault == 'dzsum_no_t0' else dz, axis=1, order=order))
    if Kz is not None:
        Kz = np.asarray(Kz, f32)
        nz = Kz.shape[0]
        dZ = _mv32([], dz.reshape(B * T, 4 * H), Kz.T, order, fma).reshape(B, T, nz)
        if fault == 'dZ_shift':
            dZ = np.concatenate([dZ[:, 1:], np.zeros((B, 1, nz), f32)], 1)
        if fault == 'dZ0_missing' and T > 0:
            dZ[:, 0] = 0
        if fault == 'Kz_leak':
            dZ[:, :, nz - 1] += _mv32([], dz.reshape(B * T, 4 * H), np.roll(Kz[:1], 1, 1).T, order, fma).reshape(B, T)
        out['dZ'] = dZ
    return out


# -------------------------------------------------------------------------------------------------- dispatch, mirrored --
def rows_per_wg(B):
    """lstm.hip: four rows for B > 512 and B % 4 == 0, else two for B > 256 and B even, else one"""
    return 4 if B > 512 and B % 4 == 0 else 2 if B > 256 and B % 2 == 0 else 1


def la_slices(H):
    """lstm_any.hip: k-slices per unit"""
    ks = 1
    while ks < 8 and 2 * ks * H <= 256:
        ks *= 2
    return ks


def la_units_per_thread(H):
    return (H + 255) // 256


def latent_group(nz):
    """lstm.hip backward: (latent groups in use, latents in the last one)"""
    return (nz + 3) // 4, (nz - 1) % 4 + 1


# -------------------------------------------------------------------------------------------------------- case tables --
# U is uniform in +-U_SCALE / H everywhere (see the module's docstring); xproj ~ N(0, 1.5) puts a fifth of the gates beyond
# the kinks, rowbias ~ N(0, 0.5), h0 uniform in +-1, c0 ~ N(0, 1), dhs ~ N(0, 1), Kz ~ N(0, 0.3).
B88 = (1, 3, 256, 257, 258, 513, 514, 516)
OPTIONS = (dict(rowbias=1, h0=1, c0=1, hT=1, cT=1, own=0, alias=0),
           dict(rowbias=0, h0=1, c0=0, hT=1, cT=1, own=1, alias=0),          # h0 without c0; gates in a buffer of their own
           dict(rowbias=1, h0=0, c0=0, hT=0, cT=0, own=0, alias=0),          # nothing optional
           dict(rowbias=0, h0=1, c0=1, hT=1, cT=0, own=1, alias=1),          # hT aliases h0
           dict(rowbias=1, h0=0, c0=1, hT=0, cT=1, own=0, alias=0))          # c0 without h0


def _fwd88_cases():
    cases, n = [], 0
    for B in B88:
        for gate_act in (HARD, LOGISTIC):
            for save in (1, 0):
                cases.append(dict(H=88, B=B, T=(1, 2, 3, 0, 4)[n % 5], gate_act=gate_act, save=save, **OPTIONS[(n // 2) % 5]))
                n += 1
    cases.append(dict(H=88, B=3, T=33, gate_act=HARD, save=1, **OPTIONS[0]))
    cases.append(dict(H=88, B=3, T=33, gate_act=LOGISTIC, save=0, **OPTIONS[1]))
    return cases


NZ = (1, 3, 4, 5, 8, 9, 32, 39, 40)


def _bwd88_cases():
    """each runs clv_lstm_seq_bwd and clv_lstm_seq_bwd_z on the records of a saving forward"""
    cases, n = [], 0
    for B in B88:
        for gate_act in (HARD, LOGISTIC):
            cases.append(dict(H=88, B=B, T=(2, 3, 1, 0, 4, 5)[n % 6], gate_act=gate_act, c0=n % 2, nz=NZ[n % 9],
                              pad=3 * ((n // 3) % 2), rowbias=1, h0=(n // 2) % 2))
            n += 1
    cases.append(dict(H=88, B=3, T=5, gate_act=HARD, c0=1, nz=39, pad=0, rowbias=0, h0=1))
    cases.append(dict(H=88, B=3, T=4, gate_act=LOGISTIC, c0=0, nz=40, pad=3, rowbias=0, h0=0))
    return cases


H_ANY = (1, 2, 7, 9, 31, 32, 33, 63, 64, 65, 87, 89, 127, 128, 129, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024)


def _any_cases():
    """lstm_any.hip: a saving forward and the backward on its records; force: 88 units through CLV_LSTM_ANY=1"""
    cases = [dict(H=H, B=2, T=(1, 2, 3, 0)[(n // 2) % 4], gate_act=n % 2, c0=(n // 2) % 2, h0=(n // 3) % 2, rowbias=n % 3 != 0,
                  hT=1, cT=1, force=0) for n, H in enumerate(H_ANY)]
    cases += [dict(H=88, B=2, T=3, gate_act=g, c0=1 - g, h0=g, rowbias=1, hT=1, cT=1, force=1) for g in (HARD, LOGISTIC)]
    cases += [dict(H=H, B=2, T=0, gate_act=g, c0=1, h0=1, rowbias=1, hT=1, cT=1, force=0) for H, g in ((7, HARD), (600, LOGISTIC))]
    return cases


# the stateful single step of the host sampling loops: T = 1, no cs / gates, the state in and out of the same buffers
STEP_CASES = tuple(dict(H=H, B=B, T=1, gate_act=g, rowbias=0, h0=1, c0=1, force=force)
                   for H, B, g, force in ((88, 1, HARD, 0), (88, 5, LOGISTIC, 0), (88, 3, HARD, 1), (7, 2, HARD, 0),
                                          (100, 2, LOGISTIC, 0), (600, 2, HARD, 0)))

# impulse probes: h0[b] = scale e_(b mod H), T = 1, xproj = 0, no rowbias
IMPULSE_88 = tuple(dict(H=88, B=B, gate_act=g) for B, g in ((88, HARD), (352, LOGISTIC), (528, HARD)))
IMPULSE_ANY = tuple(dict(H=H, B=H, gate_act=n % 2) for n, H in enumerate((7, 33, 100, 257, 600)))
IMPULSE_SCALES = (1.0, 2.0, -0.5)

# backward selection probe: U holds one 1.0 per row k, at column g H + perm[k]; T = 2
SELECT_BWD = tuple(dict(H=H, B=B, g=g, gate_act=(g + (H != 88)) % 2) for H, B in ((88, 2), (88, 258), (88, 516), (7, 2), (100, 2))
                   for g in range(4))
# bwd_z selection probe: Kz a 0/1 matrix, nz = 40, launch j takes the columns (40 j + l) mod 352
SELECT_Z = tuple(dict(H=88, B=B, T=T, j=j, gate_act=j % 2) for B, T in ((2, 1), (2, 3), (258, 3), (516, 1)) for j in range(9))

# crafted backward records
def ladder_points():
    """+-2.5 and +-2.5 +- {1, 2, 3} ulp without -2.5 itself (the tie case has it): 13 float32 values"""
    pts = []
    for base in (f32(2.5), f32(-2.5)):
        up, dn = base, base
        if base > 0:
            pts.append(base)
        for _ in range(3):
            up, dn = np.nextafter(up, f32(9)), np.nextafter(dn, f32(-9))
            pts += [up, dn]
    return np.array(pts, f32)


CRAFT_C = (0.0, 1.0, -1.0, 20.0, -20.0, 100.0, -100.0)
CRAFTED = tuple(dict(H=88, B=B, T=T, gate_act=g, c0=c0, dh0=dh0, force=force)
                for B, T, g, c0, dh0, force in
                [(2, T, g, c0, 0, 0) for T in (1, 2, 3) for g in (HARD, LOGISTIC) for c0 in (0, 1)]
                + [(258, 2, HARD, 1, 0, 0), (516, 3, HARD, 0, 0, 0), (2, 2, HARD, 1, 1, 0), (258, 2, LOGISTIC, 0, 1, 0),
                   (2, 3, HARD, 1, 0, 1), (2, 2, LOGISTIC, 0, 0, 1)])
# the tie: z = -2.5 in the blocks i, f, o; every lstm_bwd_kernel instance with a kink (R = 1, 2, 4, with and without latents)
# and lstm_any_bwd_kernel (force)
TIE_CASES = tuple(dict(H=88, B=B, T=1, gate_act=HARD, c0=1, dh0=0, force=force, tie=1)
                  for B, force in ((3, 0), (258, 0), (516, 0), (3, 1)))
TIE_UNITS = (0, 40, 87)

CASES = dict(fwd88=_fwd88_cases(), bwd88=_bwd88_cases(), any=_any_cases())


def _rng(tag, c):
    return np.random.default_rng(zlib.crc32(repr((tag, sorted(c.items()))).encode()))


def make_U(rng, H):
    return (rng.uniform(-1, 1, (H, 4 * H)) * U_SCALE / H).astype(f32)


KINK_CLEAR = 8 * 2.0 ** -22           # 8 ulp of 2.5
_INPUTS = {}


def near_kink(z):
    return A(A(np.asarray(z, f64)) - 2.5) <= KINK_CLEAR


def forward_inputs(c):
    """inputs of a forward case as fp32 arrays (None where the case has none), computed once per case and left unchanged.
    Where the fp32 evaluation's z_i, z_f or z_o lands within 8 ulp of +-2.5, xproj moves by 1e-3 there: no random case has a
    derivative that hangs on a few ulp, and only the tie case is ever flagged."""
    key = repr(sorted(c.items()))
    if key in _INPUTS:
        return _INPUTS[key]
    rng = _rng('fwd', c)
    H, B, T = c['H'], c['B'], c['T']
    inp = dict(gate_act=c['gate_act'], xproj=(1.5 * rng.standard_normal((B, T, 4 * H))).astype(f32), U=make_U(rng, H),
               rowbias=(0.5 * rng.standard_normal((B, 4 * H))).astype(f32) if c.get('rowbias') else None,
               h0=rng.uniform(-1, 1, (B, H)).astype(f32) if c.get('h0') else None,
               c0=rng.standard_normal((B, H)).astype(f32) if c.get('c0') else None)
    for _ in range(8):
        near = near_kink(f32_forward(inp)['gates'])
        near[:, :, 2 * H:3 * H] = False
        if not near.any():
            break
        inp['xproj'][near] += f32(1e-3)
    else:
        raise AssertionError("xproj still lands on a kink: %r" % (c,))
    _INPUTS[key] = inp
    return inp


def backward_inputs(c):
    """dhs and, with nz, Kz of a backward case"""
    rng = _rng('bwd', c)
    d = dict(dhs=rng.standard_normal((c['B'], c['T'], c['H'])).astype(f32))
    if c.get('nz'):
        d['Kz'] = (0.3 * rng.standard_normal((c['nz'], 4 * c['H']))).astype(f32)
    return d


def impulse_inputs(c, scale):
    H, B = c['H'], c['B']
    rng = _rng('impulse', c)
    h0 = np.zeros((B, H), f32)
    h0[np.arange(B), np.arange(B) % H] = scale
    return dict(gate_act=c['gate_act'], xproj=np.zeros((B, 1, 4 * H), f32), U=make_U(rng, H), rowbias=None, h0=h0, c0=None)


def judge_impulse(name, inp, got, scale):
    """z_i, z_f, z_o of row b are scale U[b mod H] bit for bit (a power of two times one entry plus zeros), g within the
    tanh cost of tanh(scale U)"""
    H, B = inp['U'].shape[0], inp['xproj'].shape[0]
    want = (f32(scale) * inp['U'][np.arange(B) % H])[:, None, :]
    z = np.asarray(got['gates'], f32)
    for k in (0, 1, 3):
        check_bits("%s %s" % (name, BLOCKS[k]), z[:, :, k * H:(k + 1) * H] + f32(0), want[:, :, k * H:(k + 1) * H] + f32(0), H)
    zc = want[:, :, 2 * H:3 * H].astype(f64)
    return dict(g=check(name + ' g', z[:, :, 2 * H:3 * H], np.tanh(zc), tanh_cost(zc), H))


def crafted_records(c):
    """(records, dhs, c0): gates and cs that no forward made.  Per (row, step): the 13 ladder points in the blocks i, f, o
    on the units 0..12 (the first lane group among them) and 75..87 (the last, unit 87), rotated with row + step; g = +-1
    at the units 20, 21; c through CRAFT_C at the units 30..36 (and so c_prev of the next step).  A tie case has z = -2.5
    at TIE_UNITS instead of the ladder; plain: random values only, clear of the kinks, any H."""
    rng = _rng('crafted', c)
    H, B, T = c['H'], c['B'], c['T']
    pts = ladder_points()
    gates = (1.5 * rng.standard_normal((B, T, 4 * H))).astype(f32)
    gates[:, :, 2 * H:3 * H] = np.tanh(gates[:, :, 2 * H:3 * H])
    for k in (0, 1, 3):
        blk = gates[:, :, k * H:(k + 1) * H]
        near = A(A(blk) - 2.5) < 1e-3                       # random values keep clear of the kinks
        blk[near] += f32(0.01)
        if c.get('plain'):
            continue
        if c.get('tie'):
            blk[:, :, list(TIE_UNITS)] = f32(-2.5)
            continue
        for b in range(min(B, 16)):
            for t in range(T):
                rot = (np.arange(13) + b + t + k) % 13
                blk[b, t, 0:13] = pts[rot]
                blk[b, t, 75:88] = pts[rot[::-1]]
    cs = rng.standard_normal((B, T, H)).astype(f32)
    if not c.get('plain'):
        gates[:, :, 2 * H + 20], gates[:, :, 2 * H + 21] = 1.0, -1.0
        cs[:, :, 30:37] = np.array(CRAFT_C, f32)
    dhs = np.zeros((B, T, H), f32) if c['dh0'] else rng.standard_normal((B, T, H)).astype(f32)
    c0 = rng.standard_normal((B, H)).astype(f32) if c['c0'] else None
    if c0 is not None and not c.get('plain'):
        c0[:, 30:37] = np.array(CRAFT_C[::-1], f32)
    return dict(gates=gates, cs=cs), dhs, c0


def select_bwd_inputs(c):
    """(records, dhs, U, perm): T = 2, random records clear of the kinks, U[k, g H + perm[k]] = 1"""
    rng = _rng('select', c)
    H, B = c['H'], c['B']
    rec, dhs, _ = crafted_records(dict(H=H, B=B, T=2, gate_act=c['gate_act'], c0=0, dh0=0, plain=1))
    perm = rng.permutation(H)
    Uw = np.zeros((H, 4 * H), f32)
    Uw[np.arange(H), c['g'] * H + perm] = 1.0
    return rec, dhs, Uw, perm


def select_z(c):
    """(Kz [40, 352], sel [40])"""
    sel = (40 * c['j'] + np.arange(40)) % 352
    Kz = np.zeros((40, 352), f32)
    Kz[np.arange(40), sel] = 1.0
    return Kz, sel


def outputs_of(c, rec):
    """what a call of case c stores, out of a full evaluation: no cs / gates from an inference call, hT / cT where asked"""
    keep = ['hs'] + (['cs', 'gates'] if c.get('save', 1) else []) + [k for k in ('hT', 'cT') if c.get(k, 1)]
    return {k: rec[k] for k in keep}


def sub_rows(B):
    """the rows of a large batch that the fp32 evaluation goes through (rows are independent): the first and last four"""
    return np.arange(B) if B <= 8 else np.r_[0:4, B - 4:B]


def take_rows(inp, rows):
    """the same inputs for a subset of the batch rows (rows are independent)"""
    return {k: (v[rows] if isinstance(v, np.ndarray) and k != 'U' else v) for k, v in inp.items()}
