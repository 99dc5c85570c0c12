"""Case tables and judges of the particle-filter and voice-count kernels (csrc/smc.hip, csrc/voices.hip; TEST ORACLE).

The arithmetic is that of smc_reference, gibbs_reference, smc_key_reference, voices_reference and oracle.philox; this file
adds the shapes and edges at which the kernels can go wrong, the bounds, and the invariants that need no tolerance.  A judge
takes the inputs of a case and what a kernel (or a model of it) returned as numpy arrays, returns {output: worst error /
bound} and raises AssertionError naming the first offending element.

Bounds.  u = 2^-53.  An fp64 exp / log of the device is taken to err by at most DEV_ULP ulps (2 DEV_ULP u relative), numpy's
by REF_ULP.  ell, logb: a sum of at most D logs of one sign, so rtol 1e-12 (the project's figure) leaves three orders over
(c + ceil(log2 D) + 1) u.  logW, logZ, ess: reweight_bound() below, from the operation counts of smc_reference.reweight with
the P-term sums in any order; both sides start every step from the same stored state, so their lw = logW + ell agree bit
for bit after step 0.  logZ adds lse to the stored sum: lse's bound and one rounding of |logZ| per side."""
import functools

import numpy as np

import gibbs_reference as GR
import smc_key_reference as KR
import smc_reference as SR
import voices_reference as VR
from helpers import FILL_U8

FREE = 255
U = 2.0 ** -53
DEV_ULP = 2.0           # the device's fp64 exp and log: OCML documents 1 ulp for both; twice that
REF_ULP = 1.0           # numpy's (glibc: below 1 ulp)
TINY = 2.0 ** -1074     # an underflowing exp errs by this much at most
SLACK = 1.01            # the second-order terms of every first-order bound below
BIG_M0 = 2 ** 35 + 7    # a first melody whose Philox counter has a non-zero high word
ELL_RTOL = 1e-12
I32_FILL = -7
ULP32 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------ comparing --
def _where(idx, axes):
    return ", ".join("%s %d" % (a, i) for a, i in zip(axes, idx)) if axes else str(tuple(int(i) for i in idx))


def check_bits(name, got, want, axes=None):
    """got == want bit for bit (want is cast to got's dtype first: a float64 reference frame of 0 / 1 is exact in any)"""
    got = np.ascontiguousarray(got)
    want = np.ascontiguousarray(np.asarray(want).astype(got.dtype))
    assert got.shape == want.shape, "%s: shape %s, want %s" % (name, got.shape, want.shape)
    bits = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = np.argwhere(got.view(bits) != want.view(bits))
    if len(bad):
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at (%s): got %r, want %r"
                             % (name, len(bad), got.size, _where(i, axes), got[i], want[i]))
    return 0.0


def check_close(name, got, want, bound, axes=None):
    """|got - want| <= bound element by element (a zero bound asks for equality); returns the worst ratio"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    assert got.shape == want.shape, "%s: shape %s, want %s" % (name, got.shape, want.shape)
    err = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.where(np.isfinite(got) & np.isfinite(want), ratio, np.inf)
    if ratio.size and not ratio.max() <= 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError("%s: error / bound %.3g at (%s): got %.17g, want %.17g, bound %.3g"
                             % (name, ratio[i], _where(i, axes), got[i], want[i], bound[i]))
    return float(ratio.max()) if ratio.size else 0.0


def check_ell(name, got, want, axes=('row',)):
    """rtol = 1e-12, atol = 0: a row without a forced note (and without a count) has exactly 0"""
    return check_close(name, got, want, ELL_RTOL * np.abs(want), axes)


def untouched(name, got, fill):
    got = np.asarray(got)
    bad = np.argwhere(~np.isnan(got)) if isinstance(fill, float) and np.isnan(fill) else np.argwhere(got != fill)
    assert not len(bad), "%s: %d elements written that should be untouched, first at %s" % (name, len(bad), tuple(bad[0]))


def _special(xhat, start, P):
    """voices_reference.SPECIAL into columns start .. of every row; a frame narrower than the list wraps it, one rotation
    per melody"""
    R, D = xhat.shape
    n = min(D, len(VR.SPECIAL))
    cols = (start + np.arange(n)) % D
    rot = (np.arange(R) // P)[:, None] if D < len(VR.SPECIAL) else 0
    xhat[:, cols] = VR.SPECIAL[(np.arange(n)[None] + rot) % len(VR.SPECIAL)]


CLIP_POINT = np.array([True] * 7 + [False])        # of SPECIAL: every value but 0.5 is at or beyond a clip point


# --------------------------------------------------------------------------------------------------------------- SAMPLE --
def _sample_table():
    out = []
    Ds, RPs = (1, 63, 64, 65, 88, 129, 200), ((1, 1), (3, 1), (4, 4), (5, 5), (66, 11), (1028, 4))
    for i, D in enumerate(Ds):
        for j, (R, P) in enumerate(RPs):
            out.append(dict(name="sample D=%d R=%d P=%d S=%d" % (D, R, P, 2 * ((i + j) % 2)), D=D, R=R, P=P,
                            S=2 * ((i + j) % 2), nsteps=3, seed=1000 * i + j, kind0=i + j))
    return out


SAMPLE = _sample_table()


@functools.lru_cache(maxsize=None)
def sample_inputs(i):
    """xhat, u [R, D] float32 and roll [G, nsteps, D]: melody g is all free, fully clamped, forced only at clip points, or
    mixed, in turn from the case's own start"""
    c = SAMPLE[i]
    rng = np.random.default_rng(c['seed'])
    R, D, P, nsteps = c['R'], c['D'], c['P'], c['nsteps']
    G = R // P
    xhat = rng.random((R, D)).astype(np.float32)
    _special(xhat, 0, P)
    if D >= 80:
        _special(xhat, D - 9, P)                      # and in the second round of the note loop
    u = rng.random((R, D)).astype(np.float32)
    roll = np.full((G, nsteps, D), FREE, np.uint8)
    n = min(D, 8)
    for g in range(G):
        kind = (g + c['kind0']) % 4
        if kind == 1:
            roll[g] = rng.random((nsteps, D)) < 0.5
        elif kind == 2:
            rot = g if D < 8 else 0
            cols = np.nonzero(CLIP_POINT[(np.arange(n) + rot) % 8])[0]
            roll[g][:, cols] = rng.integers(0, 2, (nsteps, len(cols)))
        elif kind == 3:
            r = rng.random((nsteps, D))
            roll[g] = np.where(r < 0.5, (r < 0.15).astype(np.uint8), np.uint8(FREE))
    for a in (xhat, u, roll):
        a.setflags(write=False)
    return dict(xhat=xhat, u=u, roll=roll)


def judge_sample(name, c, inp, k, got, increment=SR.increment):
    """got: x [R, D], ell [R], hist [nsteps, R, D] after one call at step S + k on poisoned outputs"""
    xhat, u = inp['xhat'], inp['u']
    if not 0 <= k < c['nsteps']:                      # no constraint, no weight, no history
        check_bits(name + " x (free step)", got['x'], (u <= xhat), ('row', 'note'))
        untouched(name + " ell", got['ell'], float('nan'))
        untouched(name + " hist", got['hist'], FILL_U8)
        return {}
    rows = np.repeat(inp['roll'][:, k], c['P'], axis=0)
    want = SR.sample_frame(xhat, u, rows)
    check_bits(name + " x", got['x'], want, ('row', 'note'))
    check_bits(name + " hist[k]", got['hist'][k], want, ('row', 'note'))
    untouched(name + " hist, other steps", np.delete(got['hist'], k, axis=0), FILL_U8)
    return {'ell': check_ell(name + " ell", got['ell'], increment(xhat, rows))}


def increment_log32(xhat, roll_rows):
    """MUTANT of smc_reference.increment: the logs taken in float32"""
    q = np.clip(np.asarray(xhat, np.float32), SR.CLIP_LO, SR.CLIP_HI)
    c = np.asarray(roll_rows)
    l1, l0 = np.log(q).astype(np.float64), np.log(np.float32(1) - q).astype(np.float64)
    return (np.where(c == 1, l1, 0.0) + np.where(c == 0, l0, 0.0)).sum(axis=-1)


# --------------------------------------------------------------------------------------------------------------- VOICES --
NOT_COUNTED = [(5, 3), (0, 16), (3, 200)]           # pairs that are not lo <= hi <= 15: the kernel treats them as free


def counted(pair):
    return int(pair[0]) <= int(pair[1]) <= VR.MAX_COUNT


def voices_pairs(D):
    ps = [p for p in VR.KERNEL_PAIRS if VR.is_free(p) or p[0] <= D]
    if D <= 15:
        ps.append((D, D))                             # every note on, through the b == 0 branch
    ps += [(0, 0), (min(D, 15), 15)] + NOT_COUNTED
    return ps


def _voices_table():
    out = []
    Ds, Rs = (1, 15, 16, 17, 63, 64, 65, 88, 96, 97, 127, 128), (1, 15, 16, 17, 67)
    many = {1: 1, 15: 5, 16: 4, 17: 17, 67: 67}
    for i, D in enumerate(Ds):
        for j, R in enumerate(Rs):
            P = many[R] if (i + j) % 2 else 1
            out.append(dict(name="voices D=%d R=%d P=%d" % (D, R, P), D=D, R=R, P=P, S=2 * ((i + j) % 2), nsteps=2,
                            with_roll=(i + 2 * j) % 3 != 0, seed=2000 + 100 * i + j))
    return out


VOICES = _voices_table()


@functools.lru_cache(maxsize=None)
def voices_inputs(i):
    """xhat, u [R, D], roll [G, nsteps, D] or None, voices [G, nsteps, 2]: the pairs of voices_pairs(D) in turn over
    (melody, step), so free and counted rows share a group of four rows; every counted frame is feasible"""
    c = VOICES[i]
    rng = np.random.default_rng(c['seed'])
    R, D, P, nsteps = c['R'], c['D'], c['P'], c['nsteps']
    G = R // P
    xhat = (1.0 / (1.0 + np.exp(-rng.normal(-2.5, 2.0, (R, D))))).astype(np.float32)
    _special(xhat, 20 % D, P)
    if D > 96:
        _special(xhat, D - 8, P)                      # in the upper mask word as well
    u = rng.random((R, D)).astype(np.float32)
    pairs = voices_pairs(D)
    voices = np.zeros((G, nsteps, 2), np.uint8)
    roll = np.full((G, nsteps, D), FREE, np.uint8) if c['with_roll'] else None
    for g in range(G):
        for k in range(nsteps):
            lo, hi = voices[g, k] = pairs[(g + k * 5 + i) % len(pairs)]
            if roll is None:
                continue
            if not counted((lo, hi)):
                n_on = int(rng.integers(0, min(D, 3) + 1))
                room = D - n_on
            else:
                n_on = int(rng.integers(0, min(hi, 3, D) + 1))
                room = D - max(int(lo), n_on)         # notes that may be forced off with lo still in reach
            idx = rng.permutation(D)
            roll[g, k, idx[:n_on]] = 1
            roll[g, k, idx[n_on:n_on + int(rng.integers(0, min(30, room) + 1))]] = 0
    for a in (xhat, u, voices) + (() if roll is None else (roll,)):
        a.setflags(write=False)
    return dict(xhat=xhat, u=u, roll=roll, voices=voices)


def voices_rows(c, inp, k):
    """(roll rows [R, D] or None, pairs [R, 2] with every not-counted pair replaced by the free one) of returned step k"""
    rows = None if inp['roll'] is None else np.repeat(inp['roll'][:, k], c['P'], axis=0)
    pairs = np.repeat(inp['voices'][:, k], c['P'], axis=0).astype(np.int64)
    free = ~np.array([counted(p) for p in pairs])
    pairs[free] = VR.FREE_PAIR
    return rows, pairs, free


def voices_feasible(c, inp):
    for g in range(inp['voices'].shape[0]):
        for k in range(c['nsteps']):
            lo, hi = (int(v) for v in inp['voices'][g, k])
            row = np.full(c['D'], FREE, np.uint8) if inp['roll'] is None else inp['roll'][g, k]
            if counted((lo, hi)) and not VR.feasible(row, lo, hi):
                return False
    return True


@functools.lru_cache(maxsize=None)
def voices_want(i, k):
    c, inp = VOICES[i], voices_inputs(i)
    rows, pairs, _ = voices_rows(c, inp, k)
    return VR.sample_frame(inp['xhat'], inp['u'], rows, pairs)          # x, ell, logb, margin


def judge_voices(name, c, inp, k, got, want=None):
    """got: x [R, D], logb [R] and, from the filter's kernel, ell [R], hist [nsteps, R, D]"""
    xhat, u = inp['xhat'], inp['u']
    smc = 'ell' in got
    if not 0 <= k < c['nsteps']:
        check_bits(name + " x (free step)", got['x'], (u <= xhat), ('row', 'note'))
        check_bits(name + " logb (free step)", got['logb'], np.zeros(c['R']), ('row',))
        if smc:
            untouched(name + " ell", got['ell'], float('nan'))
            untouched(name + " hist", got['hist'], FILL_U8)
        return {}
    x, ell, logb, margin = want or voices_want(VOICES.index(c), k)
    assert margin >= 1e-9, "%s: the table has a draw within %.3g of its threshold" % (name, margin)
    check_bits(name + " x", got['x'], x, ('row', 'note'))
    rep = {'logb': check_ell(name + " logb", got['logb'], logb)}
    if smc:
        check_bits(name + " hist[k]", got['hist'][k], x, ('row', 'note'))
        untouched(name + " hist, other steps", np.delete(got['hist'], k, axis=0), FILL_U8)
        rep['ell'] = check_ell(name + " ell", got['ell'], ell)
    return rep


def voices_bitmask_draw(p, u, lo, hi, roll_row=None, mutant=False):
    """A model of the kernel's two passes for one counted row: downwards, count lane c decides note j as if the walk stood at
    c and keeps the bit in mask word j >> 6 (the table is voices_reference.table's); upwards, the walk reads bit j & 31 of
    half (j >> 5) & 1 of that word in the lane of its count.  MUTANT: at note 96 the walk reads one bit further."""
    p, u = np.asarray(p, np.float32), np.asarray(u, np.float32).astype(np.float64)
    D = len(p)
    q = VR.recursion_q(p, roll_row)
    B = VR.table(q, lo, hi)
    masks = [[0, 0] for _ in range(hi + 1)]
    for j in range(D):
        forced = roll_row is not None and roll_row[j] <= 1
        for c in range(hi + 1):
            a, b = q[j] * B[j + 1, c + 1], (1.0 - q[j]) * B[j + 1, c]
            one = (roll_row[j] == 1) if forced else False if a == 0.0 else True if b == 0.0 else u[j] <= a / B[j, c]
            masks[c][j >> 6] |= int(one) << (j & 63)
    x, c = np.zeros(D), 0
    for j in range(D):
        m = masks[min(c, hi)][j >> 6]
        half = (m >> 32) if (j & 32) else (m & 0xFFFFFFFF)
        shift = (j & 31) + (1 if mutant and j == 96 else 0)
        x[j] = (half >> shift) & 1
        c += int(x[j])
    return x


# ------------------------------------------------------------------------------------------------------------- RESAMPLE --
TAUS, M0S = (0.0, 0.5, 1.0), (0, 5, BIG_M0)
SCRIPTS = ('random', 'uniform', 'dominant', 'spread', 'two_level')
RS_STEPS = 8


def _resample_table():
    """P x script, with tau, m0, S and G in turn.  The table keeps every ESS of the reference at least 1e-9 P from tau P,
    except on steps whose weights are exactly uniform (the `uniform` script, any script's all-equal steps, one particle):
    there the ESS is P to the last bit on both sides, which decides e < tau P at tau = 1 without a margin."""
    out = []
    for i, P in enumerate((1, 2, 3, 63, 64, 65, 100, 1023, 1024)):
        for j, script in enumerate(SCRIPTS):
            tau = TAUS[(i + j) % 3]
            if script == 'spread':
                tau = 0.0
            if script == 'two_level' and (tau == 0.5 or (i % 2 == 0 and tau == 0.0)):
                tau = 1.0          # an even split has an ESS of P / 2 to the last bit: never beside the threshold 0.5 P
            if script == 'dominant' and tau * P == 1.0:
                tau = 1.0          # one particle with all the weight has an ESS of exactly 1
            G = 2 if P >= 1023 else 1 + (i + j) % 5
            out.append(dict(G=G, P=P, tau=tau, m0=M0S[(i + 2 * j) % 3], S=3 * ((i + j) % 2), script=script))
    out.append(dict(G=300, P=5, tau=0.5, m0=5, S=3, script='random'))
    for n, c in enumerate(out):
        c.update(nsteps=RS_STEPS, seed=77 + n, rng=500 + n,
                 name="resample %(script)s P=%(P)d G=%(G)d tau=%(tau)g m0=%(m0)d S=%(S)d" % c)
    return out


RESAMPLE = _resample_table()


@functools.lru_cache(maxsize=None)
def resample_script(i):
    """ell [nsteps, G, P] of case i"""
    c = RESAMPLE[i]
    rng = np.random.default_rng(c['rng'])
    G, P, n = c['G'], c['P'], c['nsteps']
    ell = np.zeros((n, G, P))
    for k in range(n):
        if c['script'] == 'random':               # tests/test_gpu_smc.py's script
            ell[k] = -np.abs(rng.standard_normal((G, P))) * [0.0, 0.3, 3.0][k % 3] - rng.random((G, P)) * 2 * (k % 2)
        elif c['script'] == 'uniform':
            ell[k] = [0.0, -3.7, -3.7 * (np.arange(G)[:, None] + 1), 0.0][k % 4]
        elif c['script'] == 'dominant':
            if k % 4 != 3:                        # first, last, middle by melody; every fourth step adds nothing
                ell[k] = -800.0
                ell[k, np.arange(G), [(0, P - 1, P // 2)[m % 3] for m in range(G)]] = 0.0
        elif c['script'] == 'spread':
            ell[k] = -1400.0 * rng.random((G, P)) if k < 6 else 0.0
        else:                                     # two_level: the half at 0 alternates between the even and the first ones
            low = (np.arange(P) % 2 == 1) if k % 2 else (np.arange(P) >= (P + 1) // 2)
            ell[k] = np.where(low, -40.0, 0.0)[None] if k % 4 != 2 else 0.0
    ell.setflags(write=False)
    return ell


def filter_class(conditional):
    return GR.ConditionalFilter if conditional else SR.Filter


def reweight_bound(lw, first, ulps):
    """One side's error bounds of reweight on lw [G, P] = logW + ell: {lse [G], wn [G, P], ess [G], logP}.
    d = lw - M rounds once (u |d|), a = exp(d) carries that and the function's own error: relative rho = u |d| + 2 ulps u,
    plus TINY where it underflows.  s1 = sum a and s2 = sum a^2 in any order: (P - 1) u of the sum plus the terms' own.
    lse = M + log s1: ds1 / s1, the log's 2 ulps u log s1 (0 <= log s1 <= log P), one rounding.  wn = lw - lse: one more
    rounding of |wn| -- so the dominant particle's wn ~ -(s1 - 1) is bounded absolutely by lse's error.  ess = s1 s1 / s2:
    2 ds1 / s1 + ds2 / s2 + two roundings.  At the first step lw holds the side's own log P (2 ulps u log P) and its
    rounding (u |lw|); the shift is common to the row, so lse moves by the largest and wn by twice that."""
    G, P = lw.shape
    M = lw.max(axis=1, keepdims=True)
    d = lw - M
    a = np.exp(d)
    rho = U * np.abs(d) + 2 * ulps * U
    s1, s2 = a.sum(axis=1), (a * a).sum(axis=1)
    ds1 = (P - 1) * U * s1 + (rho * a).sum(axis=1) + P * TINY
    ds2 = (P - 1) * U * s2 + ((2 * rho + U) * a * a).sum(axis=1) + P * TINY
    lse = M[:, 0] + np.log(s1)
    logP = 2 * ulps * U * np.log(float(P))
    dlw = (logP + U * np.abs(lw)).max(axis=1) if first else np.zeros(G)
    dlse = ds1 / s1 + 2 * ulps * U * np.log(s1) + U * np.abs(lse) + dlw
    dwn = dlse[:, None] + U * np.abs(lw - lse[:, None]) + dlw[:, None]
    dess = (2 * ds1 / s1 + ds2 / s2 + 2 * U) * s1 * s1 / s2
    return dict(lse=SLACK * dlse, wn=SLACK * dwn, ess=SLACK * dess, logP=SLACK * logP)


def both_sides(lw, first):
    dev, ref = reweight_bound(lw, first, DEV_ULP), reweight_bound(lw, first, REF_ULP)
    return {k: dev[k] + ref[k] for k in dev}


def _offspring_check(name, P, grid, pts, counts, weights, skip_first):
    """counts [P] of one resampled melody against its reference grid = P * C (systematic) or C (conditional, where only
    'no weight, no offspring' applies)"""
    dead = weights == 0.0
    if skip_first:
        dead = dead.copy()
        dead[0] = False                               # the pinned particle keeps itself whatever it weighs
    bad = np.nonzero(dead & (counts > 0))[0]
    assert not len(bad), "%s: particle %d has exp(wn) = 0 and %d offspring" % (name, bad[0], counts[bad[0]])
    if pts is None:
        return
    w = 1e-9 * P
    lo_edge = np.concatenate([[-np.inf], grid[:-1]])
    hi_edge = np.concatenate([grid[:-1], [np.inf]])   # the last particle takes what is left
    least = ((pts[None] >= lo_edge[:, None] + w) & (pts[None] < hi_edge[:, None] - w)).sum(axis=1)
    most = ((pts[None] >= lo_edge[:, None] - w) & (pts[None] < hi_edge[:, None] + w)).sum(axis=1)
    bad = np.nonzero((counts < least) | (counts > most))[0]
    assert not len(bad), "%s: particle %d has %d offspring, the grid allows %d .. %d" % (name, bad[0], counts[bad[0]],
                                                                                        least[bad[0]], most[bad[0]])
    share = np.diff(np.concatenate([[0.0], grid]))
    bad = np.nonzero((counts < np.floor(share - 2 * w)) | (counts > np.ceil(share + 2 * w)))[0]
    assert not len(bad), "%s: particle %d has %d offspring for a share of %.17g" % (name, bad[0], counts[bad[0]], share[bad[0]])


def judge_resample(name, c, conditional, ell, steps):
    """steps[k]: logW [R], logZ [G], ess [G, nsteps], nres [G], flag [G], anc [nsteps, R] as they stand after step k; every
    step is judged from the state the step before left (the kernel's own), step 0 from nothing."""
    G, P, n, S, tau = c['G'], c['P'], c['nsteps'], c['S'], c['tau']
    ref = filter_class(conditional)(G, P, n, tau, c['seed'], c['m0'])
    rep = dict(logW=0.0, logZ=0.0, ess=0.0)
    base = (np.arange(G) * P)[:, None]
    running = np.zeros(G)
    for k, got in enumerate(steps):
        nm = "%s step %d" % (name, k)
        if k:
            prev = steps[k - 1]
            ref.logW, ref.logZ = prev['logW'].reshape(G, P).copy(), prev['logZ'].copy()
            ref.nres = prev['nres'].astype(np.int64)
        lw = ref.logW + ell[k]
        w_before = np.stack([SR.reweight(ref.logW[m], ell[k, m])[0] for m in range(G)])
        uniform = np.all(lw == lw[:, :1], axis=1)
        ref.step(ell[k].reshape(-1), S + k, k)
        assert not ref.near[k].any(), "%s: the table has a draw within 1e-9 of a cumulative weight" % nm
        res = ref.resampled[k]
        b = both_sides(lw, k == 0)
        check_bits(nm + " flag", got['flag'], res, ('melody',))
        check_bits(nm + " nres", got['nres'], ref.nres, ('melody',))
        check_bits(nm + " anc", got['anc'][k].reshape(G, P), ref.anc[k].reshape(G, P), ('melody', 'particle'))
        untouched(nm + " anc, later steps", got['anc'][k + 1:], I32_FILL)
        untouched(nm + " ess, later steps", got['ess'][:, k + 1:], float('nan'))
        rep['ess'] = max(rep['ess'], check_close(nm + " ess", got['ess'][:, k], ref.ess[:, k], b['ess'], ('melody',)))
        rep['logZ'] = max(rep['logZ'], check_close(nm + " logZ", got['logZ'], ref.logZ, b['lse'] + 2 * U * np.abs(ref.logZ),
                                                   ('melody',)))
        bw = np.where(res[:, None], b['logP'], b['wn'])
        rep['logW'] = max(rep['logW'], check_close(nm + " logW", got['logW'].reshape(G, P), ref.logW, bw,
                                                   ('melody', 'particle')))
        # ---- what needs no tolerance, on the kernel's own outputs
        anc = got['anc'][k].reshape(G, P).astype(np.int64) - base
        assert np.all((anc >= 0) & (anc < P)), "%s: an ancestor outside its melody's rows" % nm
        pts_all = None if conditional else SR.smc_uniforms(c['seed'], S + k, c['m0'], G)[:, None] + np.arange(P)[None]
        for m in np.nonzero(res)[0]:
            counts = np.bincount(anc[m], minlength=P)
            wm = np.exp(w_before[m])
            if conditional:
                assert anc[m, 0] == 0, "%s melody %d: the pinned particle took ancestor %d" % (nm, m, anc[m, 0])
                _offspring_check("%s melody %d" % (nm, m), P, np.cumsum(wm), None, counts, wm, True)
            else:
                assert np.all(np.diff(anc[m]) >= 0), "%s melody %d: systematic ancestors decrease" % (nm, m)
                _offspring_check("%s melody %d" % (nm, m), P, P * np.cumsum(wm), pts_all[m], counts, wm, False)
        if P == 1:
            running = running + ell[k, :, 0]
            check_bits(nm + " anc (P = 1)", got['anc'][k], np.arange(G), ('melody',))
            assert np.all(got['logW'] == 0.0), "%s: logW != 0 with one particle" % nm
            check_bits(nm + " logZ (P = 1: the running sum of ell)", got['logZ'], running, ('melody',))
        for m in np.nonzero(uniform)[0]:              # uniform weights: the ESS is P to the last bit, so nothing resamples
            assert got['ess'][m, k] == float(P) and got['flag'][m] == 0, \
                "%s melody %d: uniform weights, ess %.17g, flag %d" % (nm, m, got['ess'][m, k], got['flag'][m])
    return rep


def reference_run(c, conditional, ell):
    """the reference alone over the whole script: (filter, |ess - tau P| / P per step and melody, uniform steps)"""
    G, P, n = c['G'], c['P'], c['nsteps']
    ref = filter_class(conditional)(G, P, n, c['tau'], c['seed'], c['m0'])
    uniform = np.zeros((n, G), bool)
    for k in range(n):
        lw = ref.logW + ell[k]
        uniform[k] = np.all(lw == lw[:, :1], axis=1)
        ref.step(ell[k].reshape(-1), c['S'] + k, k)
    return ref, np.abs(ref.ess.T - c['tau'] * P) / P, uniform


# a model of smc_resample_kernel that sums in the kernel's order: the butterfly within a wave of 64, then the waves in turn
def _butterfly(v, op):
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = op(v, v[..., lane ^ o])
    return v[..., 0]


def _block(v, fill, op, start):
    G, P = v.shape
    nw = (P + 63) // 64
    pad = np.full((G, nw * 64), fill)
    pad[:, :P] = v
    red = _butterfly(pad.reshape(G, nw, 64), op)
    s = red[:, 0] if start is None else start + red[:, 0]
    for i in range(1, nw):
        s = op(s, red[:, i])
    return s


def _block_scan(v):
    """block_inclusive_scan: the shifted adds within a wave, then the wave totals in turn"""
    G, P = v.shape
    nw = (P + 63) // 64
    pad = np.zeros((G, nw, 64))
    pad.reshape(G, -1)[:, :P] = v
    lane = np.arange(64)
    for o in (1, 2, 4, 8, 16, 32):
        t = np.concatenate([np.zeros((G, nw, o)), pad[..., :-o]], axis=-1)
        pad = np.where(lane >= o, pad + t, pad)
    cum = np.zeros((G, nw, 64))
    base = np.zeros(G)
    for w in range(nw):
        cum[:, w] = base[:, None] + pad[:, w]
        base = base + pad[:, w, 63]
    return cum.reshape(G, -1)[:, :P]


def _pick(cum, n, x, strict=True):
    """systematic_pick's bisection for every x [G, K] on cum [G, P].  MUTANT strict=False: >= in place of >"""
    G, P = cum.shape
    lo, hi = np.zeros(x.shape, np.int64), np.full(x.shape, P - 1, np.int64)
    while np.any(lo < hi):
        mid = (lo + hi) >> 1
        v = n * np.take_along_axis(cum, mid, axis=1)
        right = (v > x) if strict else (v >= x)
        go = lo < hi
        hi = np.where(go & right, mid, hi)
        lo = np.where(go & ~right, mid + 1, lo)
    return lo


def exp32(x):
    """MUTANT: an exp taken in float32"""
    with np.errstate(over='ignore', under='ignore'):
        return np.exp(np.asarray(x, np.float32)).astype(np.float64)


def model_resample(c, conditional, ell, exp=np.exp, strict=True):
    """what the kernel would store after each step, in its own order of operations -> the `steps` of judge_resample"""
    G, P, n, S, tau, seed, m0 = c['G'], c['P'], c['nsteps'], c['S'], c['tau'], c['seed'], c['m0']
    logP = np.log(float(P))
    logW, logZ, nres = np.full((G, P), np.nan), np.full(G, np.nan), np.full(G, -5)
    ess, anc = np.full((G, n), np.nan), np.full((n, G * P), I32_FILL, np.int32)
    base = (np.arange(G) * P)[:, None]
    steps = []
    for k in range(n):
        lw = (np.full((G, P), -logP) if k == 0 else logW) + ell[k]
        M = _block(lw, -np.inf, np.fmax, None)
        a = exp(lw - M[:, None])
        s1, s2 = _block(a, 0.0, np.add, 0.0), _block(a * a, 0.0, np.add, 0.0)
        lse = M + np.log(s1)
        wn = lw - lse[:, None]
        e = s1 * s1 / s2
        res = e < tau * P
        cum = _block_scan(exp(wn))
        if conditional:
            pick = _pick(cum, 1.0, GR.gibbs_uniforms(seed, S + k, m0, G, P), strict)
            pick[:, 0] = 0
        else:
            pick = _pick(cum, float(P), SR.smc_uniforms(seed, S + k, m0, G)[:, None] + np.arange(P)[None], strict)
        anc[k] = (base + np.where(res[:, None], pick, np.arange(P)[None])).reshape(-1)
        logW = np.where(res[:, None], -logP, wn)
        logZ = (0.0 if k == 0 else logZ) + lse
        ess[:, k] = e
        nres = (0 if k == 0 else nres) + res
        steps.append(dict(logW=logW.reshape(-1).copy(), logZ=logZ.copy(), ess=ess.copy(), nres=nres.astype(np.int32),
                          flag=res.astype(np.int32), anc=anc.copy()))
    return steps


def tie_case():
    """(logW [2], u0, seed, step): two particles whose first grid point 2 * exp(logW[0]) IS the first draw point u0, found
    by stepping logW[0] through its neighbours -- the one input on which > and >= part (never part of a device table)"""
    seed = 4242
    for step in range(64):
        u0 = float(SR.smc_uniforms(seed, step, 0, 1)[0])
        lw = np.log(u0 / 2)
        for _ in range(8):
            lw = np.nextafter(lw, -np.inf)
        for _ in range(17):
            if 2 * np.exp(lw) == u0:
                return np.array([lw, np.log1p(-np.exp(lw))]), u0, seed, step
            lw = np.nextafter(lw, np.inf)
    raise AssertionError("no exact tie found")


# --------------------------------------------------------------------------------------------------------------- GATHER --
WIDTHS = (1, 63, 64, 65, 7, 88, 352)
NAN_BITS = np.array([0x7FC00000, 0x7FC00001, 0xFFFFFFFF, 0x7F800001, 0xFF800001, 0x7FA5A5A5], np.uint32)


def _gather_table():
    out = []
    for i, nbuf in enumerate((1, 3, 8)):
        for j, (R, P) in enumerate(((1, 1), (30, 6), (30, 1), (67, 67))):
            out.append(dict(name="gather nbuf=%d R=%d P=%d flags=%s" % (nbuf, R, P, ('none', 'all', 'mixed')[(i + j) % 3]),
                            nbuf=nbuf, R=R, P=P, flags=(i + j) % 3, widths=[WIDTHS[(j + 3 * i + b) % 7] for b in range(nbuf)],
                            nsteps=4, S=1, k=2, seed=3000 + 10 * i + j))
    return out


GATHER = _gather_table()


def ancestor_maps(rng, G, P, start=0):
    """[G * P] rows: per melody a cycle, fixed points, everything onto one particle, a random many-to-one map, in turn"""
    out = np.zeros((G, P), np.int64)
    for m in range(G):
        kind = (m + start) % 4
        out[m] = [(np.arange(P) + 1) % P, np.arange(P), np.full(P, int(rng.integers(0, P))), rng.integers(0, P, P)][kind]
    return (out + (np.arange(G) * P)[:, None]).reshape(-1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def gather_inputs(i):
    c = GATHER[i]
    rng = np.random.default_rng(c['seed'])
    R, P, G = c['R'], c['P'], c['R'] // c['P']
    bufs = []
    for w in c['widths']:
        bits = rng.integers(0, 2 ** 32, (R, w), dtype=np.uint64).astype(np.uint32)
        hit = rng.random((R, w)) < 0.2
        bits[hit] = NAN_BITS[rng.integers(0, len(NAN_BITS), int(hit.sum()))]
        bits.reshape(-1)[0] = NAN_BITS[3]
        bufs.append(bits)
    anc = np.stack([ancestor_maps(rng, G, P, s) for s in range(c['nsteps'])])      # the other steps hold other maps
    flag = [np.zeros(G), np.ones(G), np.arange(G) % 2 == 0][c['flags']].astype(np.int32)
    return dict(bufs=bufs, anc=anc, flag=flag)


def judge_gather(name, c, inp, k, got):
    """got: the buffers as uint32 bits after one call at step S + k"""
    moved = np.repeat(inp['flag'], c['P']).astype(bool) & (0 <= k < c['nsteps'])
    for b, (g, o) in enumerate(zip(got, inp['bufs'])):
        src = inp['anc'][min(max(k, 0), c['nsteps'] - 1)]
        check_bits("%s buffer %d (width %d)" % (name, b, o.shape[1]), g, np.where(moved[:, None], o[src], o), ('row', 'column'))
    return {}


# ------------------------------------------------------------------------------------------------------------ BACKTRACK --
def _backtrack_table():
    out = []
    Ds = (1, 65, 88, 200)
    for i, (P, n_out) in enumerate(((1, 1), (1, 5), (5, 64), (64, 64), (200, 9), (1024, 3), (70, 40))):
        for j, lineage in enumerate(('filter', 'random')):
            D = Ds[(i + 2 * j) % 4]
            out.append(dict(name="backtrack P=%d n_out=%d D=%d %s picks=%s" % (P, n_out, D, lineage, (i + j) % 2 == 0),
                            P=P, n_out=n_out, D=D, lineage=lineage, picks=(i + j) % 2 == 0, G=2 if P == 1024 else 4,
                            nsteps=6, seed=123 + i, m0=(0, 9, BIG_M0)[(i + j) % 3], step=50, rng=4000 + 10 * i + j))
    return out


BACKTRACK = _backtrack_table()


def two_level(k, P):
    low = (np.arange(P) % 2 == 1) if k % 2 else (np.arange(P) >= (P + 1) // 2)
    return np.where(low, -40.0, 0.0)


@functools.lru_cache(maxsize=None)
def backtrack_inputs(i):
    c = BACKTRACK[i]
    rng = np.random.default_rng(c['rng'])
    G, P, n, D = c['G'], c['P'], c['nsteps'], c['D']
    R = G * P
    if c['lineage'] == 'filter':                      # real lineages: every step resamples, the paths coalesce
        f = SR.Filter(G, P, n, 1.0, c['seed'] + 1, c['m0'])
        for k in range(n):
            f.step(np.tile(two_level(k, P), G) - 0.1 * rng.random(R), k, k)
        assert not f.near.any()
        anc, lw = f.anc.astype(np.int32), f.logW.copy()
        lw = lw - 1.5 * rng.random((G, P))            # the weights after one more frame without a resample
        lw -= np.log(np.exp(lw).sum(axis=1, keepdims=True))
    else:
        lw = rng.standard_normal((G, P)) * 1.5
        lw -= np.log(np.exp(lw).sum(axis=1, keepdims=True))
        anc = (np.arange(R)[None] // P * P + rng.integers(0, P, (n, R))).astype(np.int32)
    hist = (rng.random((n, R, D)) < 0.3).astype(np.uint8)
    return dict(logW=lw, anc=anc, hist=hist)


def backtrack_near(c, inp):
    """a draw point within 1e-9 n_out of a grid point of the final weights"""
    u = SR.smc_uniforms(c['seed'], c['step'], c['m0'], c['G'])
    for m in range(c['G']):
        _, grid = SR.systematic(inp['logW'][m], c['n_out'], u[m])
        pts = u[m] + np.arange(c['n_out'])
        if np.abs(grid[None, :-1] - pts[:, None]).min(initial=np.inf) < 1e-9 * c['n_out']:
            return True
    return False


def judge_backtrack(name, c, inp, got):
    want, picks = SR.backtrack(inp['logW'], inp['anc'], inp['hist'], c['n_out'], c['seed'], c['step'], c['m0'])
    if got.get('picks') is not None:
        check_bits(name + " picks", got['picks'], picks, ('melody', 'output'))
    check_bits(name + " Xs", got['Xs'], want, ('melody', 'output', 'step', 'note'))
    return {}


# ------------------------------------------------------------------------------------------------- PATH, PIN and TAKE_W --
def _shape_table(kind, shapes):
    return [dict(name="%s G=%d P=%d S=%d L=%d D=%d" % ((kind,) + s), G=s[0], P=s[1], S=s[2], L=s[3], D=s[4], nsteps=5,
                 rng=5000 + i) for i, s in enumerate(shapes)]


# (G, P, S, L, D)
PATH = _shape_table("path", [(6, 1, 0, 3, 88), (6, 5, 2, 3, 88), (6, 70, 1, 3, 88), (6, 5, 0, 3, 88), (1, 5, 2, 1, 1),
                             (4, 5, 0, 65, 65), (5, 70, 2, 3, 65), (5, 3, 1, 65, 1), (4, 1, 3, 1, 88)])
PIN = _shape_table("pin", [(3, 1, 0, 3, 88), (3, 5, 0, 3, 88), (3, 1, 2, 3, 88), (3, 5, 2, 3, 88), (1, 5, 2, 1, 1),
                           (4, 3, 0, 65, 65), (5, 2, 1, 3, 65), (5, 1, 3, 65, 1), (4, 70, 2, 1, 88)])
for _c in PIN:
    _c['nsteps'] = 4


def clamp_picks(picks, P):
    """min(max(pick, 0), P - 1), as smc_backtrack_path_kernel and smc_take_w_kernel read their picks"""
    return np.clip(np.asarray(picks, np.int64), 0, P - 1)


def clamp_anc(anc, P):
    """every entry into the rows of the melody that owns the row it stands in (a walk never leaves its melody's rows, so
    this is the clamp smc_backtrack_path_kernel applies as it goes)"""
    anc = np.asarray(anc, np.int64)
    first = np.arange(anc.shape[-1]) // P * P
    return np.clip(anc, first, first + P - 1)


@functools.lru_cache(maxsize=None)
def path_inputs(i):
    c = PATH[i]
    rng = np.random.default_rng(c['rng'])
    G, P, S, L, D, n = c['G'], c['P'], c['S'], c['L'], c['D'], c['nsteps']
    R, T = G * P, S + n
    anc = (np.arange(R)[None] // P * P + rng.integers(0, P, (n, R))).astype(np.int32)
    anc[:, 0] = 0                                     # melody 0's pinned row keeps itself, and is picked below
    picks = rng.integers(0, P, G).astype(np.int32)
    picks[0] = 0
    if G > 1:
        picks[1] = -1                                 # read as 0
    if G > 2:
        picks[2] = P + 3                              # read as P - 1
    m = G - 1                                         # the last step of the last melody's walk points outside its rows
    start = m * P + int(clamp_picks(picks, P)[m])
    if m > 0:
        anc[n - 1, start] = (m - 1) * P + P // 2      # into the melody before: read as its own first row
    if i % 2 == 0 and G > 3:
        anc[n - 1, 3 * P + int(picks[3])] = R + 5     # beyond every row: read as melody 3's last row
    return dict(picks=picks, anc=anc, hist=(rng.random((n, R, D)) < 0.3).astype(np.uint8),
                zhist=rng.standard_normal((T, R, L)).astype(np.float32), brows=(rng.random((R, D)) < 0.3).astype(np.float32))


def judge_path(name, c, inp, got):
    S, P = c['S'], c['P']
    wx, wz, wb, wr = GR.backtrack_path(clamp_picks(inp['picks'], P), clamp_anc(inp['anc'], P), inp['hist'], inp['zhist'],
                                       inp['brows'] if S else None, P, S)
    check_bits(name + " x_ref", got['x_ref'], wx, ('melody', 'step', 'note'))
    check_bits(name + " z_ref", got['z_ref'], wz, ('melody', 'step', 'latent'))
    check_bits(name + " renewed", got['renewed'], wr, ('melody', 'step'))
    if S:
        check_bits(name + " bridge_ref", got['bridge_ref'], wb, ('melody', 'note'))
    assert not wr[0].any()
    return {}


@functools.lru_cache(maxsize=None)
def pin_inputs(i):
    c = PIN[i]
    rng = np.random.default_rng(c['rng'])
    G, P, S, L, D, n = c['G'], c['P'], c['S'], c['L'], c['D'], c['nsteps']
    R, T = G * P, S + n
    return dict(z_ref=rng.standard_normal((G, T, L)).astype(np.float32), x_ref=(rng.random((G, n, D)) < 0.4).astype(np.uint8),
                bridge=(rng.random((G, D)) < 0.4).astype(np.float32), z0=rng.standard_normal((R, L)).astype(np.float32),
                x0=(rng.random((R, D)) < 0.4).astype(np.float32), h0=np.full((n, R, D), 7, np.uint8))


def judge_pin(name, c, inp, step, with_bridge, got):
    """got: z [R, L], x [R, D], hist [nsteps, R, D] after both pins at chain step `step`"""
    S, P = c['S'], c['P']
    check_bits(name + " z", got['z'], GR.pin_z(inp['z0'], inp['z_ref'], step, P), ('row', 'latent'))
    wx, wh = GR.pin_frame(inp['x0'], inp['h0'], inp['x_ref'], inp['bridge'] if with_bridge else None, step, S, P)
    check_bits(name + " x", got['x'], wx, ('row', 'note'))
    check_bits(name + " hist", got['hist'], wh, ('step', 'row', 'note'))
    return {}


# (P, C, n_out, G)
TAKE_W = [dict(name="take_w P=%d C=%d n_out=%d G=%d" % s, P=s[0], C=s[1], n_out=s[2], G=s[3], rng=6000 + i)
          for i, s in enumerate([(1, 2, 1, 6), (5, 10, 3, 6), (64, 25, 64, 6), (1024, 10, 9, 6), (5, 32, 3, 1), (3, 2, 7, 4),
                                 (65, 32, 2, 5)])]


@functools.lru_cache(maxsize=None)
def take_w_inputs(i):
    c = TAKE_W[i]
    rng = np.random.default_rng(c['rng'])
    picks = rng.integers(0, c['P'], (c['G'], c['n_out'])).astype(np.int32)
    picks[0, 0], picks[-1, -1] = 0, c['P'] - 1
    if picks.size > 3:
        picks.reshape(-1)[1], picks.reshape(-1)[2] = -1, c['P'] + 3
    return dict(picks=picks, wr=rng.standard_normal((c['G'] * c['P'], c['C'])).astype(np.float32))


def judge_take_w(name, c, inp, got):
    check_bits(name, got['w_out'], KR.take_w(inp['wr'], clamp_picks(inp['picks'], c['P']), c['P']), ('melody', 'output', 'class'))
    return {}


# ------------------------------------------------------------------------------------------------- INIT_W and POSTERIOR --
INIT_W = ([dict(name="init_w categorical P=%d C=%d m0=%d" % (P, C, m0), mode=0, P=P, C=C, G=7, seed=1234567890123, m0=m0,
                rng=100 * C + P)
           for i, P in enumerate((1, 63, 64, 65, 1024)) for j, C in enumerate((2, 10, 25, 32))
           for m0 in [(11, BIG_M0)[(i + j) % 2]]] +
          [dict(name="init_w logistic-normal P=%d C=%d m0=%d" % (P, C, m0), mode=1, P=P, C=C, G=5, seed=99, m0=m0, rng=P + C)
           for P, C, m0 in ((1, 2, 3), (63, 10, 3), (64, 25, BIG_M0), (65, 10, 3), (1024, 10, BIG_M0), (200, 32, 3),
                            (5, 2, BIG_M0), (3, 32, BIG_M0))])
LOGISTIC_NORMAL_ULPS = 16       # of 1.0 in float32: the derivation stands in tests/test_gpu_smc_key.py


def key_probs(rng, G, C):
    """test_gpu_smc_key._probs: skewed rows with zeros; row 0 one-hot in the middle, row 1 all mass in the last class"""
    p = rng.dirichlet(np.full(C, 0.3), G)
    p[rng.random((G, C)) < 0.3] = 0.0
    p[:, 0] += (p.sum(axis=1) == 0)
    p /= p.sum(axis=1, keepdims=True)
    p[0], p[1] = np.eye(C)[C // 2], np.eye(C)[C - 1]
    p[2] = np.eye(C)[0] * 0.5 + np.eye(C)[C - 1] * 0.5
    return p


@functools.lru_cache(maxsize=None)
def init_w_inputs(i):
    c = INIT_W[i]
    rng = np.random.default_rng(c['rng'])
    G, C = c['G'], c['C']
    if c['mode'] == 0:
        return dict(probs=key_probs(rng, G, C))
    mean = rng.uniform(-1, 1, (G, C - 1)).astype(np.float32)
    lv = rng.uniform(-3, 0, (G, C - 1)).astype(np.float32)
    mean[0], lv[0] = 0.0, 0.0
    return dict(mean=mean, log_var=lv)


def init_w_near(c, inp):
    """categorical: a draw point within 1e-9 P of a grid point P * cum below the last"""
    u = KR.key_uniforms(c['seed'], c['m0'], c['G'])
    for m in range(c['G']):
        _, grid = KR.allocate_keys(inp['probs'][m], c['P'], u[m])
        pts = u[m] + np.arange(c['P'])
        if np.abs(grid[None, :-1] - pts[:, None]).min(initial=np.inf) < 1e-9 * c['P']:
            return True
    return False


def judge_init_w(name, c, inp, got):
    P, C = c['P'], c['C']
    if c['mode'] == 0:
        want, keys = KR.init_categorical(inp['probs'], P, c['seed'], c['m0'])
        check_bits(name, got['wr'], want, ('row', 'class'))
        counts = np.stack([np.bincount(k, minlength=C) for k in keys])
        assert np.all(counts[inp['probs'] == 0] == 0) and np.all(np.abs(counts - P * inp['probs']) < 1 + 1e-9)
        return {}
    want = KR.init_logistic_normal(inp['mean'], inp['log_var'], P, c['seed'], c['m0'])
    rep = {'logistic-normal w': check_close(name, got['wr'], want, LOGISTIC_NORMAL_ULPS * ULP32, ('row', 'class'))}
    assert np.abs(np.asarray(got['wr'], np.float64).sum(axis=1) - 1).max() <= 4 * ULP32 * np.sqrt(C), name + ": a row's sum"
    return rep


POSTERIOR = [dict(name="posterior P=%d C=%d" % s, P=s[0], C=s[1], G=4, nsteps=5, S=2, rng=7 * s[0] + s[1])
             for s in [(1, 2), (5, 10), (64, 25), (100, 10), (1024, 10), (1000, 32), (65, 32), (3, 2)]]
POSTERIOR_RTOL = 1e-12          # tests/test_gpu_smc_key.py's: a sum of P non-negative products


@functools.lru_cache(maxsize=None)
def posterior_inputs(i):
    c = POSTERIOR[i]
    rng = np.random.default_rng(c['rng'])
    G, P, C = c['G'], c['P'], c['C']
    lw = rng.standard_normal((G, P)) * 3
    lw -= np.log(np.exp(lw).sum(axis=1, keepdims=True))
    wr = rng.dirichlet(np.ones(C), G * P).astype(np.float32)
    wr[:P] = np.eye(C, dtype=np.float32)[rng.integers(0, C, P)]          # melody 0: one-hot rows
    return dict(logW=lw, wr=wr)


def judge_posterior(name, c, inp, written, got):
    """got: out [G, nsteps, C] (-7 where no step wrote) after calls at the returned steps `written`"""
    want = KR.w_posterior(inp['logW'], inp['wr'])
    other = np.ones(c['nsteps'], bool)
    other[list(written)] = False
    untouched(name + " other steps", got['out'][:, other], -7.0)
    worst = 0.0
    for k in written:
        worst = max(worst, check_close("%s step %d" % (name, k), got['out'][:, k], want, POSTERIOR_RTOL * np.abs(want),
                                       ('melody', 'class')))
    return {'w_posterior': worst}
