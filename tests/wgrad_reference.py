"""fp64 reference of the LSTM kernel-gradient product (include/clvae.h: clv_lstm_wgrad, clv_lstm_wgrad_pair), a bound per
output element, and an fp32 emulation with planted faults.  numpy only.

Written from the header's contract, not from the kernel's structure (N = 4H = 352):
  dKx [nx,N] = beta dKx + X^T . dz     X [K,ldx]: the first nx columns (bytes when the frames are uint8, ldx then in bytes)
  dU  [nh,N] = beta dU  + H'^T . dz    H'_k = H[k - h_shift], rows in front of row 0 read as zero, and zero where
                                       k % h_zero_period == 0 (h_zero_period == 0: no such rows)
  dKz [nz,N] = beta dKz + Z^T . dz     Z [K,ldz]: the first nz columns; nz == 0: absent
with every output at its own row stride (ld_kx, ld_u, ld_kz >= N: only the first N columns of a row are written).

The bound of one output element, |got - reference| <= |D| + KAPPA sigma (U = 2^-24, KAPPA = 6: tests/vae_reference.py):
  (a) D, the piece pairs the kernel leaves out.  An fp32 number is p0 + p1 + p2 in bf16 pieces (`split3`, the arithmetic
      of bf16_split_pair in csrc/common.h); of the nine pairs a_i b_j of a float operand and dz the three with i + j >= 3
      are dropped.  D = sum_k (a1 b2 + a2 b1 + a2 b2) is formed in fp64 from the pieces of the case's own operands: a
      deterministic term, not an estimate.  A bf16 number has 8 significant bits, so |p1| <= 2^-8 |x| and |p2| <= 2^-16 |x|:
      the dropped pairs of one product are below (2^-24 + 2^-24 + 2^-32) |a_k b_k| < 2^-23 |a_k b_k| -- the promise of the
      header, which `promise` checks on the cases.  (Random mantissas stay near 2^-27; the operands here carry the largest
      lower pieces there are, `rich`, and reach 2^-24.)  Byte frames and frames that are exact bf16 numbers are ONE piece
      times all three pieces of dz: D = 0 for dKx there.
  (b) sigma, fp32 accumulation of the exact piece products in an order the reference does not know.  What the contract does
      fix is the slab structure (the workspace size is part of the ABI): a row range of kc = `kc_rule` rows per slab, `splits`
      slabs, C = beta C + their sum.  Every fp32 addition rounds by at most U |s|, s the partial sum it produces, uniformly:
      variance U^2 s^2 / 3.
        - inside range r: P kc_r additions (P = 6 kept pairs per row, 3 for one-piece frames; kc_r the range's real rows,
          added in stages of 32 -- a stage's padding rows add exact zeros).  A partial sum is the sum of a SUBSET of the
          range's terms t_k = a_k b_k; over the orders of a sum of n terms with total P_r and sum of squares Q_r a subset of
          i terms has E s^2 = (i/n) Q_r (n-i)/(n-1) + (i/n)^2 P_r^2 <= Q_r + P_r^2, which is used for every addition:
          U^2/3 . P kc_r (Q_r + P_r^2).  (Q_r, P_r from the fp64 operands: the partial-sum magnitudes.)
        - the slab reduction: splits - 1 additions of subset sums of the P_r, each <= sum_r P_r^2 + R^2 by the same argument
          (R = the whole sum), and one more rounding of R for the value that leaves the reduction: U^2/3 . splits (sum_r P_r^2 + R^2).
        - beta C: the product and the final addition, U^2/3 ((beta C)^2 + out^2); nothing when beta == 0.
      The (i/n) factors that were dropped average 1/2 and 1/3 and a rounding error is uniform within +-ulp/2 <= U |s|, so
      sigma over-estimates an honest evaluation's standard error by about two: tests/test_wgrad_reference.py requires every
      honest order of `evaluate32` to stay below HALF of every bound.
  (c) nothing else: the piece products themselves are exact in fp32 (8 x 8 mantissa bits).
A sum over ALL K rows in one accumulator is NOT inside the bound and is not what the contract describes: at K = 16513 its own
rounding noise (6 K roundings at the full partial sum) is as large as the smallest kept piece pair, so no bound could admit
it and still notice that pair missing.  NOT covered: denormal pieces (no case produces one).

`evaluate32(case, data, order, faults, rows)` forms the kept pairs in float32 in three honest orders --
  'seq'    one accumulator per row range, row after row, pair after pair; the slabs added one after the other
  'stage'  per 32-row stage and pair one float32 matrix product added to the range's accumulator; the slabs on 16 strided
           lanes, the lanes in a tree of fours (the reduction's documented order)
  'pair'   the six products of a row added, the rows of a range in a pairwise tree, the slabs in a pairwise tree
-- with `kc_rule` for 128 (single launch) and 64 (pair launch) base ranges times split_scale, and applies the planted
faults of FAULTS, each one switch.  `can_act(case, fault)` is the explicit list of (case, fault) combinations in which a
fault changes nothing; tests/test_wgrad_reference.py asserts that those are the only ones it does not reject.
`rows`: evaluate (and bound) only these output rows per tensor -- a fault rejected on some rows is rejected on all, and the
sequential orders cost K x rows x N.
"""
from collections import namedtuple

import numpy as np

from vae_reference import U, KAPPA

N, HALF, STAGE = 352, 176, 32
TENSORS = ('dKx', 'dU', 'dKz')
FRAMES_MODE = {'general': 0, 'exact': 1, 'u8': 2}                 # CLV_FRAMES_F32, _F32_EXACT, _U8
KEPT = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (2, 0)]          # i + j <= 2
ONE_PIECE = [(0, 0), (0, 1), (0, 2)]
PAD_F32, PAD_U8 = 1.5, 200                                        # what the padding columns of the operands hold
CANARY = 4321.0                                                   # ... and those of the outputs (tests/helpers.py)

# ----------------------------------------------------------------------------------------------------- the case tables --
# the row counts of tests/test_gpu_wgrad_edges.py (tests/test_wgrad_reference.py asserts that they still are)
K_ONE_STAGE = [31, 32, 33, 64, 65, 97, 160]
K_SINGLE = K_ONE_STAGE + [4225, 8225, 12353, 16513]
K_PAIR = K_ONE_STAGE + [2113, 4161, 6209, 8257]
NXS = [4, 64, 88, 96]
HZ = [(4, 0), (88, 0), (88, 1), (88, 3), (88, 8), (64, 32), (88, 9), (96, 1), (96, 32)]        # (nh, nz): 5 narrow, 4 wide
FRAMES = ['u8', 'exact', 'general']
WINDOWS = [16, 5, 7, -1, 0]                                       # -1: one window (K); 0: no zero rows
SHIFTS = [1, 0, 2]
BETAS = [0.0, 1.0, -0.5]
FAMILIES = ['wide', 'cancel', 'mixed']
# padding of (ldx, ldh, ldz, lddz, ld_kx, ld_u, ld_kz); ldx / ldh / lddz must stay multiples of 4, the others need not
PADS = [(0, 0, 0, 0, 0, 0, 0), (4, 4, 3, 4, 4, 4, 4), (8, 0, 1, 8, 3, 0, 5), (0, 12, 5, 0, 0, 7, 1)]
PAD_NAMES = ('ldx', 'ldh', 'ldz', 'lddz', 'ld_kx', 'ld_u', 'ld_kz')

Case = namedtuple('Case', 'K nx nh nz frames period h_shift beta scale base pads family seed')


def wide(nh, nz):
    """the launcher's dispatch rule, restated from the header: more than 96 rows of H and Z together, or more than 8 of Z"""
    return nh + nz > 96 or nz > 8


def frames_for(nh, nz, frames):
    """the wide form takes no general float frames (clv_lstm_wgrad_supported): exact ones there"""
    return 'exact' if frames == 'general' and wide(nh, nz) else frames


def instance(c):
    """the template instance a case launches: (h row tiles, x pieces, byte frames)"""
    return (8 if wide(c.nh, c.nz) else 6, 3 if c.frames == 'general' else 1, c.frames == 'u8')


def kc_rule(K, scale, base):
    """rows per slab: base * scale row ranges of whole 32-row stages (split_scale in include/clvae.h)"""
    ranges = base * scale
    return (-(-K // ranges) + 31) // 32 * 32


def n_splits(K, scale, base):
    return -(-K // kc_rule(K, scale, base))


def strides(c):
    p = c.pads
    return dict(ldx=c.nx + p[0], ldh=c.nh + p[1], ldz=max(c.nz, 1) + p[2], lddz=N + p[3], ld_kx=N + p[4], ld_u=N + p[5], ld_kz=N + p[6])


def _case(K, n, i, j, hz, base, frames_i=None):
    nh, nz = HZ[hz]
    period = WINDOWS[(n + i) % 5]
    return Case(K=K, nx=NXS[(n + i) % 4], nh=nh, nz=nz, frames=frames_for(nh, nz, FRAMES[(n + n // 3) % 3 if frames_i is None else frames_i]),
                period=K if period < 0 else period, h_shift=SHIFTS[(n + n // 4) % 3], beta=BETAS[(n + i + j // 2) % 3],
                scale=1 + (i + j // 2) % 2, base=base, pads=PADS[(n + n // 5) % 4], family=FAMILIES[(n + j) % 3], seed=n)


def single_cases():
    """every K with four combinations of the other parameters, each list walked at its own stride: every value of every list
    meets one-stage K and many-stage K (tests/test_wgrad_reference.py checks that)"""
    return [_case(K, 4 * i + j, i, j, (4 * i + j) % 9, 128) for i, K in enumerate(K_SINGLE) for j in range(4)]


PAIR_HZ = [(1, 2), (5, 6), (3, 4), (7, 8), (0, 1), (8, 5), (4, 3), (6, 7), (2, 0), (5, 8), (1, 4)]     # same form of the kernel


def pair_cases():
    """[(p, q)]: the same K, frame mode and kernel form; nx, nh, nz, strides, beta, h_shift and the window differ"""
    out = []
    for i, K in enumerate(K_PAIR):
        for j in range(2):
            n = 2 * i + j
            a, b = PAIR_HZ[n % 11]
            fi = (n + n // 3) % 3
            if wide(*HZ[a]) and FRAMES[fi] == 'general':
                fi = n % 2
            p, q = _case(K, n, i, 2 * j, a, 64, fi), _case(K, n + 23, i + 1, 2 * j + 1, b, 64, fi)
            out.append((p, q._replace(scale=p.scale)))
    return out


# ----------------------------------------------------------------------------------------------------------- operands --
Data = namedtuple('Data', 'X H Z dz C0')


def rich(x):
    """x with the low 16 mantissa bits set to 0x7F3F: p0 is x truncated to bf16, p1 = 0x7F00 and p2 = 0x3F units of the last
    place, both of x's sign -- the lower pieces as large as they get without a round-up (|p1| ~ 2^-8 |x|, |p2| ~ 2^-17 |x|),
    so that every piece pair is a COHERENT share of the product (2^-17 for the smallest kept ones) and not a random 2^-20"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u & np.uint32(0xffff0000)) | np.uint32(0x7F3F)).view(np.float32).astype(np.float64)


def _signs(c):
    """'mixed': the sign of row k of dz (beta, random) and of the float rows of X, H' and Z (alpha): random, except that
    rows 8..15 of a stage carry the dz sign of the row 16 further on and rows 24..31 that of the row 16 back -- correctly paired
    terms have random signs, terms of a half stage paired with the other half's dz rows are all positive"""
    rng = np.random.default_rng([c.seed, 77])
    n = (c.K + 95) // 32 * 32
    beta, alpha = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
    k = np.arange(n)
    lo, hi = k[(k % STAGE) // 8 == 1], k[(k % STAGE) // 8 == 3]
    alpha[lo], alpha[hi] = beta[lo + 16], beta[hi - 16]
    return alpha[:, None], beta[:, None]


def build(c):
    """The operands of a case, at their strides (the padding columns hold PAD_F32 / PAD_U8), and the outputs' initial
    contents C0 (finite where beta != 0, NaN otherwise; CANARY in the padding columns).  Families:
      'wide'    dz = normal x exp(2 normal) per row, the dz of tests/test_gpu_wgrad_edges.py (rows 0, 1, 2 and K - 1 at the largest
                scale, so that a fault on those rows is never below every bound)
      'cancel'  the rows of X, H' and Z in pairs (a, a (1 - 2^-11)) (byte and exact frames: (a, a)), dz rows (v, -v (1 + 2^-12)):
                the sums are ~2^-12 of the magnitudes, and no piece product of one row cancels its partner's
      'mixed'   |values| with the sign of rows 24..31 of every 32-row stage flipped on both sides of the float products (on dz
                alone for unsigned frames): every correctly paired float term is positive, and a stage half paired with the
                wrong dz rows changes sign instead of cancelling."""
    rng = np.random.default_rng([c.seed, c.K, c.nx, c.nh, c.nz, c.base])
    K, ld, fam = c.K, strides(c), c.family
    k = np.arange(K)
    alpha, sbeta = _signs(c)
    def odd_up(v, shift=0):                   # 'cancel': the second row of every pair (as H' sees it) times 1 - 2^-11
        if fam == 'cancel':
            o = (k + shift) % 2 == 1
            v[o] = (v[o] * (1 - 2.0 ** -11)).astype(np.float32)
        return v
    half = lambda gen, shift=0: gen((K + shift + 1) // 2 + 1)[(np.arange(K) + shift) // 2] if fam == 'cancel' else gen(K)
    if c.frames == 'general':
        Xv = half(lambda m: rng.standard_normal((m, c.nx)))
        if fam == 'mixed':
            Xv = np.abs(Xv) * alpha[k]
        X, Xv = np.full((K, ld['ldx']), PAD_F32, np.float32), odd_up(rich(Xv))
    else:
        Xv = half(lambda m: (rng.random((m, c.nx)) < 0.3) * (rng.integers(1, 256, (m, c.nx)) if c.frames == 'u8' else 1))
        X = np.full((K, ld['ldx']), PAD_U8 if c.frames == 'u8' else PAD_F32, np.uint8 if c.frames == 'u8' else np.float32)
    X[:, :c.nx] = Xv
    if c.frames != 'general':
        X[K - 1, :c.nx] = np.maximum(X[K - 1, :c.nx], 1)          # every note of the last frame on: a dropped last row shows in every dKx row
    # H'_k = H[k - h_shift]: the pairs and the signs are laid out on H' (row j of H is seen at k = j + h_shift)
    Hv = half(lambda m: np.tanh(rng.standard_normal((m, c.nh))), c.h_shift)
    if fam == 'mixed':
        Hv = np.abs(Hv) * alpha[k + c.h_shift]
    H = np.full((K, ld['ldh']), PAD_F32, np.float32)
    H[:, :c.nh] = odd_up(rich(Hv), c.h_shift)
    Z = None
    if c.nz:
        Zv = half(lambda m: rng.standard_normal((m, c.nz)))
        if fam == 'mixed':
            Zv = np.abs(Zv) * alpha[k]
        Z = np.full((K, ld['ldz']), PAD_F32, np.float32)
        Z[:, :c.nz] = odd_up(rich(Zv))
    dz = np.full((K, ld['lddz']), PAD_F32, np.float32)
    if fam == 'wide':
        s = np.exp(rng.standard_normal((K, 1)) * 2)
        s[[0, 1, 2, K - 1]] = s.max()
        dz[:, :N] = rich(rng.standard_normal((K, N)) * s)
    elif fam == 'cancel':
        v = rich(rng.standard_normal(((K + 1) // 2, N)))
        dz[0::2, :N], dz[1::2, :N] = v[:(K + 1) // 2], (-v * (1 + 2.0 ** -12))[:K // 2]
    else:
        dz[:, :N] = rich((np.abs(rng.standard_normal((K, N))) + 0.25) * sbeta[k])
    C0 = {}
    for name, n, l in (('dKx', c.nx, ld['ld_kx']), ('dU', c.nh, ld['ld_u']), ('dKz', c.nz, ld['ld_kz'])):
        if n:
            C0[name] = np.full((n, l), CANARY, np.float32)
            C0[name][:, :N] = rng.standard_normal((n, N)) if c.beta != 0 else np.nan
    return Data(X, H, Z, dz, C0)


def h_prime(Hv, K, shift, period, zero_at=0, front=0.0):
    """H'_k = H[k - shift]; `front` where k - shift < 0, zero where it is >= K; zero where k % period == zero_at"""
    Hp = np.zeros((K, Hv.shape[1]), Hv.dtype)
    src = np.arange(K) - shift
    Hp[src < 0] = front
    ok = (src >= 0) & (src < K)
    Hp[ok] = Hv[src[ok]]
    if period and zero_at is not None:
        Hp[np.arange(K) % period == zero_at] = 0
    return Hp


def operands(c, D, faults=()):
    """{tensor: A [K, n] float64}, dz [K, N] float64: the values the products are over (the faults that act on them applied)"""
    K, X = c.K, D.X[:, :c.nx].astype(np.float64)
    if 'byte_reverse' in faults and c.frames == 'u8':
        X = X.reshape(K, c.nx // 4, 4)[:, :, ::-1].reshape(K, c.nx)
    shift = c.h_shift + (1 if 'h_shift_off' in faults else 0)
    Hp = h_prime(D.H[:, :c.nh].astype(np.float64), K, shift, c.period,
                 zero_at=None if 'no_zero_start' in faults else (1 if 'zero_next_row' in faults else 0),
                 front=1.0 if 'row_before_0' in faults else 0.0)
    A = {'dKx': X, 'dU': Hp}
    if c.nz:
        Z = D.Z[:, :c.nz].astype(np.float64)
        if 'z_leak' in faults and D.Z.shape[1] > c.nz:
            Z = Z.copy()
            Z[:, -1] = (D.Z[:, c.nz - 1] + D.Z[:, c.nz]).astype(np.float64)
        A['dKz'] = Z
    dz = D.dz[:, :N].astype(np.float64)
    if 'drop_last_row' in faults:
        dz = dz.copy()
        dz[K - 1] = 0
    if 'garbage_past_K' in faults and K % STAGE:                    # one more row, all ones, in the ragged last stage
        A = {t: np.vstack([a, np.ones((1, a.shape[1]))]) for t, a in A.items()}
        dz = np.vstack([dz, np.ones((1, N))])
    return A, dz


def all_rows(c):
    return {t: np.arange(n) for t, n in zip(TENSORS, (c.nx, c.nh, c.nz)) if n}


def some_rows(c, count=4):
    """the first and the last row of every tensor and evenly spaced ones between (at most `count`)"""
    return {t: np.unique(np.linspace(0, n - 1, min(n, count)).astype(int)) for t, n in zip(TENSORS, (c.nx, c.nh, c.nz)) if n}


# ------------------------------------------------------------------------------------------------- reference and bound --
def reference(c, D, rows=None):
    """{tensor: fp64 [rows, N]}"""
    A, dz = operands(c, D)
    rows = rows or all_rows(c)
    out = {}
    for t, a in A.items():
        out[t] = a[:, rows[t]].T @ dz
        if c.beta != 0:
            out[t] += np.float64(np.float32(c.beta)) * D.C0[t][rows[t], :N].astype(np.float64)
    return out


def _bf16(x):
    """float32 -> the nearest bf16 number (ties to even), as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((u + (0x7fff + ((u >> 16) & 1))) & np.uint32(0xffff0000)).view(np.float32)


def split3(x):
    """x = p0 + p1 + p2 in bf16 pieces (float32 arrays): round, subtract (exact in fp32), round, subtract, round"""
    x = np.ascontiguousarray(x, np.float32)
    p0 = _bf16(x)
    r = x - p0
    p1 = _bf16(r)
    return p0, p1, _bf16(r - p1)


def float_operand(c, t):
    return t != 'dKx' or c.frames == 'general'


def promise(c, D):
    """the largest |dropped pairs of a product| / |a b| the pieces of this case's operands allow (the largest relative p1 and p2
    of either side combined): the header says < 2^-23"""
    A, dz = operands(c, D)
    rel = lambda x: [np.max(np.abs(p)[x != 0] / np.abs(x)[x != 0], initial=0.0) for p in split3(x)]
    _, b1, b2 = rel(dz.astype(np.float32))
    worst = 0.0
    for t, a in A.items():
        if float_operand(c, t):
            _, a1, a2 = rel(a.astype(np.float32))
            worst = max(worst, a1 * b2 + a2 * b1 + a2 * b2)
    return worst


def bound(c, D, rows=None):
    """{tensor: (bound, sigma, dropped) fp64 [rows, N]}: the module docstring's |D| + KAPPA sigma"""
    A, dz = operands(c, D)
    rows = rows or all_rows(c)
    kc, S = kc_rule(c.K, c.scale, c.base), n_splits(c.K, c.scale, c.base)
    b = [p.astype(np.float64) for p in split3(dz)]
    out = {}
    for t, a in A.items():
        a = np.ascontiguousarray(a[:, rows[t]])
        fl = float_operand(c, t)
        var = np.zeros((a.shape[1], N))
        sumP2 = np.zeros_like(var)
        R = np.zeros_like(var)
        for r in range(S):
            ar, br = a[r * kc:(r + 1) * kc], dz[r * kc:(r + 1) * kc]
            P, Q = ar.T @ br, (ar * ar).T @ (br * br)
            var += (6 if fl else 3) * len(ar) * (Q + P * P)
            sumP2 += P * P
            R += P
        var += S * (sumP2 + R * R)
        if c.beta != 0:
            bc = np.float64(np.float32(c.beta)) * D.C0[t][rows[t], :N].astype(np.float64)
            var += bc * bc + (R + bc) ** 2
        sigma = U * np.sqrt(var / 3)
        dropped = np.zeros_like(var)
        if fl:
            p = [q.astype(np.float64) for q in split3(a)]
            dropped = np.abs(p[1].T @ b[2] + p[2].T @ (b[1] + b[2]))
        out[t] = (dropped + KAPPA * sigma, sigma, dropped)
    return out


def old_bar(c, D, rows=None):
    """the bar of the older tests: 2e-6 x sum |a b|"""
    A, dz = operands(c, D)
    rows = rows or all_rows(c)
    return {t: 2e-6 * (np.abs(a[:, rows[t]]).T @ np.abs(dz)) for t, a in A.items()}


def first_offender(got, ref, bnd):
    """(row, column, |err|, bound) of the first element beyond its bound (a NaN counts), or None"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    bad = ~(err <= bnd)
    if not bad.any():
        return None
    r, col = np.argwhere(bad)[0]
    return int(r), int(col), float(err[r, col]), float(bnd[r, col])


def worst_ratio(got, ref, bnd):
    """max |err| / bound (0 / 0 = 0; an error where the bound is 0, or a NaN: inf)"""
    err = np.abs(np.asarray(got, np.float64) - ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0, 0.0, err / bnd)
    return float(np.max(np.where(np.isnan(q), np.inf, q)))


# ------------------------------------------------------------------------------------------------------- the emulation --
ORDERS = ('seq', 'stage', 'pair')
FAULTS = ([('drop_pair', g, i, j) for g in ('dU', 'dKz', 'dKx') for i, j in KEPT] +
          [('drop_dz_piece', 1), ('drop_dz_piece', 2), ('one_piece', 'dU'),
           'no_zero_start', 'zero_next_row', 'h_shift_off', 'row_before_0', 'garbage_past_K', 'drop_last_row',
           ('stage', 'first', 0), ('stage', 'last', 0), ('stage', 'first', 2), ('stage', 'last', 2),
           ('slab', 0), ('slab', 2), 'beta_ignored', 'beta_per_slab', 'swap_halves', 'tile_leak', 'byte_reverse', 'z_leak',
           'mispair_half', 'stride_N'])


def can_act(c, fault):
    """False for exactly the (case, fault) combinations in which the fault changes nothing -- the explicit list:
      a piece pair of the Z rows without Z rows; of the X rows, and a dz piece of the X rows, with the other kind of frames;
      the window faults with h_zero_period == 0, and with ONE window (period K) where the rows they touch read in front of
        row 0 anyway (no_zero_start: h_shift > 0; zero_next_row: h_shift == 2);
      a row in front of row 0 where no row reads there (h_shift == 0) or the only such row is a window start (h_shift == 1
        with a period);
      a garbage row past K when the last stage is not ragged (K % 32 == 0);
      the slab faults and beta per slab with one slab; the beta faults with beta == 0;
      the byte order for other than byte frames; the Z column leak without Z or without a longer Z row;
      the output stride when no output of two or more rows has ld > N."""
    S = n_splits(c.K, c.scale, c.base)
    ld = strides(c)
    name = fault if isinstance(fault, str) else fault[0]
    if name == 'drop_pair':
        return {'dU': True, 'dKz': c.nz > 0, 'dKx': c.frames == 'general'}[fault[1]]
    if name == 'drop_dz_piece':
        return c.frames != 'general'
    if name == 'no_zero_start':
        return c.period != 0 and (c.period < c.K or c.h_shift == 0)
    if name == 'zero_next_row':
        return c.period != 0 and (c.period < c.K or c.h_shift < 2)
    if name == 'row_before_0':
        return c.h_shift == 2 or (c.h_shift == 1 and c.period == 0)
    if name == 'garbage_past_K':
        return c.K % STAGE != 0
    if name == 'slab':
        return S > 1
    if name == 'beta_ignored':
        return c.beta != 0
    if name == 'beta_per_slab':
        return c.beta != 0 and S > 1
    if name == 'byte_reverse':
        return c.frames == 'u8'
    if name == 'z_leak':
        return c.nz > 0 and ld['ldz'] > c.nz
    if name == 'stride_N':
        return ld['ld_kx'] > N or ld['ld_u'] > N or (c.nz > 1 and ld['ld_kz'] > N)
    return True


def _tree(x, axis_len):
    """pairwise tree over axis 1 of float32 x [S, axis_len, ...]"""
    while x.shape[1] > 1:
        n = x.shape[1]
        y = x[:, 0:n - n % 2:2] + x[:, 1:n:2]
        x = np.concatenate([y, x[:, n - 1:]], axis=1) if n % 2 else y
    return x[:, 0]


def evaluate32(c, D, order='stage', faults=(), rows=None):
    """{tensor: float32 [rows, N]}: the contract evaluated in float32 from bf16 pieces (module docstring)"""
    assert order in ORDERS
    faults = tuple(faults)
    names = [f if isinstance(f, str) else f[0] for f in faults]
    A, dz = operands(c, D, names)
    rows = rows or all_rows(c)
    if 'stride_N' in names:
        rows = {t: np.arange(min(len(all_rows(c)[t]), 3)) for t in rows}
    kc, S = kc_rule(c.K, c.scale, c.base), n_splits(c.K, c.scale, c.base)
    f32 = np.float32

    def ranges(x):                        # [K', n] -> float32 [S, kc, n], zero rows behind the last one
        y = np.zeros((S * kc, x.shape[1]), f32)
        y[:len(x)] = x
        return y.reshape(S, kc, x.shape[1])
    B = [ranges(p) for p in split3(dz)]
    wslab = np.ones(S, f32)
    for f in faults:
        if f[0] == 'slab' and S > 1:
            wslab[S // 2] = f[1]
    beta = f32(c.beta)
    out = {}
    for t, a in A.items():
        a = a[:, rows[t]]
        fl = float_operand(c, t)
        pairs = list(KEPT if fl else ONE_PIECE)
        for f in faults:
            if f[0] == 'drop_pair' and f[1] == t and fl:
                pairs.remove((f[2], f[3]))
            if f[0] == 'drop_dz_piece' and t == 'dKx' and not fl:
                pairs.remove((0, f[1]))
            if f[0] == 'one_piece' and f[1] == t:
                pairs = ONE_PIECE
        P = [ranges(p) for p in (split3(a) if fl else (a.astype(f32),))]
        if not fl:
            assert np.array_equal(_bf16(P[0]), P[0]), "frames that are not bf16 numbers"
        last = -(-c.K // STAGE) - 1 - (S - 1) * (kc // STAGE)          # the last real stage of the last range
        for f in faults:
            if f[0] == 'stage':                                        # one stage of one row range dropped or counted twice
                r = S // 2
                s = 0 if f[1] == 'first' else (last if r == S - 1 else kc // STAGE - 1)
                for p in P:
                    p[r, s * STAGE:(s + 1) * STAGE] *= f32(f[2])
        if 'mispair_half' in names:                                    # rows 8..15 of every stage of A <-> rows 24..31
            for p in P:
                v = p.reshape(S, kc // STAGE, 4, 8, -1)
                v[:, :, [1, 3]] = v[:, :, [3, 1]]
        m = a.shape[1]
        if order == 'stage':
            acc = np.zeros((S, m, N), f32)
            for s in range(kc // STAGE):
                sl = slice(s * STAGE, (s + 1) * STAGE)
                for i, j in pairs:
                    acc += np.matmul(P[i][:, sl].transpose(0, 2, 1), B[j][:, sl])
        elif order == 'seq':
            acc = np.zeros((S, m, N), f32)
            for k in range(kc):
                for i, j in pairs:
                    acc += P[i][:, k, :, None] * B[j][:, k, None, :]
        else:
            acc = np.empty((S, m, N), f32)
            for r in range(m):                                         # (row by row: [S, kc, N] at a time)
                terms = np.zeros((S, kc, N), f32)
                for i, j in pairs:
                    terms += P[i][:, :, r, None] * B[j]
                acc[:, r] = _tree(terms, kc)
        acc *= wslab[:, None, None]
        if order == 'seq':
            v = np.zeros((m, N), f32)
            for r in range(S):
                v += acc[r]
        elif order == 'pair':
            v = _tree(acc[None], S) if S > 1 else acc[0]
            v = np.asarray(v, f32).reshape(m, N)
        else:
            lanes = []
            for z in range(min(16, S)):
                w = np.zeros((m, N), f32)
                for r in range(z, S, 16):
                    w += acc[r]
                lanes.append(w)
            lanes += [np.zeros((m, N), f32)] * (16 - len(lanes))
            four = [(lanes[4 * q] + lanes[4 * q + 1]) + (lanes[4 * q + 2] + lanes[4 * q + 3]) for q in range(4)]
            v = (four[0] + four[1]) + (four[2] + four[3])
        if 'swap_halves' in names:
            v = np.concatenate([v[:, HALF:], v[:, :HALF]], axis=1)
        if 'tile_leak' in names:                                       # the padded twelfth tile of the first half is the next 16 columns
            v = v.copy()
            v[:, HALF - 16:HALF] += v[:, HALF:HALF + 16]
        if c.beta != 0 and 'beta_ignored' not in names:
            c0 = D.C0[t][rows[t], :N]
            v = v + (beta * f32(S) if 'beta_per_slab' in names else beta) * c0
        if 'stride_N' in names:                                        # row r written at r * N of a buffer whose rows are ld apart
            ld = D.C0[t].shape[1]
            flat = D.C0[t][:len(rows[t])].copy().reshape(-1)
            src = v.copy()
            if c.beta == 0:
                flat[:] = 0                                            # (what was there is unknown: any finite number)
            flat[:src.size] = src.reshape(-1)
            w = flat.reshape(len(rows[t]), ld)[:, :N]
            known = (np.arange(len(rows[t]))[:, None] * ld + np.arange(N)[None, :]) < src.size
            v = np.where(known, w, src)
        out[t] = v
    return out
