"""fp64 reference of the output head of cl_vrnn in training (include/clvae.h: clv_out_head_train; H = D = 88).

Written from the header's contract, not from either kernel's structure:
  logits = hs.Wo + bo                                                      [R,88]
  rownll = sum_j max(l, 0) + log(1 + exp(-|l|)) - l y,  l = clip(logits)     [R]     (O.bce_from_logits_keras)
  dl     = scale (sigmoid(l) - y) where LO <= logits <= HI, else 0         [R,88]  (the clip points themselves inside)
  dhs    = dl.Wo^T   [R,88],   dWo = hs^T.dl   [88,88],   dbo = sum_r dl   [88]
LO / HI are the float32 Keras clip points BCE_CLIP_LO / BCE_CLIP_HI of csrc/common.h (asymmetric: -16.118095,
+15.942385), here the fp32 constants themselves, so that a logit that IS a clip point is inside for the reference as for a
kernel; tests/test_out_head_reference.py checks that they are the oracle's points rounded to fp32.

Bounds.  As tests/vae_reference.py (U, KAPPA and the transcendental budgets are imported from there): beside every output
element a first-order standard error sigma ('s_' + name) of an fp32 evaluation of the contract, the element's bound
('b_' + name) is KAPPA sigma:
  * a dot product of n terms: (U sum|terms|)^2 n / 3 for its roundings plus (U |result|)^2 (n = 89 with the bias; the
    weight gradients sum over the R rows: n = R + 1);
  * __expf, __logf, fast_rcp: EXP_ULP (+ |x| for the argument), LOG_ABS, RCP_ULP; every other fp32 operation one U;
  * logits' variance reaches rownll and dl through the first derivative, dl's reaches dhs, dWo, dbo the same way;
  * dropped=True (the bf16-MFMA kernel, csrc/out_head_bf16.hip): every product a b is formed from bf16 pieces
    a = a0 + a1 + a2, b = b0 + b1 + b2 without the pairs a1 b2, a2 b1, a2 b2.  Piece widths: bf16 keeps 8 significant bits,
    round to nearest even, so for 2^e <= |x| < 2^(e+1):  |x - p0| <= 2^(e-8),  hence |p1| <= 2^(e-8) <= 2^-8 |x|;  the
    residual r1 = x - p0 has at most 16 significant bits and is either 2^(e-8) exactly (then p2 = 0) or below it, in a
    binade 2^e1 with e1 <= e - 9, where p1 = bf16(r1) leaves |p2| <= 2^(e1-8) <= 2^(e-17) <= 2^-17 |x|; r1 - p1 has at
    most 8 bits, so p2 is exact and p0 + p1 + p2 == x.  The dropped pairs are therefore at most
        (2 * 2^-8 * 2^-17 + 2^-34) |a b| = 2^-24 (1 + 2^-10) |a b| = DROP |a b|
    per product (the kernel's header promises 2^-24; the exact emulation below measures 0.9 * 2^-24 at worst).  It enters
    sigma^2 as sum over the terms of (DROP |term|)^2 (no distribution assumed: the whole bound as one standard error).
Flags (r['flags']): clip_l, the logits within their bound of a clip point, where fp32 may take the other branch of dl:
sigma of dl there is widened by the whole difference |scale (sigmoid(l) - y)|.
Criteria: `violations` (any element beyond its bound; a NaN counts) and, per output tensor of at least 1000 elements,
rms(err / sigma) <= 1 (`rms_violations`): sigma is an upper estimate of the standard error, so an honest evaluation stays
below 1, while a small systematic fault that no single element betrays can raise the rms above it.

Single-product cases (`single_case`: Wo = a permutation matrix times random values, bo = 0): logits[r, perm[h]] =
hs[r, h] v[h] is ONE product, and with the stored dl taken as exact input so are dhs[r, h] = dl[r, perm[h]] v[h] and, at
R = 1, dWo[h, j] = hs[0, h] dl[0, j]; dbo = dl[0] bit for bit (the ones column has the pieces (1, 0, 0)).  No accumulation
of different terms takes part, so the bound is a worst case, not a sigma:
  f32-MFMA kernel: the product, rounded once:                                    U |a b|
  bf16 kernel: six partial products added one after the other (each sum at most (1 + 2^-7) |a b|: |a0| <= (1 + 2^-8) |a|),
  six roundings, plus what is dropped:                                           (6 U (1 + 2^-7) + DROP) |a b|
This separates the kernel's 6 of 9 pairs (at most 7.05 U) from 5 of 9 (a0 b2 left out too: up to 2^-17 = 128 U of a product,
median 23 U): per element the random cases cannot, because the bound of an honest fp32 accumulation of 88 terms covers it
(tests/test_out_head_reference.py has the figures).
Nothing here is fitted to errors seen on a GPU.
"""
import numpy as np

from oracle import clvae_oracle as O
from vae_reference import U, KAPPA, EXP_ULP, LOG_ABS, RCP_ULP, CLIP_LO32, CLIP_HI32, F32

N = 88                                   # hidden units == notes
OUTPUTS = ('logits', 'rownll', 'dl', 'dhs', 'dWo', 'dbo')
CLIP = (float(CLIP_LO32), float(CLIP_HI32))
DROP = 2.0 ** -24 * (1 + 2.0 ** -10)     # derived above: what 6 of 9 piece pairs leave out of a product, relative
SINGLE = {'f32': U, 'bf16': 6 * U * (1 + 2.0 ** -7) + DROP}        # single-product bounds, relative to |a b|
RMS_MIN = 1000                           # the rms criterion is enforced for tensors of at least this many elements


# ---------------------------------------------------------------------------------------------------------- pieces --
def bf16_rne(x):
    """fp32 -> the nearest bf16 as fp32, ties to even (v_cvt_pk_bf16_f32), on the bits"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    u = (u + (((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7fff))) & np.uint32(0xffff0000)
    return u.view(np.float32)


def split3(x):
    """exact emulation of bf16_split_pair (csrc/common.h): fp32 x -> pieces (p0, p1, p2), each a bf16 value held in fp32;
    the residuals are exact fp32 subtractions"""
    x = np.ascontiguousarray(x, np.float32)
    p0 = bf16_rne(x)
    r1 = x - p0
    p1 = bf16_rne(r1)
    p2 = bf16_rne(r1 - p1)
    return p0, p1, p2


def piece_product(a, b, pieces):
    """a * b in fp64 from bf16 pieces: 9 = all pairs (a b itself: 48 bits, exact in fp64), 6 = the kernel's pairs
    (i + j <= 2), 5 = a0 b2 left out too, 1 = a0 b0 alone.  a, b: fp32 arrays that broadcast."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    if pieces == 9:
        return a64 * b64
    a0, a1, a2 = [p.astype(np.float64) for p in split3(a)]
    b0, b1, b2 = [p.astype(np.float64) for p in split3(b)]
    if pieces == 1:
        return a0 * b0
    t = a64 * b64 - a1 * b2 - a2 * (b1 + b2)
    if pieces == 5:
        t = t - a0 * b2
    elif pieces != 6:
        raise ValueError(pieces)
    return t


class F32P(F32):
    """vae_reference.F32 with the products optionally formed from emulated bf16 pieces; long sums (the weight gradient's R
    rows) run in 64 shuffled lanes that are added at the end, a shuffled order like any other"""
    LANES = 64

    def __init__(self, rng, pieces=9):
        F32.__init__(self, rng)
        self.pieces = pieces

    def _term(self, a, b):
        if self.pieces == 9:
            return a * b                                     # fp32: the product rounded once
        return piece_product(a, b, self.pieces)

    def _add(self, acc, t):
        return acc + t if t.dtype == np.float32 else (acc.astype(np.float64) + t).astype(np.float32)

    def dot(self, A, B):
        A, B = self.c(A), self.c(B)
        K = A.shape[1]
        perm = self.rng.permutation(K)
        if K <= 4 * self.LANES:
            acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
            for k in perm:
                acc = self._add(acc, self._term(A[:, k, None], B[None, k, :]))
            return acc
        G = self.LANES
        acc = np.zeros((G, A.shape[0], B.shape[1]), np.float32)
        AT = np.ascontiguousarray(A.T)
        for s in range(0, K, G):
            ks = perm[s:s + G]
            acc[:len(ks)] = self._add(acc[:len(ks)], self._term(AT[ks][:, :, None], B[ks][:, None, :]))
        out = np.zeros(acc.shape[1:], np.float32)
        for g in self.rng.permutation(G):
            out = out + acc[g]
        return out

    def colsum(self, A):
        A = self.c(A)
        if A.shape[0] <= 4 * self.LANES:
            return F32.colsum(self, A)
        G = self.LANES
        perm = self.rng.permutation(A.shape[0])
        acc = np.zeros((G,) + A.shape[1:], np.float32)
        for s in range(0, A.shape[0], G):
            ks = perm[s:s + G]
            acc[:len(ks)] = acc[:len(ks)] + A[ks]
        return F32.colsum(self, acc)


class _F64:
    dt = np.float64
    c = staticmethod(lambda a: np.asarray(a, np.float64))
    dot = staticmethod(lambda A, B: A @ B)
    colsum = staticmethod(lambda A: A.sum(0))
    rowsum = staticmethod(lambda A: A.sum(-1))
    exp = staticmethod(np.exp)
    log = staticmethod(np.log)
    rcp = staticmethod(lambda x: 1.0 / x)


# ----------------------------------------------------------------------------------------------------------- values --
FAULTS = ('sym_clip', 'dl_outside', 'bias_tile', 'nll_drop_80_87', 'sigmoid_branch', 'y_col_plus1', 'y_pitch88',
          'scale_twice', 'dhs_Wo_not_T', 'dWo_drop_last_row', 'row_beyond_R', 'slab_dropped', 'dbo_from_hs87')


def targets(Ypad, R, ldy, faults=()):
    """the [R,88] targets out of the padded [R,ldy] array (faults: the misreadings a kernel could make)"""
    flat = np.asarray(Ypad).reshape(-1)
    pitch = N if 'y_pitch88' in faults else ldy
    idx = np.arange(R)[:, None] * pitch + np.arange(N)[None, :] + (1 if 'y_col_plus1' in faults else 0)
    return flat[np.minimum(idx, flat.size - 1)]


def _values(ar, hs, Wo, bo, Y, scale, clip=CLIP, faults=(), rng=None):
    c = ar.c
    hs, Wo, bo, Y = c(hs), c(Wo), c(bo), c(Y)
    R = hs.shape[0]
    lo, hi = clip
    if 'sym_clip' in faults:
        hi = -lo
    lo, hi = c(lo), c(hi)
    if 'bias_tile' in faults:
        bo = bo.copy()
        bo[32:48] = 0
    logits = ar.dot(hs, Wo) + bo
    l = np.clip(logits, lo, hi)
    el = ar.exp(-np.abs(l))
    terms = np.maximum(l, 0) + ar.log(c(1.0) + el) - l * Y
    rownll = ar.rowsum(terms[:, :80] if 'nll_drop_80_87' in faults else terms)
    r1 = ar.rcp(c(1.0) + el)
    sg = r1 if 'sigmoid_branch' in faults else np.where(l >= 0, r1, el * r1)
    inside = (logits >= lo) & (logits <= hi)
    if 'dl_outside' in faults:
        inside = np.ones_like(inside)
    sc = c(scale)
    if 'scale_twice' in faults:
        sc = sc * sc
    dl = np.where(inside, sc * (sg - Y), c(0.0)).astype(ar.dt)
    dhs = ar.dot(dl, Wo if 'dhs_Wo_not_T' in faults else Wo.T)
    gh, gd = hs, dl
    if 'dWo_drop_last_row' in faults:
        gh, gd = hs[:-1], dl[:-1]
    if 'slab_dropped' in faults:
        assert R > 256
        gh, gd = np.delete(hs, np.s_[128:256], 0), np.delete(dl, np.s_[128:256], 0)
    if 'row_beyond_R' in faults:               # a row of garbage hs scored against y = 0
        g = c(np.tanh(rng.standard_normal((1, N))))
        gl = np.clip(g.astype(np.float64) @ Wo.astype(np.float64) + bo, float(lo), float(hi))
        gh, gd = np.concatenate([hs, g]), np.concatenate([dl, c(float(sc) * O.sigmoid(gl))])
    dWo = ar.dot(gh.T, gd) if gh.shape[0] else np.zeros((N, N), ar.dt)
    dbo = ar.dot(gh[:, 87:88].T, gd)[0] if 'dbo_from_hs87' in faults else (ar.colsum(gd) if gd.shape[0] else np.zeros(N, ar.dt))
    out = dict(logits=logits, rownll=rownll, dl=dl, dhs=dhs, dWo=dWo, dbo=dbo)
    return out, dict(l=l, el=el, sg=sg, inside=inside)


# -------------------------------------------------------------------------------------------------------- reference --
def reference(hs, Wo, bo, Y, scale, dropped=True, clip=CLIP, values=None):
    """the fp64 reference: the six outputs, 's_' + name (sigma), 'b_' + name (KAPPA sigma), 'flags'.  Inputs hold fp32
    values; Y [R,88].  dropped: include what the bf16 kernel's 6 of 9 piece pairs leave out (False: the f32-MFMA kernel).
    values: r['values'] of an earlier call on the same inputs (the bounds of the other kernel without the fp64 pass)."""
    hs, Wo, bo, Y = [np.asarray(a, np.float64) for a in (hs, Wo, bo, Y)]
    R = hs.shape[0]
    scale = float(np.float32(scale))
    values = values or _values(_F64, hs, Wo, bo, Y, scale, clip)
    r, k = dict(values[0]), values[1]
    r['values'] = values
    A, sq = np.abs, np.square
    d2 = DROP ** 2 if dropped else 0.0

    def dotvar(a, va, B, bias, n):
        """variance of a . B (+ bias): the operand's through B, the n roundings, the result's own, the dropped pairs"""
        loc = U * (A(a) @ A(B) + (A(bias) if bias is not None else 0.0))
        return va @ sq(B) + sq(loc) * n / 3.0 + sq(U * A(a @ B + (bias if bias is not None else 0.0))) + d2 * (sq(a) @ sq(B))

    v_l = dotvar(hs, np.zeros_like(hs), Wo, bo, N + 1)
    b_l = KAPPA * np.sqrt(v_l)
    logits, l, el, sg, inside = r['logits'], k['l'], k['el'], k['sg'], k['inside']
    lo, hi = clip
    flag = (A(logits - lo) <= b_l) | (A(logits - hi) <= b_l)
    gl = np.where(inside | flag, A(sg - Y), 0.0)
    tn = A(np.maximum(l, 0)) + A(np.log1p(el)) + A(l * Y)
    v_nll = (sq(gl) * v_l).sum(1) + (sq(U * (2 * tn + LOG_ABS)) + sq(el / (1 + el) * (EXP_ULP + A(l)) * U)).sum(1) \
        + sq(U * tn.sum(1)) * (N + 1) / 3.0
    # dl = scale (sg - y): the logit's error through sigmoid', sg's own (exp, 1 + e, rcp, e r1), the subtraction, the scaling
    v_dl = np.where(inside, sq(scale * sg * (1 - sg)) * v_l + sq(scale * sg * U * (RCP_ULP + EXP_ULP + A(l) + 2))
                    + 2 * sq(scale * U * A(sg - Y)), 0.0)
    v_dl = v_dl + np.where(flag, sq(scale * A(sg - Y)), 0.0)
    dl = r['dl']
    v_dhs = dotvar(dl, v_dl, Wo.T, None, N + 1)
    v_dWo = sq(hs).T @ v_dl + sq(U * (A(hs).T @ A(dl))) * (R + 1) / 3.0 + sq(U * A(r['dWo'])) + d2 * (sq(hs).T @ sq(dl))
    v_dbo = v_dl.sum(0) + sq(U * A(dl).sum(0)) * (R + 1) / 3.0 + sq(U * A(r['dbo']))
    for name, v in (('logits', v_l), ('rownll', v_nll), ('dl', v_dl), ('dhs', v_dhs), ('dWo', v_dWo), ('dbo', v_dbo)):
        r['s_' + name] = np.sqrt(v)
        r['b_' + name] = KAPPA * r['s_' + name]
    r['flags'] = dict(clip_l=flag)
    r['outside'] = int((~inside).sum())
    return r


def ref_case(case, **kw):
    return reference(case['hs'], case['Wo'], case['bo'], case['Y'], case['scale'], **kw)


def evaluate32(case, seed=0, pieces=9, faults=()):
    """an fp32 evaluation of the contract: shuffled summation orders, transcendentals perturbed within their budgets, the
    products from bf16 pieces (9 exact, 6 the kernel's scheme, 5 / 1 planted faults); faults: names out of FAULTS"""
    rng = np.random.default_rng(seed)
    ar = F32P(rng, pieces)
    f = lambda a: np.asarray(a, np.float32)
    Y = targets(case['Ypad'], case['hs'].shape[0], case['ldy'], faults)
    r, _ = _values(ar, f(case['hs']), f(case['Wo']), f(case['bo']), f(Y), np.float32(case['scale']), CLIP, faults, rng)
    return r


# ------------------------------------------------------------------------------------------------------- comparison --
def _err(g, rf):
    return np.abs(np.asarray(g, np.float64) - rf)


def ratios(got, ref):
    """worst |got - ref| / bound per output present in got; a NaN, or an error where the bound is 0, gives inf"""
    out = {}
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        e = _err(got[k], ref[k])
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(e == 0, 0.0, e / ref['b_' + k])
        out[k] = float(np.nan_to_num(q, nan=np.inf, posinf=np.inf).max()) if q.size else 0.0
    return out


def rms(got, ref):
    """rms(err / sigma) per output present in got (elements with sigma = 0 and no error do not count; with an error: inf)"""
    out = {}
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        e, s = _err(got[k], ref[k]), ref['s_' + k]
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(e == 0, 0.0, e / s)
        q = np.nan_to_num(q, nan=np.inf, posinf=np.inf)
        n = int(((s > 0) | (e != 0)).sum())
        out[k] = float(np.sqrt(np.square(q).sum() / n)) if n else 0.0
    return out


def violations(got, ref):
    """[(output, worst ratio)] of the outputs with an element beyond its bound"""
    return [(k, v) for k, v in ratios(got, ref).items() if not v <= 1.0]


def rms_violations(got, ref):
    """[('rms ' + output, rms)] of the outputs of at least RMS_MIN elements whose rms(err / sigma) exceeds 1"""
    return [('rms ' + k, v) for k, v in rms(got, ref).items() if np.size(ref[k]) >= RMS_MIN and not v <= 1.0]


def flag_counts(ref):
    return {k: int(np.sum(v)) for k, v in ref['flags'].items()}


def single_ratios(case, got, kernel):
    """single-product cases: worst |got - a b| / (SINGLE[kernel] |a b|) for logits, dhs (from the stored dl) and, at R = 1,
    dWo; 'dbo': the number of entries that differ from dl[0] (R = 1)"""
    perm, v = case['perm'], case['v'].astype(np.float64)
    hs = case['hs'].astype(np.float64)
    dl = np.asarray(got['dl'], np.float64)

    def one(g, want):
        e = _err(g, want)
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(e == 0, 0.0, e / (SINGLE[kernel] * np.abs(want)))
        return float(np.nan_to_num(q, nan=np.inf, posinf=np.inf).max())
    out = dict(logits=one(np.asarray(got['logits'])[:, perm], hs * v), dhs=one(got['dhs'], dl[:, perm] * v))
    if hs.shape[0] == 1:
        out['dWo'] = one(got['dWo'], hs[0][:, None] * dl[0][None, :])
        out['dbo'] = int((np.asarray(got['dbo'], np.float64) != dl[0]).sum())
    return out


def single_violations(case, got, kernel):
    return [(k, v) for k, v in single_ratios(case, got, kernel).items() if not (v == 0 if k == 'dbo' else v <= 1.0)]


# ------------------------------------------------------------------------------------------------------------ cases --
def _f(a):
    return np.asarray(a, np.float32).astype(np.float64)


def pad_targets(Y, ldy, fill=np.nan):
    P = np.full((Y.shape[0], ldy), fill, np.float64)
    P[:, :N] = Y
    return P


def make_case(seed, R, ldy=N, scale=None):
    """the input distribution of test_out_head_train_matches_numpy: hs = tanh(normal), Wo = 0.4 normal with column 3 scaled
    by 30 (logits far outside the clip), bo normal, 10 % notes; all fp32 values.  Ypad: the [R,ldy] array with NaN padding."""
    rng = np.random.default_rng(seed)
    hs = _f(np.tanh(rng.standard_normal((R, N))))
    Wo = rng.standard_normal((N, N)) * 0.4
    Wo[:, 3] *= 30.0
    Y = (rng.random((R, N)) < 0.1).astype(np.float64)
    return dict(hs=hs, Wo=_f(Wo), bo=_f(rng.standard_normal(N)), Y=Y, Ypad=pad_targets(Y, ldy), ldy=ldy,
                scale=float(np.float32(1.0 / R if scale is None else scale)))


EDGE_PTS = np.array([CLIP_HI32, np.nextafter(CLIP_HI32, np.float32(np.inf)), CLIP_LO32, np.nextafter(CLIP_LO32, np.float32(-np.inf)),
                     16.0, 16.1, 15.9, -16.0, -16.2, 30.0, -30.0, 0.0, 3.0, -3.0], np.float32)
EDGE_COL0 = 8                        # the points sit in columns 8 .. 21 of rows 0 (y = 0) and 1 (y = 1)
EDGE_NEAR = 4                        # the first four: on a clip point or one fp32 step outside it -> flagged clip_l
EDGE_ZERO_COL, EDGE_BIG_COL = 50, 3


def edge_case(ldy=N):
    """R = 37, bo = 0.  Rows 0, 1: hs = e_0, so logits = Wo[0] exactly: EDGE_PTS (both clip points, one fp32 step outside each,
    between HI and the symmetric clip's 16.118, far outside) against y = 0 and y = 1; rows 2, 3: hs = 0; row 4: every entry
    1e-30; rows 5..: random with 1e-30 entries in every 7th column.  Wo: column 50 zeros, column 3 scaled by 30."""
    case = make_case(77, 37, ldy, scale=0.37)
    hs, Wo, Y = case['hs'].copy(), case['Wo'].copy(), case['Y'].copy()
    Wo[:, EDGE_ZERO_COL] = 0.0
    Wo[0] = 0.0
    Wo[0, EDGE_COL0:EDGE_COL0 + EDGE_PTS.size] = EDGE_PTS.astype(np.float64)
    hs[:4] = 0.0
    hs[:2, 0] = 1.0
    hs[4] = _f(1e-30)
    hs[5:, ::7] = _f(1e-30)
    Y[0], Y[1] = 0.0, 1.0
    return dict(case, hs=hs, Wo=Wo, bo=np.zeros(N), Y=Y, Ypad=pad_targets(Y, ldy))


def single_case(seed, R, ldy=N, scale=1.0):
    """Wo[h, perm[h]] = v[h], zero elsewhere; bo = 0; |hs v| < 4, inside the clip"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(N)
    v = _f(rng.uniform(0.25, 4.0, N) * rng.choice([-1.0, 1.0], N))
    Wo = np.zeros((N, N))
    Wo[np.arange(N), perm] = v
    hs = _f(np.tanh(rng.standard_normal((R, N))))
    Y = (rng.random((R, N)) < 0.3).astype(np.float64)
    return dict(hs=hs, Wo=Wo, bo=np.zeros(N), Y=Y, Ypad=pad_targets(Y, ldy), ldy=ldy, scale=float(np.float32(scale)),
                perm=perm, v=v)


# The random cases of tests/test_gpu_out_head.py: (R, kernel, what selects it, target pitch, stored, scale, reductions).
#   kernel 'bf16': everything 16-byte aligned and ldy % 4 == 0; 'f32' by `how`: 'ldy' (pitch 89 / 91), or the named pointer
#   one float past a 16-byte boundary.  stored: 'both' / 'logits' / 'dlogits' / 'none'.  scale: None = 1 / R.
#   reductions: 'i' immediate, 'd' a deferred job flushed through ops.ReduceQueue.
# Not a cross product: every value of every axis at least once per kernel; the row counts around 128 and 32768 with both
# kinds of reduction.  The largest R runs once per kernel.
S_ODD = 0.0123456
GPU_CASES = [
    (1, 'bf16', None, 88, 'both', None, 'id'), (1, 'f32', 'ldy', 89, 'both', None, 'id'),
    (15, 'bf16', None, 92, 'logits', 1.0, 'i'), (15, 'f32', 'dhs', 88, 'dlogits', S_ODD, 'd'),
    (16, 'bf16', None, 96, 'dlogits', S_ODD, 'd'), (16, 'f32', 'ldy', 91, 'logits', 1.0, 'i'),
    (17, 'bf16', None, 88, 'none', None, 'i'), (17, 'f32', 'Y', 88, 'none', None, 'i'),
    (127, 'bf16', None, 92, 'both', None, 'id'), (127, 'f32', 'logits', 88, 'both', None, 'id'),
    (128, 'bf16', None, 88, 'both', 1.0, 'id'), (128, 'f32', 'ldy', 89, 'both', 1.0, 'id'),
    (129, 'bf16', None, 96, 'both', None, 'id'), (129, 'f32', 'dlogits', 88, 'both', None, 'id'),
    (1000, 'bf16', None, 88, 'dlogits', None, 'd'), (1000, 'f32', 'ldy', 91, 'logits', S_ODD, 'd'),
    (32767, 'bf16', None, 88, 'both', None, 'i'), (32767, 'f32', 'ldy', 89, 'both', None, 'd'),
    (32768, 'bf16', None, 92, 'both', None, 'd'), (32768, 'f32', 'dhs', 88, 'both', None, 'i'),
    (32769, 'bf16', None, 88, 'both', None, 'id'), (32769, 'f32', 'ldy', 91, 'both', None, 'id'),
    (32768 + 129, 'bf16', None, 96, 'both', None, 'd'), (32768 + 129, 'f32', 'Y', 88, 'both', None, 'i'),
    (128 * 513 + 7, 'bf16', None, 88, 'both', None, 'd'), (128 * 513 + 7, 'f32', 'ldy', 89, 'both', None, 'd'),
]


def gpu_case(R, ldy, scale):
    return make_case(5000 + R, R, ldy, scale)
