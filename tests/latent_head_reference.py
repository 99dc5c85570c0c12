"""fp64 reference of the latent head of cl_vrnn (include/clvae.h, above clv_latent_head_supported: clv_latent_head_fwd,
clv_latent_head_bwd; H = 88, 1 <= L <= 32).

Written from the header's contract, not from the kernels' structure:
  forward   zargs = hs.Wz + bz                                               [R,2L] = (mean | log_var)
            Z     = mean + exp(log_var / 2) eps                              [R,L]
            rowkl = -0.5 sum_l (1 + log_var - mean^2 - exp(log_var))         [R]
  backward  (zargs an exact fp32 INPUT, as the entry point takes it)
            dzargs = (dZ + kl mean | dZ eps sd / 2 - kl (1 - sd^2) / 2),  sd = exp(log_var / 2)     [R,2L]
            dhs = dzargs.Wz^T  [R,88],   dWz = hs^T.dzargs  [88,2L],   dbz = sum_r dzargs  [2L]

Bounds.  As tests/vae_reference.py and tests/out_head_reference.py (U, KAPPA, EXP_ULP are imported from there): beside every
output element a first-order standard error sigma ('s_' + name) of an honest fp32 evaluation of the contract; the element's
bound ('b_' + name) is KAPPA sigma.
  * a dot product of n terms: (U sum|terms|)^2 n / 3 for its roundings plus (U |result|)^2; n = 89 for zargs (88 products and
    the bias), 2L for dhs, R + 1 for dWz and dbz, L for rowkl;
  * expf (the device code is compiled without fast-math: the precise one): EXP_ULP ulp of the result plus |x| U for the
    argument; every other fp32 operation one U of its result;
  * Z = m + sd eps: zargs' variance through the first derivative (1 for the mean, sd eps / 2 for log_var), sd's own
    budget, the product's and the sum's rounding;
  * rowkl: exp(log_var) may be formed as sd^2, so sd's relative error counts DOUBLE (2 (EXP_ULP + |lv| / 2) U sd^2); the
    terms 1, lv, m^2, sd^2 each with their roundings (4 U of their absolute sum), the L-term sum; zargs' variance through
    d/dm = -m ... 2 m, d/dlv = 1 - sd^2 (times the 0.5 in front);
  * dzargs: the mean half d + kl m rounds twice (the product, the sum): U (|d| + 2 |kl m|).  The log_var half
    t1 - t2, t1 = d eps sd / 2, t2 = kl (1 - sd^2) / 2: the roundings of both chains (U (4 |t1| + 3 |t2| + |kl| sd^2): the
    cancellation in 1 - sd^2 is carried as an ABSOLUTE term in sd^2, not relative to the difference) and sd's budget, which
    reaches t1 once and sd^2 twice ((EXP_ULP + |lv| / 2) U (|t1| + |kl| sd^2));
  * dzargs' variance reaches dhs, dWz and dbz through the first derivative (Wz^T, hs, 1).
The elementwise budgets are sums of worst cases used as ONE standard error (no distribution assumed); the dot products'
roundings are independent and add in variance.
Criteria: `violations` (any element beyond its bound; a NaN counts) and, per output tensor of at least RMS_MIN elements,
rms(err / sigma) <= 1 (`rms_violations`): sigma is an upper estimate of the standard error, so an honest evaluation stays
below 1, while a small systematic fault that no single element betrays can raise the rms above it.
Nothing here is fitted to errors seen on a GPU; tests/test_latent_head_reference.py checks the bounds against fp32
evaluations of the contract (`evaluate32`) and that planted faults (FAULTS) are rejected.
NOT covered: denormal intermediates (no case produces one; the matrix cores may flush them).
"""
import numpy as np

from vae_reference import U, KAPPA, EXP_ULP

H = 88                                   # hidden units of the encoder LSTM
OUTPUTS = ('zargs', 'Z', 'rowkl', 'dzargs', 'dhs', 'dWz', 'dbz')
FWD, BWD = OUTPUTS[:3], OUTPUTS[3:]
RMS_MIN = 1000                           # the rms criterion is enforced for tensors of at least this many elements
BLOCK, TILE, GRID = 128, 16, 256         # rows per block, rows per wave, the most workgroups (the shapes' boundaries; the
                                         # reference itself uses none of them, the planted faults do)


def lp16(L):
    """16-column tiles per half of the head (the kernels' template parameter)"""
    return 1 if L <= 16 else 2


# ------------------------------------------------------------------------------------------------------- arithmetic --
class A64:
    dt = np.float64
    c = staticmethod(lambda a: np.asarray(a, np.float64))
    dot = staticmethod(lambda A, B, cs=None: A @ B)
    colsum = staticmethod(lambda A: A.sum(0))
    rowsum = staticmethod(lambda A: A.sum(-1))
    exp = staticmethod(np.exp)


class A32:
    """an fp32 evaluation: every product and sum rounded to fp32.  order 'seq': sums run in index order; 'pair': in chunks
    (8 per short dot product, BLOCK rows per chunk of a sum over the rows) that are added in a pairwise tree.  rng: expf
    perturbed within its budget (uniformly, independently per element); None: the correctly rounded value."""
    dt = np.float32

    def __init__(self, order='seq', rng=None):
        assert order in ('seq', 'pair')
        self.order, self.rng = order, rng

    def c(self, a):
        return np.asarray(a, np.float32)

    def _chunks(self, K, cs):
        if self.order == 'seq':
            return K
        return cs if cs is not None else -(-K // 8)

    def _tree(self, acc):
        while acc.shape[0] > 1:
            n = acc.shape[0]
            head = acc[:n // 2 * 2:2] + acc[1:n // 2 * 2:2]
            acc = head if n % 2 == 0 else np.concatenate([head, acc[-1:]])
        return acc[0]

    def dot(self, A, B, cs=None):
        """A [M,K] . B [K,N]; cs: chunk length of the 'pair' order (None: K / 8)"""
        A, B = self.c(A), self.c(B)
        K = A.shape[1]
        cs = self._chunks(K, cs)
        nc = -(-K // cs) if K else 1
        acc = np.zeros((nc, A.shape[0], B.shape[1]), np.float32)
        AT = np.ascontiguousarray(A.T)
        for i in range(min(cs, K)):
            ks = np.arange(i, K, cs)
            acc[:len(ks)] = acc[:len(ks)] + AT[ks][:, :, None] * B[ks][:, None, :]
        return self._tree(acc)

    def colsum(self, A):
        A = self.c(A)
        return self.dot(A.T, np.ones((A.shape[0], 1), np.float32), cs=BLOCK)[:, 0]

    def rowsum(self, A):
        A = self.c(A)
        return self.dot(A, np.ones((A.shape[1], 1), np.float32))[:, 0]

    def exp(self, x):
        x64 = self.c(x).astype(np.float64)
        with np.errstate(over='ignore'):
            e = np.exp(x64)
            if self.rng is not None:
                e = e * (1.0 + self.rng.uniform(-1.0, 1.0, x64.shape) * (EXP_ULP + np.abs(x64)) * U)
            return self.c(e)


# ----------------------------------------------------------------------------------------------------------- values --
FAULTS = ('wave_dropped', 'round2_dropped', 'dbz_beyond_R', 'dWz_beyond_R',                              # accumulation, masking
          'lv_from_mean_col', 'padded_col', 'eps_row_plus1', 'Z_pitch_L', 'dZ_pitch_L', 'dhs_Wz_not_T',   # operand, pitch
          'kl_exp_half', 'Z_exp_full', 'kl_half_missing', 'kl_sign', 'kl_on_dZ', 'bias_tile',            # arithmetic
          'stale_hs_fwd', 'stale_hs_bwd', 'slab_dropped')                                                # loop, slabs


def _strided(flat, R, L, pitch, col0=0):
    """[R,L] read out of a flat buffer at `pitch` (indices beyond the buffer: its last element)"""
    idx = np.arange(R)[:, None] * pitch + np.arange(L)[None, :] + col0
    return flat[np.minimum(idx, flat.size - 1)]


def _stale(hs, grid):
    """hs with the rows of every block after a workgroup's first replaced by the rows of the workgroup's block before"""
    R = hs.shape[0]
    r = np.arange(R)
    src = np.where(r // BLOCK >= grid, r - grid * BLOCK, r)
    return hs[src]


def forward_values(ar, hs, Wz, bz, eps, ldz=None, faults=(), grid=GRID):
    """zargs, Z (as the [R,ldz] buffer's first L columns), rowkl in arithmetic `ar`"""
    c = ar.c
    hs, Wz, bz, eps = c(hs), c(Wz), c(bz), c(eps)
    R, L = hs.shape[0], Wz.shape[1] // 2
    ldz = L if ldz is None else ldz
    if 'bias_tile' in faults:                      # the last 16-column tile of the mean half
        bz = bz.copy()
        bz[16 * (lp16(L) - 1):L] = 0
    if 'eps_row_plus1' in faults:
        eps = eps[np.minimum(np.arange(R) + 1, R - 1)]
    hz = _stale(hs, grid) if 'stale_hs_fwd' in faults else hs
    zargs = ar.dot(hz, Wz) + bz
    m, lv = zargs[:, :L], zargs[:, L:]
    if 'lv_from_mean_col' in faults:
        lv = m
    if 'padded_col' in faults:                     # log_var stored at, and taken from, column 16 LP16 + c of the row
        zf = np.full(R * 2 * L + 32, np.nan, ar.dt)
        zf[(np.arange(R)[:, None] * 2 * L + np.arange(L)[None, :]).ravel()] = m.ravel()
        zf[(np.arange(R)[:, None] * 2 * L + 16 * lp16(L) + np.arange(L)[None, :]).ravel()] = lv.ravel()
        zargs = zf[:R * 2 * L].reshape(R, 2 * L)
    with np.errstate(over='ignore', invalid='ignore'):
        sd = ar.exp(c(0.5) * lv)
        sz = ar.exp(lv) if 'Z_exp_full' in faults else sd
        Z = m + sz * eps
        ex = sd if 'kl_exp_half' in faults else sd * sd
        f = c(-1.0 if 'kl_half_missing' in faults else -0.5) * c(-1.0 if 'kl_sign' in faults else 1.0)
        rowkl = f * ar.rowsum(c(1.0) + lv - m * m - ex)
    Zb = np.full(R * ldz + L, np.nan, ar.dt)
    pitch = L if 'Z_pitch_L' in faults else ldz
    Zb[(np.arange(R)[:, None] * pitch + np.arange(L)[None, :]).ravel()] = Z.ravel()
    return dict(zargs=zargs, Z=Zb[:R * ldz].reshape(R, ldz)[:, :L], rowkl=rowkl)


def backward_values(ar, hs, Wz, zargs, eps, dZpad, kl, faults=(), grid=GRID):
    """dzargs, dhs, dWz, dbz in arithmetic `ar`; dZpad: the [R,lddz] buffer (padding columns: anything)"""
    c = ar.c
    hs, Wz, zargs, eps, dZpad = c(hs), c(Wz), c(zargs), c(eps), c(dZpad)
    R, L = hs.shape[0], Wz.shape[1] // 2
    kl = c(kl)
    d = _strided(dZpad.reshape(-1), R, L, L if 'dZ_pitch_L' in faults else dZpad.shape[1])
    if 'eps_row_plus1' in faults:
        eps = eps[np.minimum(np.arange(R) + 1, R - 1)]
    m, lv = zargs[:, :L], zargs[:, L:]
    if 'lv_from_mean_col' in faults:
        lv = m
    if 'padded_col' in faults:
        lv = _strided(zargs.reshape(-1), R, L, 2 * L, 16 * lp16(L))
    with np.errstate(over='ignore', invalid='ignore'):
        sd = ar.exp(c(0.5) * lv)
        sz = ar.exp(lv) if 'Z_exp_full' in faults else sd
        ex = sd if 'kl_exp_half' in faults else sd * sd
        h = c(1.0 if 'kl_half_missing' in faults else 0.5) * c(-1.0 if 'kl_sign' in faults else 1.0)
        km = -kl if 'kl_sign' in faults else kl
        dm = d + km * m
        dl = d * eps * c(0.5) * sz - h * kl * (c(1.0) - ex)
        if 'kl_on_dZ' in faults:
            dm = kl * d + km * m
            dl = kl * (d * eps * c(0.5) * sz) - h * kl * (c(1.0) - ex)
        dz = np.concatenate([dm, dl], 1).astype(ar.dt)
        WT = Wz.reshape(2 * L, H) if 'dhs_Wz_not_T' in faults else Wz.T
        dhs = ar.dot(dz, WT)
    gh, gd = (_stale(hs, grid) if 'stale_hs_bwd' in faults else hs), dz
    keep = np.ones(R, bool)
    if 'wave_dropped' in faults:                   # the second wave of the first block
        assert R >= 2 * TILE
        keep[TILE:2 * TILE] = False
    if 'slab_dropped' in faults:                   # the blocks of workgroup 1
        assert R > BLOCK
        keep[(np.arange(R) // BLOCK) % grid == 1] = False
    gh, gd = gh[keep], gd[keep]
    extra = (-R) % TILE                            # the rows that a ragged last tile clamps to row R - 1
    with np.errstate(over='ignore', invalid='ignore'):
        if 'dWz_beyond_R' in faults:
            assert extra
            dWz = ar.dot(np.concatenate([gh, np.repeat(hs[-1:], extra, 0)]).T, np.concatenate([gd, np.repeat(dz[-1:], extra, 0)]), cs=BLOCK)
        else:
            dWz = ar.dot(gh.T, gd, cs=BLOCK)
        if 'dbz_beyond_R' in faults:
            assert extra
            dbz = ar.colsum(np.concatenate([gd, np.repeat(dz[-1:], extra, 0)]))
        else:
            dbz = ar.colsum(gd)
    if 'round2_dropped' in faults:
        assert L > 16
        dWz, dbz = dWz.copy(), np.zeros_like(dbz)
        dWz[48:] = 0
    return dict(dzargs=dz, dhs=dhs, dWz=dWz, dbz=dbz)


# -------------------------------------------------------------------------------------------------------- reference --
def _finish(r, var):
    for name, v in var.items():
        r['s_' + name] = np.sqrt(v)
        r['b_' + name] = KAPPA * r['s_' + name]
    return r


def forward_reference(hs, Wz, bz, eps):
    """the fp64 forward reference: zargs, Z, rowkl, 's_' + name, 'b_' + name.  The inputs hold fp32 values."""
    hs, Wz, bz, eps = [np.asarray(a, np.float64) for a in (hs, Wz, bz, eps)]
    L = Wz.shape[1] // 2
    r = forward_values(A64, hs, Wz, bz, eps)
    A, sq = np.abs, np.square
    v_za = sq(U * (A(hs) @ A(Wz) + A(bz))) * (H + 1) / 3.0 + sq(U * A(r['zargs']))
    m, lv = r['zargs'][:, :L], r['zargs'][:, L:]
    vm, vlv = v_za[:, :L], v_za[:, L:]
    sd = np.exp(0.5 * lv)
    se = sd * eps
    bud = (EXP_ULP + 0.5 * A(lv)) * U                                       # expf's relative budget at lv / 2
    v_z = vm + sq(se) * (0.25 * vlv + sq(bud)) + sq(U * A(se)) + sq(U * A(r['Z']))
    tk = 1 + A(lv) + m * m + sd * sd
    v_kl = 0.25 * ((4 * sq(m) * vm + sq(1 - sd * sd) * vlv).sum(1) + (sq(4 * U * tk) + sq(2 * bud * sd * sd)).sum(1)
                   + sq(U * tk.sum(1)) * L / 3.0)
    return _finish(r, dict(zargs=v_za, Z=v_z, rowkl=v_kl))


def backward_reference(hs, Wz, zargs, eps, dZ, kl):
    """the fp64 backward reference from zargs as an exact fp32 input: dzargs, dhs, dWz, dbz and their sigmas and bounds.
    dZ: [R,L] (the values, without padding columns)"""
    hs, Wz, zargs, eps, dZ = [np.asarray(a, np.float64) for a in (hs, Wz, zargs, eps, dZ)]
    R, L = hs.shape[0], Wz.shape[1] // 2
    kl = float(np.float32(kl))
    r = backward_values(A64, hs, Wz, zargs, eps, dZ, kl)
    A, sq = np.abs, np.square
    m, lv = zargs[:, :L], zargs[:, L:]
    sd = np.exp(0.5 * lv)
    t1 = dZ * eps * 0.5 * sd
    t2 = 0.5 * kl * (1 - sd * sd)
    ks2 = A(kl) * sd * sd
    bud = (EXP_ULP + 0.5 * A(lv)) * U
    v_dm = sq(U * (A(dZ) + 2 * A(kl * m)))
    v_dl = sq(U * (4 * A(t1) + 3 * A(t2) + ks2)) + sq(bud * (A(t1) + ks2))
    v_dz = np.concatenate([v_dm, v_dl], 1)
    dz = r['dzargs']
    v_dhs = v_dz @ sq(Wz.T) + sq(U * (A(dz) @ A(Wz.T))) * (2 * L) / 3.0 + sq(U * A(r['dhs']))
    v_dWz = sq(hs).T @ v_dz + sq(U * (A(hs).T @ A(dz))) * (R + 1) / 3.0 + sq(U * A(r['dWz']))
    v_dbz = v_dz.sum(0) + sq(U * A(dz).sum(0)) * (R + 1) / 3.0 + sq(U * A(r['dbz']))
    return _finish(r, dict(dzargs=v_dz, dhs=v_dhs, dWz=v_dWz, dbz=v_dbz))


def f32(a):
    """the fp32 rounding of `a`, held in fp64"""
    return np.asarray(a, np.float32).astype(np.float64)


def ref_case(case, zargs=None, eps=None, backward=True):
    """forward and backward reference of a case in one dict; 'zargs32': the backward pass's input (default: the forward
    reference's zargs rounded to fp32).  eps: other noise than the case's (what a launch drew)."""
    eps = case['eps'] if eps is None else np.asarray(eps, np.float64)
    r = forward_reference(case['hs'], case['Wz'], case['bz'], eps)
    r['zargs32'] = f32(r['zargs']) if zargs is None else np.asarray(zargs, np.float64)
    if backward:
        r.update(backward_reference(case['hs'], case['Wz'], r['zargs32'], eps, case['dZ'], case['kl']))
    return r


def evaluate32(case, order='seq', seed=None, faults=(), zargs=None, grid=GRID):
    """an fp32 evaluation of the contract (see A32); zargs: the backward pass's input (None: this evaluation's own, as a
    training step chains the two); faults: names out of FAULTS"""
    ar = A32(order, None if seed is None else np.random.default_rng(seed))
    out = forward_values(ar, case['hs'], case['Wz'], case['bz'], case['eps'], case['ldz'], faults, grid)
    za = out['zargs'] if zargs is None else zargs
    out.update(backward_values(ar, case['hs'], case['Wz'], za, case['eps'], case['dZpad'], case['kl'], faults, grid))
    return out


# ------------------------------------------------------------------------------------------------------- comparison --
def _err(g, rf):
    return np.abs(np.asarray(g, np.float64) - rf)


def ratios(got, ref):
    """worst |got - ref| / bound per output present in got; a NaN, or an error where the bound is 0, gives inf"""
    out = {}
    for k in OUTPUTS:
        if got.get(k) is None or k not in ref:
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
        if got.get(k) is None or k not in ref:
            continue
        e, s = _err(got[k], ref[k]), ref['s_' + k]
        with np.errstate(divide='ignore', invalid='ignore'):
            q = np.where(e == 0, 0.0, e / s)
        q = np.nan_to_num(q, nan=np.inf, posinf=np.inf)
        n = int(((s > 0) | (e != 0)).sum())
        with np.errstate(over='ignore'):
            out[k] = float(np.sqrt(np.square(q).sum() / n)) if n else 0.0
    return out


def violations(got, ref):
    """[(output, worst ratio)] of the outputs with an element beyond its bound"""
    return [(k, v) for k, v in ratios(got, ref).items() if not v <= 1.0]


def rms_violations(got, ref):
    """[('rms ' + output, rms)] of the outputs of at least RMS_MIN elements whose rms(err / sigma) exceeds 1"""
    return [('rms ' + k, v) for k, v in rms(got, ref).items() if np.size(ref[k]) >= RMS_MIN and not v <= 1.0]


# ------------------------------------------------------------------------------------------------------------ cases --
HS_BIG_COL, HS_BIG = 7, 4.0              # hidden column 7 of hs scaled by 4: its term dominates many sums over the units
WZ_BIG = 5.0                             # one column of the mean half of Wz scaled by 5: it dominates sums over the head columns
KL_C = 0.37                              # kl_scale = KL_C / R (engine.py:_latent_bwd: kl_weight / (B T))


def pad(a, ld, fill=np.nan):
    P = np.full((a.shape[0], ld), fill, np.float64)
    P[:, :a.shape[1]] = a
    return P


def _assert_finite32(case):
    """every value of the fp64 evaluation is finite in fp32"""
    fw = forward_values(A64, case['hs'], case['Wz'], case['bz'], case['eps'])
    bw = backward_values(A64, case['hs'], case['Wz'], f32(fw['zargs']), case['eps'], case['dZ'], case['kl'])
    with np.errstate(over='ignore'):
        for k, v in list(fw.items()) + list(bw.items()):
            assert np.isfinite(np.asarray(v, np.float32)).all(), k
    return fw


def make_case(seed, R, L, wide=False, ldz=None, lddz=None, kl=None):
    """all fp32 values: hs = tanh(normal) with column HS_BIG_COL scaled by HS_BIG; Wz: mean half 0.2 normal with column
    min(3, L - 1) scaled by WZ_BIG, log_var half 0.06 normal (log_var roughly -1 .. 1) or, wide, 0.45 normal (-8 .. 8); bz
    0.3 normal; eps normal; dZ = normal / R in an [R,lddz] buffer with NaN padding; kl_scale = KL_C / R."""
    rng = np.random.default_rng(seed)
    hs = np.tanh(rng.standard_normal((R, H)))
    hs[:, HS_BIG_COL] *= HS_BIG
    Wz = rng.standard_normal((H, 2 * L))
    Wz[:, :L] *= 0.2
    Wz[:, L:] *= 0.45 if wide else 0.06
    Wz[:, min(3, L - 1)] *= WZ_BIG
    ldz, lddz = ldz or L, lddz or L
    dZ = f32(rng.standard_normal((R, L)) / R)
    case = dict(R=R, L=L, hs=f32(hs), Wz=f32(Wz), bz=f32(rng.standard_normal(2 * L) * 0.3), eps=f32(rng.standard_normal((R, L))),
                dZ=dZ, dZpad=pad(dZ, lddz), ldz=ldz, lddz=lddz, kl=float(np.float32(KL_C / R if kl is None else kl)))
    _assert_finite32(case)
    return case


EDGE_R = 150
EDGE_LV = 40.0


def edge_case(L=9, kl_zero=False, ldz=None, lddz=None):
    """R = 150 (two blocks, a ragged tile).  Head column 0: Wz[:, L] = 40 e_0 and bz[L] = 0, so log_var = 40 hs[r, 0] is ONE
    product, hs[:, 0] spread over -1 .. 1 with both ends present: sd^2 from e^-40 = 4e-18 to e^40 = 2e17, finite in fp32.
    Head column 1 (L >= 2): a zero mean column and bias: mean = 0 exactly, and log_var = -40 from the bias alone
    (Wz[:, L + 1] = 0).  Rows 0..19: eps = 0; rows 10..39: dZ = 0 (the KL terms alone); kl_zero: kl_scale = 0 (the dZ terms
    alone).  The other columns: the wide random case."""
    case = make_case(4242, EDGE_R, L, wide=True, ldz=ldz, lddz=lddz)
    hs, Wz, bz, eps, dZ = [case[k].copy() for k in ('hs', 'Wz', 'bz', 'eps', 'dZ')]
    hs[:, 0] = f32(np.linspace(-1.0, 1.0, EDGE_R))
    Wz[:, L] = 0.0
    Wz[0, L] = EDGE_LV
    bz[L] = 0.0
    if L >= 2:
        Wz[:, 1] = 0.0
        bz[1] = 0.0
        Wz[:, L + 1] = 0.0
        bz[L + 1] = -EDGE_LV
    eps[:20] = 0.0
    dZ[10:40] = 0.0
    case = dict(case, hs=hs, Wz=Wz, bz=bz, eps=eps, dZ=dZ, dZpad=pad(dZ, case['lddz']), kl=0.0 if kl_zero else case['kl'])
    fw = _assert_finite32(case)
    lv0 = fw['zargs'][:, L]
    assert lv0[0] == -EDGE_LV and lv0[-1] == EDGE_LV
    assert L < 2 or ((fw['zargs'][:, 1] == 0).all() and (fw['zargs'][:, L + 1] == -EDGE_LV).all())
    return case


# The cases of tests/test_gpu_latent_head.py: (R, L, ldz, lddz, wide, reductions 'i' | 'd', dzargs stored, rowkl present,
# misaligned: Wz, bz, eps, zargs, Z, dZ, dzargs, dhs each one float past a 16-byte boundary).
# R on the wave tile (16), the block (128) and the grid cap (256 workgroups): 1, 2 and 3 blocks per workgroup, the last block
# holding 1 or 7 rows.  Not a cross product: each list is walked at its own stride, so that every L (both templates) meets
# every kind of R, and every other axis takes every value with both templates.  The two largest R run with four L only.
RS_SMALL = (1, 15, 16, 17, 127, 128, 129, 300)
RS_LARGE = (BLOCK * GRID + 1, BLOCK * 513 + 7)
LS = (1, 2, 4, 9, 15, 16, 17, 24, 31, 32)
LS_LARGE = (9, 16, 17, 32)
PADS = (0, 3, 8)


def _gpu_cases():
    out = []
    for i, R in enumerate(RS_SMALL):
        for j in range(4):
            n = 4 * i + j
            L = LS[(3 * n) % 10]                     # 3 and 10 coprime: every L; {b, b + 3, b + 6, b + 9} holds both templates
            out.append((R, L, L + PADS[n % 3], L + PADS[(n // 2 + j) % 3], (i + j) % 2 == 1, 'id'[(n // 3) % 2],
                        (n // 2) % 2 == 0, (i + j // 2) % 2 == 0, n % 3 == 1))
    for i, R in enumerate(RS_LARGE):
        for j, L in enumerate(LS_LARGE):
            n = 4 * i + j
            out.append((R, L, L + PADS[(n + 1) % 3], L + PADS[(n // 2 + j) % 3], j % 2 == 1, 'id'[(i + j // 2) % 2],
                        (i + j) % 2 == 0, j < 2 or i == 1, j == 3 - 2 * i))
    return out


GPU_CASES = _gpu_cases()


def gpu_case(R, L, ldz, lddz, wide):
    return make_case(7000 + 37 * R + L, R, L, wide, ldz, lddz)
