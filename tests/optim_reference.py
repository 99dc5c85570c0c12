"""fp64 reference of ONE optimizer step over the flat buffers (include/clvae.h: clv_adam_wn_step, clv_adam_known_sums,
CLV_OPT_*, the step_t rules), with a bound beside every output element.

Written from the header's contract and from oracle.adam_wn_step / oracle.rmsprop_step, not from the kernels' structure:
  t      = counter + 1 ('advance', 'readonly'), counter ('advanced': CLV_STEP_ADVANCED), or given (('explicit', t), no counter)
  lr_t   = lr sqrt(1 - b2^t) / (1 - b1^t)
  CLV_OPT_ADAM_WN, a matrix, per column:  V = W / s,  A = sum_r V^2,  B = sum_r g V,  Vn = sqrt(A),  grad_g = B / Vn,
      gov = grad_g / Vn,  grad_V = s (g - gov V);  Adam on the gain s Vn with (mg, vg) and on V with (m, v);
      C = sum_r V'^2,  s' = g' / sqrt(C),  W' = s' V';  a matrix of more than 144 rows also leaves vn2' = C when the call was
      given the vnorm2 array (known is not None)
  the known-sums form (known['use']): A and B are INPUTS, A = vn2, B = gdot / s;  true_sums() gives what they should be
  a bias, and every tensor under CLV_OPT_ADAM: plain Adam;  CLV_OPT_RMSPROP: a' = b2 a + (1 - b2) g^2 in `v`,
      p' = p - lr g / (sqrt(a') + eps), `m` untouched
The state goes in exactly as it is stored (fp32 flat arrays, FlatParams' layout: layout()); every output comes back in fp64
as a whole flat array, padding included, so that "what a step must not touch" is the same comparison: the bound there is 0.
A multi-step test restarts the reference at every step from the state read back from the device.

Bounds.  As tests/vae_reference.py and tests/out_head_reference.py (U, KAPPA imported from there): beside every output
element a first-order standard error sigma ('s_' + name) of an fp32 evaluation of the contract; the bound ('b_' + name) is
KAPPA sigma.  Terms:
  * V = W (1 / s): two roundings;
  * the column sums A, B, C of n = rows terms, fp32 accumulation in any order: (U sum|terms|)^2 n / 3, the terms' own
    roundings, the result's; the operands' variance through the first derivative.  Known sums: A exact, B one rounding;
  * gov = B / A: dB / A and B dA / A^2 (the error of Vn enters twice, coherently);
  * the cancellation in grad_V = s (g - gov V): the roundings of gov V and of the difference are relative to the operands,
    not to the result; the error of gov is common to a column and is carried coherently into C.  v' takes grad_V squared:
    beside the first-order term 2 grad_V d its bound carries the second-order one, (1 - b2) d^2 <= (1 - b2) (KAPPA sigma)^2,
    which is all there is where grad_V is an exact 0 in exact arithmetic (a one-row matrix);
  * m / (sqrt(v) + eps): grad_V's variance through d upd / d grad_V = lr_t [(1 - b1) / den - m' (1 - b2) grad_V / (sqrt(v') den^2)],
    the roundings of m' and v' through d/dm and d/dv.  Where v' ~ 0 those derivatives are unbounded, the update is not:
    |m'| / sqrt(v') <= CAP = (1 - b1) / sqrt((1 - b2)(1 - b1^2 / b2)) for any history (Cauchy-Schwarz over the two geometric
    series; RMSprop: 1 / sqrt(1 - b2)), so the bound of an update never exceeds 2 lr_t CAP;
  * s' = g' / sqrt(C), W' = s' V': the variances of g', C, V' and the roundings; on re-entry V = W / s is two roundings again;
  * lr_t: powf within POW_ULP ulp (1 ulp <= 2 U relative), so 1 - b^t is off by up to 2 U POW_ULP b^t / (1 - b^t) relative (at
    t = 1, b2 = 0.999: 1.9e-3, the four digits that the cancellation costs), halved by the square root, plus the square
    root, the division and the product: rel_lr(t).  It is a worst case, common to every element, and enters sigma^2 whole
    (as DROP does in out_head_reference).  The test of lr_t by itself holds the device to rel_lr(t) plus the six roundings
    of the update itself.
    POW_ULP = 16: no accuracy table of the device's math library is installed with the compiler's documentation, so
    this is OpenCL full profile's figure for pow.  Measured on an MI355X (tests/test_gpu_optim.py, lr_t by itself): worst
    observed error 0.136 of that bound (t = 1 .. 10^6, b2 = 0.999 and 0.9).
Nothing here is fitted to errors seen on a GPU.

Criteria: `violations` (any element beyond its bound; a NaN counts; an element the step does not own has bound 0) and
rms(err / sigma) <= 1 per output and tensor of at least RMS_MIN elements (`rms_violations`).
Insensitive elements: bound of params' above INSENS lr_t (cancelling grad_V, v ~ 0).  tests/test_optim_reference.py asserts
that they are at most 1 % of params' in every case of GPU_CASES; DEGENERATE_CASES (one-row matrices, whose grad_V is
rounding noise around an exact 0; all-zero gradients) cannot stay within that and are held to finiteness, the exact zeros
the contract implies and the bounds of m', v' only.
"""
import collections

import numpy as np

from vae_reference import U, KAPPA

POW_ULP = 16
RMS_MIN = 1000
INSENS = 0.1
TALL_ROWS = 144                          # "more than 144 rows" (include/clvae.h)
OPT_ADAM, OPT_ADAM_WN, OPT_RMSPROP = 0, 1, 2
STEP_READONLY, STEP_ADVANCED = -1, -2
SENTINEL = 4321.0                        # helpers.CANARY: what the padding floats and columns hold
FLAT = ('params', 'm', 'v')
COLS = ('mg', 'vg', 's', 'vn2')
OUTPUTS = FLAT + COLS

Desc = collections.namedtuple('Desc', 'name shape offset rows cols col_offset is_matrix')


def f32(x):
    return float(np.float32(x))


def layout(shapes):
    """FlatParams' layout rules (params.py): offsets and column offsets padded to 4 floats, a bias is 1 x n with column
    offset 0, the column arrays hold at least 4 floats.  Returns (table, n, n_cols)."""
    table, off, col = [], 0, 0
    for name, shp in shapes:
        n = int(np.prod(shp))
        is_mat = len(shp) > 1
        rows = int(np.prod(shp[:-1])) if is_mat else 1
        table.append(Desc(name, tuple(shp), off, rows, int(shp[-1]), col if is_mat else 0, int(is_mat)))
        if is_mat:
            col += (int(shp[-1]) + 3) // 4 * 4
        off += (n + 3) // 4 * 4
    return table, off, max(col, 4)


def is_tall(d):
    return bool(d.is_matrix) and d.rows > TALL_ROWS


def hyper(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, opt=OPT_ADAM_WN):
    return dict(lr=f32(lr), b1=f32(b1), b2=f32(b2), eps=f32(eps), opt=int(opt))


def step_of(counter, mode):
    """(t, counter afterwards) by the step_t rules"""
    if isinstance(mode, tuple):
        return int(mode[1]), None
    if mode == 'advance':
        return counter + 1, counter + 1
    if mode == 'readonly':
        return counter + 1, counter
    if mode == 'advanced':
        return counter, counter
    raise ValueError(mode)


def lr_t64(h, t):
    return h['lr'] * np.sqrt(1.0 - h['b2'] ** t) / (1.0 - h['b1'] ** t)


def rel_lr(h, t):
    """relative bound of an fp32 lr_t (docstring)"""
    p1, p2 = h['b1'] ** t, h['b2'] ** t
    one = lambda p: 2 * U * POW_ULP * p / (1.0 - p) + U
    return 0.5 * one(p2) + one(p1) + 3 * U


def cap(h):
    if h['opt'] == OPT_RMSPROP:
        return 1.0 / np.sqrt(1.0 - h['b2'])
    b1, b2 = h['b1'], h['b2']
    q = 1.0 - b1 * b1 / b2
    return (1.0 - b1) / np.sqrt((1.0 - b2) * q) if q > 0 else np.inf


# -------------------------------------------------------------------------------------------------------- reference --
def _ema(b, x, y, vy, square):
    """x' = b x + (1 - b) y  (square: y^2) and its variance: y's through the derivative, two or three products, the sum"""
    t = (1.0 - b) * (y * y if square else y)
    out = b * x + t
    d = (1.0 - b) * (2.0 * y if square else 1.0)
    return out, d * d * vy + U * U * ((b * x) ** 2 + (2 if square else 1) * t * t + out * out), d


def _upd(mn, vm, vn, vv, lr_t, eps, rl, vcap):
    """upd = lr_t mn / (sqrt(vn) + eps) with independent variances of mn, vn"""
    sq = np.sqrt(vn)
    den = sq + eps
    upd = lr_t * mn / den
    d_m = lr_t / den
    with np.errstate(divide='ignore', invalid='ignore'):
        d_v = np.where(vn > 0, -lr_t * mn / (den * den * 2.0 * sq), 0.0)
    var = d_m * d_m * vm + d_v * d_v * vv + upd * upd * (4 * U * U + rl * rl)
    return upd, np.minimum(var, vcap), d_m, d_v


def true_sums(params, s, grads, d):
    """the two column sums of the known-sums form for tensor d, from the stored fp32 arrays: A = sum_r (W / s)^2 and
    Bs = sum_r g W / s (= gdot / s), each with sigma and bound of an fp32 evaluation ('s_A', 'b_A', 's_B', 'b_B'); gdot itself
    (sum_r g W, fp64) as 'gdot'"""
    n, c = d.rows, d.cols
    sl = slice(d.offset, d.offset + n * c)
    W = np.asarray(params[sl], np.float64).reshape(n, c)
    g = np.asarray(grads[sl], np.float64).reshape(n, c)
    sc = np.asarray(s[d.col_offset:d.col_offset + c], np.float64)
    V = W / sc
    vV = 2 * U * U * V * V
    A = (V * V).sum(0)
    vA = (4 * V * V * vV).sum(0) + (U * U * V ** 4).sum(0) + (U * A) ** 2 * (n / 3.0 + 1)
    B = (g * V).sum(0)
    vB = (g * g * vV).sum(0) + (U * U * (g * V) ** 2).sum(0) + (U * np.abs(g * V).sum(0)) ** 2 * n / 3.0 + (U * B) ** 2
    return dict(A=A, B=B, gdot=(g * W).sum(0), s_A=np.sqrt(vA), b_A=KAPPA * np.sqrt(vA), s_B=np.sqrt(vB), b_B=KAPPA * np.sqrt(vB),
                V=V, vV=vV, vA=vA, vB=vB)


def ref_step(state, grads, table, hyp, mode='advance', known=None):
    """One step.  state: dict of the stored fp32 arrays params, m, v [n], mg, vg, s, vn2 [n_cols] and the counter 't' (int;
    ignored for ('explicit', t)).  table: the Desc of the tensors this call names (a sub-table for only=).  hyp: hyper().
    known: None (no vnorm2 array), or dict(tensor=index into table, use=bool, gdot=fp32 [cols] or None).
    Returns every array in fp64 (whole, untouched elements as stored), 's_' / 'b_' + name beside it, 'counter' (None for an
    explicit t), 't', 'lr_t', 'rel_lr', 'insens' (mask over params)."""
    h = hyp
    t, counter = step_of(int(state['t']), mode)
    opt, b1, b2, eps = h['opt'], h['b1'], h['b2'], h['eps']
    lr_t = h['lr'] if opt == OPT_RMSPROP else lr_t64(h, t)
    rl = 0.0 if opt == OPT_RMSPROP else rel_lr(h, t)
    vcap = (2.0 * lr_t * cap(h) / KAPPA) ** 2
    R = {k: np.asarray(state[k], np.float64).copy() for k in OUTPUTS}
    for k in OUTPUTS:
        R['s_' + k] = np.zeros_like(R[k])
    G = np.asarray(grads, np.float64)
    P0 = {k: np.asarray(state[k], np.float64) for k in OUTPUTS}
    for i, d in enumerate(table):
        n, c = d.rows, d.cols
        sl = slice(d.offset, d.offset + n * c)
        g = G[sl].reshape(n, c)
        m0, v0 = P0['m'][sl].reshape(n, c), P0['v'][sl].reshape(n, c)
        W = P0['params'][sl].reshape(n, c)

        def put(name, val, var, where=sl):
            R[name][where] = np.reshape(val, -1)
            R['s_' + name][where] = np.sqrt(np.reshape(var, -1))
        if opt == OPT_RMSPROP:
            an, va, _ = _ema(b2, v0, g, 0.0, True)
            sq = np.sqrt(an)
            den = sq + eps
            upd = lr_t * g / den
            with np.errstate(divide='ignore', invalid='ignore'):
                d_v = np.where(an > 0, -upd / (den * 2.0 * sq), 0.0)
            vu = np.minimum(d_v * d_v * va + 4 * U * U * upd * upd, vcap)
            put('v', an, va)
            put('params', W - upd, vu + (U * (W - upd)) ** 2)
            continue
        if opt == OPT_ADAM or not d.is_matrix:
            mn, vm, _ = _ema(b1, m0, g, 0.0, False)
            vn, vv, _ = _ema(b2, v0, g, 0.0, True)
            upd, vu, _, _ = _upd(mn, vm, vn, vv, lr_t, eps, rl, vcap)
            put('m', mn, vm)
            put('v', vn, vv)
            put('params', W - upd, vu + (U * (W - upd)) ** 2)
            continue
        cs = slice(d.col_offset, d.col_offset + c)
        sc, mg0, vg0 = P0['s'][cs], P0['mg'][cs], P0['vg'][cs]
        ts = true_sums(state['params'], state['s'], grads, d)
        V, vV = ts['V'], ts['vV']
        if known is not None and known.get('use') and known['tensor'] == i:
            A, vA = P0['vn2'][cs], 0.0
            B = np.asarray(known['gdot'], np.float64) / sc
            vB = (U * B) ** 2
        else:
            A, vA, B, vB = ts['A'], ts['vA'], ts['B'], ts['vB']
        Vn = np.sqrt(A)
        vVn = vA / (4 * A) + (U * Vn) ** 2
        gg = B / Vn
        vgg = vB / A + gg * gg * vVn / A + 3 * (U * gg) ** 2
        gov = gg / Vn
        vgov = vB / A ** 2 + B * B * vA / A ** 4 + 4 * (U * gov) ** 2
        mgn, vmg, _ = _ema(b1, mg0, gg, vgg, False)
        vgn, vvg, _ = _ema(b2, vg0, gg, vgg, True)
        gp = sc * Vn
        updg, vug, _, _ = _upd(mgn, vmg, vgn, vvg, lr_t, eps, rl, vcap)
        gnew = gp - updg
        vgnew = sc * sc * vVn + (U * gp) ** 2 + vug + (U * gnew) ** 2
        # the elements: grad_V, its independent variance and its derivative by the column's gov
        gV = sc * (g - gov * V)
        vgV_i = sc * sc * (gov * gov * vV + U * U * ((gov * V) ** 2 + (g - gov * V) ** 2)) + (U * gV) ** 2
        dgV_gov = -sc * V
        vgV = vgV_i + dgV_gov ** 2 * vgov
        mn, vm_r, dm_g = _ema(b1, m0, gV, 0.0, False)
        vn, vv_r, dv_g = _ema(b2, v0, gV, 0.0, True)
        upd, vu_r, d_m, d_v = _upd(mn, vm_r, vn, vv_r, lr_t, eps, rl, np.inf)
        D = d_m * dm_g + d_v * dv_g                      # d upd / d grad_V
        vu_i = np.minimum(vu_r + D * D * vgV_i, vcap)
        vu = np.minimum(vu_r + D * D * vgV, vcap)
        Vp = V - upd
        vVp_i = vV + vu_i + (U * Vp) ** 2
        vVp = vV + vu + (U * Vp) ** 2
        C = (Vp * Vp).sum(0)
        vC = (4 * Vp * Vp * vVp_i).sum(0) + (2 * Vp * D * dgV_gov).sum(0) ** 2 * vgov + ((2 * Vp * upd).sum(0) * rl) ** 2 \
            + (U * U * Vp ** 4).sum(0) + (U * C) ** 2 * (n / 3.0 + 1)
        sn = gnew / np.sqrt(C)
        vsn = vgnew / C + sn * sn * vC / (4 * C * C) + 2 * (U * sn) ** 2
        Wn = sn * Vp
        put('m', mn, vm_r + dm_g ** 2 * vgV)
        put('v', vn, vv_r + dv_g ** 2 * vgV)
        R['s_v'][sl] += ((1.0 - b2) * KAPPA * vgV).reshape(-1)       # the square's second-order term (see the docstring)
        put('params', Wn, sn * sn * vVp + Vp * Vp * vsn + (U * Wn) ** 2)
        put('mg', mgn, vmg, cs)
        put('vg', vgn, vvg, cs)
        put('s', sn, vsn, cs)
        if known is not None and is_tall(d):
            put('vn2', C, vC, cs)
    for k in OUTPUTS:
        R['b_' + k] = KAPPA * R['s_' + k]
    R.update(counter=counter, t=t, lr_t=lr_t, rel_lr=rl)
    R['insens'] = R['b_params'] > INSENS * lr_t
    return R


# ------------------------------------------------------------------------------------------------ fp32 evaluation --
ORDERS = ('seq', 'pair', 'u16', 'u64')
FAULTS = ('ragged_out', 'partial_last', 'partial_704', 'col_neighbour', 'col_group16', 'col_group64', 't_plus1',
          'no_bias_corr', 'b1b2_swap', 'eps_in_sqrt', 'gov_once', 'old_s', 'mgvg_per_unit', 'vn2_after_rescale',
          'm_under_rmsprop', 'skip_last_float4', 'float2_second')
F = np.float32


def colsum32(X, order):
    """column sums of the fp32 [n, c] array in fp32: 'seq' row after row, 'pair' a binary tree, 'u16' / 'u64' per-unit partials
    of 16 / 64 rows (row after row), then partial after partial"""
    X = np.ascontiguousarray(X, F)
    n = X.shape[0]
    if order == 'pair':
        k = 1
        while k < n:
            k *= 2
        Y = np.zeros((k,) + X.shape[1:], F)
        Y[:n] = X
        while k > 1:
            k //= 2
            Y = Y[:k] + Y[k:]
        return Y[0]
    if order in ('u16', 'u64'):
        u = int(order[1:])
        nun = (n + u - 1) // u
        Y = np.zeros((nun * u,) + X.shape[1:], F)
        Y[:n] = X
        Y = Y.reshape((nun, u) + X.shape[1:])
        part = np.zeros((nun,) + X.shape[1:], F)
        for r in range(u):
            part = part + Y[:, r]
        X = part
    acc = np.zeros(X.shape[1:], F)
    for r in range(X.shape[0]):
        acc = acc + X[r]
    return acc


def _rowmask(n, faults):
    keep = np.ones(n, bool)
    if 'ragged_out' in faults:
        keep[n // 16 * 16:] = False
    nun = (n + 15) // 16
    if 'partial_last' in faults:
        keep[(nun - 1) * 16:] = False
    if 'partial_704' in faults and nun > 704:
        keep[704 * 16:705 * 16] = False
    return keep[:, None].astype(F)


def eval32(state, grads, table, hyp, mode='advance', known=None, order='seq', faults=()):
    """an honest fp32 evaluation of the contract (numpy float32 throughout, powf from the host's libm), column sums in the
    given order; faults: names out of FAULTS.  Returns the arrays (fp32) and 'counter'."""
    h = hyp
    t, counter = step_of(int(state['t']), mode)
    if 't_plus1' in faults:
        t += 1
    opt = h['opt']
    lr, b1, b2, eps = F(h['lr']), F(h['b1']), F(h['b2']), F(h['eps'])
    one = F(1)
    lr_t = lr * np.sqrt(one - np.power(b2, F(t))) / (one - np.power(b1, F(t)))
    if 'no_bias_corr' in faults:
        lr_t = lr
    if 'b1b2_swap' in faults:
        b1, b2 = b2, b1
    den = (lambda v: np.sqrt(v + eps)) if 'eps_in_sqrt' in faults else (lambda v: np.sqrt(v) + eps)
    R = {k: np.asarray(state[k], F).copy() for k in OUTPUTS}
    G = np.asarray(grads, F)
    for i, d in enumerate(table):
        n, c = d.rows, d.cols
        sl = slice(d.offset, d.offset + n * c)
        g, W = G[sl].reshape(n, c), R['params'][sl].reshape(n, c).copy()
        m0, v0 = R['m'][sl].reshape(n, c).copy(), R['v'][sl].reshape(n, c).copy()
        if opt == OPT_RMSPROP:
            an = b2 * v0 + (one - b2) * g * g
            R['v'][sl] = an.reshape(-1)
            R['params'][sl] = (W - lr * g / den(an)).reshape(-1)
            if 'm_under_rmsprop' in faults:
                R['m'][sl] = (b1 * m0 + (one - b1) * g).reshape(-1)
            continue
        if opt == OPT_ADAM or not d.is_matrix:
            mn = b1 * m0 + (one - b1) * g
            vn = b2 * v0 + (one - b2) * g * g
            R['m'][sl], R['v'][sl] = mn.reshape(-1), vn.reshape(-1)
            R['params'][sl] = (W - lr_t * mn / den(vn)).reshape(-1)
            continue
        cs = slice(d.col_offset, d.col_offset + c)
        sc = R['s'][cs].copy()
        inv_s = one / sc
        V = W * inv_s
        keep = _rowmask(n, faults)
        if known is not None and known.get('use') and known['tensor'] == i:
            A = R['vn2'][cs].copy()
            Vn = np.sqrt(A)
            gg = np.asarray(known['gdot'], F) * inv_s / Vn
        else:
            A = colsum32(V * V * keep, order)
            Vn = np.sqrt(A)
            gg = colsum32(g * V * keep, order) / Vn
        gov = gg if 'gov_once' in faults else gg / Vn
        mg0, vg0 = R['mg'][cs].copy(), R['vg'][cs].copy()
        mgn, vgn = mg0, vg0
        for _ in range((n + 15) // 16 if 'mgvg_per_unit' in faults else 1):
            mgn = b1 * mgn + (one - b1) * gg
            vgn = b2 * vgn + (one - b2) * gg * gg
        gnew = sc * Vn - lr_t * mgn / den(vgn)
        idx = np.arange(c)
        if 'col_neighbour' in faults:
            idx = np.minimum(idx + 1, c - 1)
        if 'col_group16' in faults:
            idx = np.where(idx >= 16, idx - 16, idx)
        if 'col_group64' in faults:
            idx = np.where(idx >= 64, idx - 64, idx)
        if 'float2_second' in faults:
            idx = idx - (idx % 2)
        e_is, e_gov, e_sc = inv_s[idx], gov[idx], sc[idx]          # the scalars the element pass uses
        Ve = W * e_is
        gV = e_sc * (g - e_gov * Ve)
        mn = b1 * m0 + (one - b1) * gV
        vn = b2 * v0 + (one - b2) * gV * gV
        Vp = Ve - lr_t * mn / den(vn)
        C = colsum32(Vp * Vp * keep, order)
        sn = gnew / np.sqrt(C)
        Wn = (sc if 'old_s' in faults else sn) * Vp
        if 'skip_last_float4' in faults:                    # the last 16 bytes of every 64-row tile left as they were
            assert c % 4 == 0
            for r0 in range(0, n, 64):
                r = min(r0 + 64, n) - 1
                mn[r, c - 4:], vn[r, c - 4:], Wn[r, c - 4:] = m0[r, c - 4:], v0[r, c - 4:], W[r, c - 4:]
        R['m'][sl], R['v'][sl], R['params'][sl] = mn.reshape(-1), vn.reshape(-1), Wn.reshape(-1)
        R['mg'][cs], R['vg'][cs], R['s'][cs] = mgn, vgn, sn
        if known is not None and is_tall(d):
            R['vn2'][cs] = sn * sn * C if 'vn2_after_rescale' in faults else C
    R['counter'] = counter
    return R


# ------------------------------------------------------------------------------------------------------- comparison --
def _q(got, rf, scale):
    e = np.abs(np.asarray(got, np.float64) - rf)
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(e == 0, 0.0, e / scale)
    return np.nan_to_num(q, nan=np.inf, posinf=np.inf), e


def ratios(got, ref, outputs=OUTPUTS):
    """worst |got - ref| / bound per output; a NaN, or an error where the bound is 0 (an element the step does not own), inf"""
    return {k: float(_q(got[k], ref[k], ref['b_' + k])[0].max()) for k in outputs}


def violations(got, ref, outputs=OUTPUTS):
    return [(k, v) for k, v in ratios(got, ref, outputs).items() if not v <= 1.0]


def rms(got, ref, table, outputs=FLAT):
    """worst rms(err / sigma) per output over the tensors of the table with at least RMS_MIN elements (elements with sigma = 0
    and no error do not count); outputs without such a tensor are left out"""
    out = {}
    for k in outputs:
        for d in table:
            if d.rows * d.cols < RMS_MIN:
                continue
            sl = slice(d.offset, d.offset + d.rows * d.cols)
            q, e = _q(got[k][sl], ref[k][sl], ref['s_' + k][sl])
            n = int(((ref['s_' + k][sl] > 0) | (e != 0)).sum())
            if n:
                out[k] = max(out.get(k, 0.0), float(np.sqrt(np.square(q).sum() / n)))
    return out


def rms_violations(got, ref, table, outputs=FLAT):
    return [('rms ' + k, v) for k, v in rms(got, ref, table, outputs).items() if not v <= 1.0]


def sums_ratio(vn2, params, s, grads, d):
    """worst |stored vn2 - true sum_r (W / s)^2| / bound over the columns of tensor d"""
    ts = true_sums(params, s, grads, d)
    return float(_q(np.asarray(vn2)[d.col_offset:d.col_offset + d.cols], ts['A'], ts['b_A'])[0].max())


def insensitive_share(ref, table):
    n = sum(d.rows * d.cols for d in table)
    return float(ref['insens'].sum()) / n


# ------------------------------------------------------------------------------------------------------------ cases --
# name, tensors, routes, only (the sub-table of the fast route's own call; the other tensors go in a second, chain call).
# Routes: 'small' (no tall matrix: every tensor in its own blocks), 'chain' (five launches), 'fast' (step 1 by the chain, then the
# two-launch known-sums form; which of its bodies follows from cols % 4 of the tall matrix), 'adam', 'rmsprop'.
def _case(name, shapes, routes, only=None):
    return dict(name=name, shapes=shapes, routes=routes, only=only)


K, B_ = '/kernel', '/bias'
GPU_CASES = [
    _case('small', [('a' + K, (2, 1)), ('a' + B_, (1,)), ('b' + K, (15, 3)), ('b' + B_, (3,)), ('c' + K, (16, 16)), ('c' + B_, (352,)),
                    ('d' + K, (17, 17)), ('e' + K, (143, 88)), ('e' + B_, (300,)), ('f' + K, (144, 352)), ('g' + K, (2, 88))], ('small',)),
    _case('chain_two_tall_narrow', [('t' + K, (145, 1)), ('t' + B_, (3,)), ('u' + K, (160, 3))], ('chain',)),
    _case('chain_tall_last', [('s' + K, (16, 17)), ('s' + B_, (17,)), ('t' + K, (200, 88))], ('chain',)),
    _case('chain_704_units', [('t' + K, (11264, 88))], ('chain',)),
    _case('chain_two_tall_main_loop', [('p' + B_, (5,)), ('t' + K, (11265, 3)), ('q' + K, (15, 16)), ('u' + K, (12293, 130))], ('chain',)),
    _case('flat_first_145x4', [('t' + K, (145, 4)), ('a' + K, (16, 17)), ('a' + B_, (17,))], ('fast', 'chain')),
    _case('flat_middle_160x8', [('a' + K, (17, 3)), ('t' + K, (160, 8)), ('a' + B_, (3,))], ('fast', 'chain')),
    _case('flat_last_192x12', [('a' + B_, (5,)), ('a' + K, (144, 16)), ('t' + K, (192, 12))], ('fast', 'chain')),
    _case('flat_193x100', [('a' + K, (15, 88)), ('t' + K, (193, 100)), ('a' + B_, (88,))], ('fast', 'chain')),
    _case('flat_11264x88', [('t' + K, (11264, 88)), ('a' + K, (130, 352)), ('a' + B_, (352,))], ('fast', 'chain')),
    _case('flat_only_193x128', [('a' + K, (16, 16)), ('b' + B_, (16,)), ('t' + K, (193, 128)), ('c' + K, (17, 3))], ('fast', 'chain'),
          only=('b' + B_, 't' + K)),
    _case('pair_first_145x2', [('t' + K, (145, 2)), ('a' + B_, (3,))], ('fast', 'chain')),
    _case('pair_middle_160x6', [('a' + K, (16, 3)), ('t' + K, (160, 6)), ('a' + B_, (3,))], ('fast', 'chain')),
    _case('pair_last_192x90', [('a' + B_, (1,)), ('t' + K, (192, 90))], ('fast', 'chain')),
    _case('pair_193x126', [('a' + K, (2, 17)), ('t' + K, (193, 126)), ('a' + B_, (17,))], ('fast', 'chain')),
    _case('pair_11264x90', [('t' + K, (11264, 90))], ('fast', 'chain')),
    _case('mixed_plain', [('a' + K, (17, 88)), ('a' + B_, (88,)), ('t' + K, (200, 130)), ('b' + B_, (352,)), ('c' + K, (144, 3))],
          ('adam', 'rmsprop')),
]
DEGENERATE_CASES = [
    _case('one_row', [('r' + K, (1, 16)), ('r' + B_, (16,)), ('q' + K, (1, 3)), ('p' + K, (1, 1))], ('small',)),
    _case('zero_gradient', [('a' + K, (17, 16)), ('a' + B_, (5,)), ('t' + K, (160, 8))], ('chain', 'fast')),
]
ROUTE_OPT = dict(small=OPT_ADAM_WN, chain=OPT_ADAM_WN, fast=OPT_ADAM_WN, adam=OPT_ADAM, rmsprop=OPT_RMSPROP)


def fast_body(d):
    """the launcher's rule for the two-launch form's body"""
    return 'flat' if d.cols % 4 == 0 else 'pair'


def tall_index(table):
    tall = [i for i, d in enumerate(table) if is_tall(d)]
    return tall[0] if len(tall) == 1 else None


def make_grads(table, n, seed, zero=False):
    """gradients: six orders of magnitude across the rows of every tensor (a row keeps its scale from step to step, so that the
    moments of the small ones stay small: v down to 1e-9, where eps counts), about one row in sixteen zero (at least one where
    there are 8 rows), column 1 of every matrix of at least two columns zero (always the same one, so that its moments
    stay 0 as well); the padding holds SENTINEL.  Returns (grads fp32, counts)."""
    rng = np.random.default_rng(seed)
    g = np.full(n, SENTINEL, F)
    cnt = dict(zero_rows=0, zero_cols=0)
    for d in table:
        x = rng.standard_normal((d.rows, d.cols))
        prng = np.random.default_rng(d.offset)          # a row's (a bias element's) scale is the same at every step
        if d.is_matrix:
            x *= 10.0 ** (prng.permutation(np.linspace(-3, 3, d.rows)) if d.rows > 1 else np.zeros(1))[:, None]
            if d.rows >= 8:
                z = rng.random(d.rows) < 1 / 16.0
                z[rng.integers(d.rows)] = True
                x[z] = 0
                cnt['zero_rows'] += int(z.sum())
            if d.cols >= 2:
                x[:, 1] = 0
                cnt['zero_cols'] += 1
        else:
            x *= 10.0 ** prng.permutation(np.linspace(-3, 3, d.cols))[None, :]
        g[d.offset:d.offset + d.rows * d.cols] = (0 * x if zero else x).reshape(-1)
    return g, cnt


def store(ref):
    """the reference's outputs rounded to fp32 as the next stored state"""
    out = {k: np.asarray(ref[k], F) for k in OUTPUTS}
    out['t'] = ref['counter'] if ref['counter'] is not None else ref['t']
    return out


def make_state(case, route, seed=0, history=2):
    """(table, n, n_cols, state): parameters 0.1 normal (0.3 for the biases), s = 1, zero moments, then `history` reference steps of
    the route's optimizer on fresh gradients, each stored in fp32: non-zero m, v, mg, vg, s != 1 and t = history from real
    steps.  Every padding float and column, and vn2, hold SENTINEL."""
    table, n, n_cols = layout(case['shapes'])
    rng = np.random.default_rng(1000 + seed)
    st = {k: np.full(n, SENTINEL, F) for k in FLAT}
    st.update({k: np.full(n_cols, SENTINEL, F) for k in COLS})
    for d in table:
        sl = slice(d.offset, d.offset + d.rows * d.cols)
        st['params'][sl] = (0.1 if d.is_matrix else 0.3) * rng.standard_normal(d.rows * d.cols)
        st['m'][sl] = st['v'][sl] = 0
        if d.is_matrix:
            cs = slice(d.col_offset, d.col_offset + d.cols)
            st['mg'][cs] = st['vg'][cs] = 0
            st['s'][cs] = 1
    st['t'] = 0
    hyp = hyper(opt=ROUTE_OPT[route])
    for k in range(history):
        g, _ = make_grads(table, n, 7000 + 10 * seed + k, zero=case['name'] == 'zero_gradient')
        st = store(ref_step(st, g, table, hyp))
    return table, n, n_cols, st
