"""fp64 reference of the fused cl_vae step (include/clvae.h: clv_vae_fused_step, clv_vae_step_opts).

Written from the header's contract, not from the kernel's structure, out of oracle/clvae_oracle.py pieces:

  params    the 12 tensors of host_offsets12 in that order: {h_w, wargs, h, zargs, decoder_h, x_decoded_mean} x {kernel,
            bias}, the two head pairs FUSED ([in, 2n] kernels: w_mean | w_log_var and z_mean | z_log_var).  `fuse` /
            `unfuse_grads` convert from / to the oracle's Keras names; `layout` / `scatter` / `gather` place them in a flat
            buffer at arbitrary element offsets (the tests use their own order with gaps; nothing here reads
            engine.FlatParams).
  forward   O.vae_forward's graph with injected eps: logits [B,D], w [B,C], wargs [B,2(C-1)] = mean | log_var,
            zargs [B,2L], rownll [B] (O.bce_from_logits_keras, float32 clip points), rowkl [B] (O.kl_gauss),
            rowloss [B,3] = kl_w (O.kl_w_prior), w_rec (O.cce_keras), hit (argmax, first index on ties; hit = w_rec = 0
            without onehot).  target: what the decoder output is scored against (None: x).
  backward  the gradient of (sum_rows vae + kl_weight kl_z + w_kl_weight kl_w + class_weight w_rec) / B, O.vae_loss_and_grads'
            formulas on the fused tensors.
  bf16      opts.bf16: every Dense product (forward and backward, DY . W^T) and every weight-gradient product GA^T . DY rounds
            BOTH operands to bf16 (round to nearest even, v_cvt_pk_bf16_f32) and accumulates in fp32; the biases, the bias
            gradients (column sums), sampling and the losses stay fp32.

Bounds.  Beside every output element the reference carries sigma, a first-order standard error of an fp32 evaluation of
the same contract, and the element's bound is KAPPA * sigma:
  * a dot product of n terms rounds n times, each time by at most U |partial sum| <= U sum|terms|; those roundings are
    independent, so it contributes a variance of (U sum|terms|)^2 n / 3 (the uniform distribution's);
  * a transcendental contributes its budget below (EXP_ULP, LOG_ABS, RCP_ULP; exp also |x| U for the argument rounding
    inside v_exp_f32), every other fp32 operation one U of its result;
  * every input's variance reaches an output through the exact first derivative (Jacobian squared, root-sum-square
    over distinct sources: rounding errors of different units are independent).  Worst-case |J| b chains would grow by
    about sqrt(K) per Dense layer, 11 layers deep for the h_w gradient, and leave no bar at all.
  * bf16 mode: a bf16-rounded operand is exact unless the fp64 value lies within its bound of a rounding midpoint
    (round(v - b) != round(v + b)): there the two roundings may differ by one bf16 ulp, which enters as sigma on top
    of the fp32 one.
Flags (the elements where fp32 may legitimately take the other branch) widen sigma by the whole difference the branch
makes; they are counted in r['flags']:
  relu_*    pre-activations of h_w, h, decoder_h within their bound of 0 (the backward masks);
  clip_l    logits within their bound of BCE_CLIP_LO / BCE_CLIP_HI (the gradient is 0 outside);
  clip_w    w_rec's renormalised w of the true class within its bound of the 1e-7 / 1 - 1e-7 clip;
  tie       rows whose two largest w lie within their bounds of each other but are not equal (hit may differ).
Nothing here is fitted to errors seen on a GPU; tests/test_vae_reference.py checks the bounds against an fp32 evaluation
(`evaluate32`: shuffled summation orders, every transcendental perturbed by its budget).
"""
import numpy as np

from oracle import clvae_oracle as O

U = 2.0 ** -24
KAPPA = 6.0          # bound = KAPPA sigma (Hoeffding: P(|sum of independent bounded errors| > 6 sigma) <= 2 e^-18)
EXP_ULP = 4          # expf / __expf: ulp of the result on top of |x| U (v_exp_f32 takes x log2(e), rounded)
LOG_ABS = 4          # logf / __logf: absolute error in U (v_log_f32 is 1 ulp of log2; ln 2 scaling and the
                     # rounding of the argument, relative U -> absolute U, are included)
RCP_ULP = 2          # fast_rcp = v_rcp_f32: 1 ulp, doubled
CLIP_LO32, CLIP_HI32 = np.float32(-16.11809555), np.float32(15.94238503)   # BCE_CLIP_LO / BCE_CLIP_HI (common.h)
EPS_LO32, EPS_HI32 = float(np.float32(1e-7)), float(np.float32(1.0) - np.float32(1e-7))
W2 = 1e-10

NAMES = ('h_w/kernel', 'h_w/bias', 'wargs/kernel', 'wargs/bias', 'h/kernel', 'h/bias', 'zargs/kernel', 'zargs/bias',
         'decoder_h/kernel', 'decoder_h/bias', 'x_decoded_mean/kernel', 'x_decoded_mean/bias')
OUTPUTS = ('logits', 'w', 'wargs', 'zargs', 'rownll', 'rowkl', 'rowloss')
LOSS_COLS = ('vae', 'kl_z', 'kl_w', 'w_rec', 'acc')       # loss_means order: rownll, rowkl, rowloss columns


# ---------------------------------------------------------------------------------------------------------- layout --
def shapes(D, H, Hc, C, L, use_x_prev):
    KD = C + (D if use_x_prev else 0) + L
    return [(D, Hc), (Hc,), (Hc, 2 * (C - 1)), (2 * (C - 1),), (D + C, H), (H,), (H, 2 * L), (2 * L,),
            (KD, H), (H,), (H, D), (D,)]


def fuse(p):
    """oracle parameter dict (Keras names) -> the 12 tensors in host_offsets12 order"""
    cat = lambda a, b: np.concatenate([p[a], p[b]], -1)
    return [p['h_w/kernel'], p['h_w/bias'], cat('w_mean/kernel', 'w_log_var/kernel'), cat('w_mean/bias', 'w_log_var/bias'),
            p['h/kernel'], p['h/bias'], cat('z_mean/kernel', 'z_log_var/kernel'), cat('z_mean/bias', 'z_log_var/bias'),
            p['decoder_h/kernel'], p['decoder_h/bias'], p['x_decoded_mean/kernel'], p['x_decoded_mean/bias']]


def unfuse_grads(g, C, L):
    C1 = C - 1
    return {'h_w/kernel': g[0], 'h_w/bias': g[1], 'w_mean/kernel': g[2][:, :C1], 'w_log_var/kernel': g[2][:, C1:],
            'w_mean/bias': g[3][:C1], 'w_log_var/bias': g[3][C1:], 'h/kernel': g[4], 'h/bias': g[5],
            'z_mean/kernel': g[6][:, :L], 'z_log_var/kernel': g[6][:, L:], 'z_mean/bias': g[7][:L], 'z_log_var/bias': g[7][L:],
            'decoder_h/kernel': g[8], 'decoder_h/bias': g[9], 'x_decoded_mean/kernel': g[10], 'x_decoded_mean/bias': g[11]}


def layout(shp, order=None, gaps=None):
    """element offsets of the 12 tensors placed in `order` (default host_offsets12 order) with gaps[i] elements in front of
    the i-th placed one and gaps[-1] more behind the last.  Returns (offsets [12] int64 in host_offsets12 order, length)."""
    order = list(range(12)) if order is None else list(order)
    gaps = [0] * 12 if gaps is None else list(gaps)
    offs, o = np.zeros(12, np.int64), 0
    for i, t in enumerate(order):
        o += gaps[i]
        offs[t] = o
        o += int(np.prod(shp[t]))
    return offs, o + gaps[-1]


def scatter(ts, offs, n, fill=0.0, dtype=np.float32):
    flat = np.full(n, fill, dtype)
    for t, o in zip(ts, offs):
        flat[o:o + np.size(t)] = np.ravel(t)
    return flat


def gather(flat, offs, shp):
    return [np.asarray(flat[o:o + int(np.prod(s))]).reshape(s) for o, s in zip(offs, shp)]


def gap_mask(offs, shp, n):
    """True on the elements of a flat buffer that no tensor covers"""
    m = np.ones(n, bool)
    for o, s in zip(offs, shp):
        m[o:o + int(np.prod(s))] = False
    return m


# ------------------------------------------------------------------------------------------------------------ bf16 --
def bf16(a):
    """round to the nearest bf16, ties to even (normal range; the values here are far from bf16's limits)"""
    a = np.asarray(a, np.float64)
    m, e = np.frexp(a)
    return np.ldexp(np.round(m * 256.0), e - 8)


# ------------------------------------------------------------------------------------------------------- arithmetic --
class _F64:
    """exact-as-possible arithmetic of the reference"""
    dt = np.float64

    def dot(self, A, B):
        return A @ B

    def colsum(self, A):
        return A.sum(0)

    def rowsum(self, A):
        return A.sum(-1)

    def exp(self, x):
        return np.exp(x)

    def log(self, x):
        return np.log(x)

    def rcp(self, x):
        return 1.0 / x

    def c(self, a):
        return np.asarray(a, np.float64)


class F32:
    """an fp32 evaluation of the contract: products and sums in a random order, transcendentals perturbed within their
    budgets (uniformly, independently per element)"""
    dt = np.float32

    def __init__(self, rng):
        self.rng = rng

    def c(self, a):
        return np.asarray(a, np.float32)

    def dot(self, A, B):
        A, B = self.c(A), self.c(B)
        acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
        for k in self.rng.permutation(A.shape[1]):
            acc = acc + A[:, k, None] * B[None, k, :]
        return acc

    def colsum(self, A):
        A = self.c(A)
        acc = np.zeros(A.shape[1:], np.float32)
        for b in self.rng.permutation(A.shape[0]):
            acc = acc + A[b]
        return acc

    def rowsum(self, A):
        return self.colsum(self.c(A).T)

    def _u(self, shape):
        return self.rng.uniform(-1.0, 1.0, shape)

    def exp(self, x):
        x = self.c(x)
        x64 = x.astype(np.float64)
        return self.c(np.exp(x64) * (1.0 + self._u(x.shape) * (EXP_ULP + np.abs(x64)) * U))

    def log(self, x):
        x = self.c(x)
        return self.c(np.log(x.astype(np.float64)) + self._u(x.shape) * LOG_ABS * U)

    def rcp(self, x):
        x = self.c(x)
        return self.c(1.0 / x.astype(np.float64) * (1.0 + self._u(x.shape) * RCP_ULP * U))


def _relu(a):
    return np.maximum(a, 0)


# ----------------------------------------------------------------------------------------------------------- values --
def _values(ar, P, x, xp, onehot, eps_w, eps_z, prior, cw, kw, wkw, use_x_prev, target, need_grads, bf, faults=()):
    """the step's values in arithmetic `ar`; returns (outputs, cache).  faults: names of planted faults (tests only)."""
    c = ar.c
    Khw, bhw, Kwa, bwa, Kh, bh, Kza, bza, Kd, bd, Ko, bo = [c(t) for t in P]
    x, eps_w, eps_z = c(x), c(eps_w), c(eps_z)
    B, D = x.shape
    C1, L = Kwa.shape[1] // 2, Kza.shape[1] // 2
    C = C1 + 1
    y = x if target is None else c(target)
    if 'score_against_x' in faults:
        y = x
    R = (lambda a: c(bf16(a))) if bf else (lambda a: a)
    mm = lambda A, K: ar.dot(R(A), R(K))                 # Dense product / weight-gradient product
    k = {}
    k['a_hw'] = mm(x, Khw) + bhw
    k['hw'] = _relu(k['a_hw'])
    wargs = mm(k['hw'], Kwa) + bwa
    m, lv = wargs[:, :C1], wargs[:, C1:]
    sdw = ar.exp(c(0.5) * lv)
    s = m + sdw * eps_w
    e = np.concatenate([ar.exp(s), np.ones((B, 1), ar.dt)], 1)
    S = ar.rowsum(e)[:, None]
    w = e * ar.rcp(S)
    k.update(m=m, lv=lv, sdw=sdw, s=s, w=w, S=S)
    ep = ar.exp(c(prior))
    klw = c(-0.5) * ar.rowsum(c(1.0) - c(prior) + lv - sdw * sdw / ep - m * m / ep)
    q = w + c(W2)
    qs = ar.rowsum(q)[:, None]
    n = q / qs
    k.update(ep=ep, n=n, qs=qs)
    if onehot is not None:
        oh = c(onehot)
        nc = np.clip(n, c(EPS_LO32 if ar.dt == np.float32 else O.EPS_K), c(EPS_HI32 if ar.dt == np.float32 else 1 - O.EPS_K))
        wrec = c(C1) * -ar.rowsum(oh * ar.log(nc))
        hit = (np.argmax(w, 1) == np.argmax(oh, 1)).astype(ar.dt)
    else:
        oh = np.zeros((B, C), ar.dt)
        wrec, hit = np.zeros(B, ar.dt), np.zeros(B, ar.dt)
    k['xw'] = np.concatenate([x, w], 1)
    k['a_h'] = mm(k['xw'], Kh) + bh
    k['h'] = _relu(k['a_h'])
    zargs = mm(k['h'], Kza) + bza
    zm, zlv = zargs[:, :L], zargs[:, L:]
    sdz = ar.exp(c(0.5) * zlv)
    z = zm + sdz * eps_z
    k.update(zm=zm, zlv=zlv, sdz=sdz, z=z)
    rowkl = c(-0.5) * ar.rowsum(c(1.0) + zlv - zm * zm - sdz * sdz)
    if 'rowkl_drop_last' in faults:
        rowkl = rowkl.copy()
        r = 16 * ((B - 16) // 16) + 15 if B >= 16 else B - 1          # the last row 16 k + 15 of the batch
        rowkl[r] = c(-0.5) * ar.rowsum((c(1.0) + zlv - zm * zm - sdz * sdz)[r:r + 1, :-1])[0] if L > 1 else 0.0
    k['wz'] = np.concatenate([w, c(xp), z] if use_x_prev else [w, z], 1)
    k['a_dh'] = mm(k['wz'], Kd) + bd
    k['hd'] = _relu(k['a_dh'])
    logits = mm(k['hd'], Ko) + bo
    lo, hi = (CLIP_LO32, CLIP_HI32) if ar.dt == np.float32 else (O.LOGIT_CLIP_LO, O.LOGIT_CLIP_HI)
    l = np.clip(logits, c(lo), c(hi))
    el = ar.exp(-np.abs(l))
    rownll = ar.rowsum(np.maximum(l, 0) + ar.log(c(1.0) + el) - l * y)
    out = dict(logits=logits, w=w, wargs=wargs, zargs=zargs, rownll=rownll, rowkl=rowkl,
               rowloss=np.stack([klw, wrec, hit], 1))
    k.update(l=l, el=el, y=y, oh=oh)
    if not need_grads:
        return out, k
    # ---- backward ----
    inv_b = c(1.0 / B) if ar.dt == np.float64 else np.float32(1.0) / np.float32(B)
    r1 = ar.rcp(c(1.0) + el)
    sg = np.where(l >= 0, r1, el * r1)
    inside = (logits >= c(lo)) & (logits <= c(hi))
    if 'bce_grad_outside_clip' in faults:
        inside = np.ones_like(inside)
    dl = np.where(inside, inv_b * (sg - y), c(0.0))
    k.update(dl=dl, sg=sg, inside=inside)
    mmT = lambda A, K: ar.dot(R(A), R(K).T)
    relu_dh = k['a_dh'] > 0
    if 'drop_relu_mask_dh' in faults:
        relu_dh = np.ones_like(relu_dh)
    g1 = mmT(dl, Ko) * relu_dh
    xo = D if use_x_prev else 0
    dw_dec = mmT(g1, Kd[:C])
    dz = mmT(g1, Kd[C + xo:])
    ks = c(kw) * inv_b
    dzm = dz + ks * zm
    dzlv = dz * eps_z * c(0.5) * sdz - c(0.5) * ks * (c(1.0) - sdz * sdz)
    dza = np.concatenate([dzm, dzlv], 1)
    g2 = mmT(dza, Kza) * (k['a_h'] > 0)
    dw = dw_dec + mmT(g2, Kh[D:])
    # label head backward: w_rec through the renormalisation and the clip, then the softmax and the sampling
    if onehot is not None:
        ins = (n >= c(EPS_LO32 if ar.dt == np.float32 else O.EPS_K)) & (n <= c(EPS_HI32 if ar.dt == np.float32 else 1 - O.EPS_K))
        dn = np.where(ins, -c(C1) * oh / nc, c(0.0))
    else:
        ins, dn = np.ones_like(n, bool), np.zeros_like(n)
    dot = ar.rowsum(dn * n)[:, None]
    d = dw + c(cw) * inv_b * ((dn - dot) / qs)
    dsum = ar.rowsum(d * w)[:, None]
    ds = (w * (d - dsum))[:, :C1]
    dwm = ds + c(wkw) * inv_b * (m / ep)
    dwlv = ds * eps_w * c(0.5) * sdw + c(wkw) * inv_b * (c(-0.5) * (c(1.0) - sdw * sdw / ep))
    dwa = np.concatenate([dwm, dwlv], 1)
    g3 = mmT(dwa, Kwa) * (k['a_hw'] > 0)
    k.update(g1=g1, g2=g2, g3=g3, dw=dw, d=d, dsum=dsum, ds=ds, dza=dza, dwa=dwa, dn=dn, ins=ins, dz=dz, ks=ks,
             inv_b=inv_b, dot=dot)
    wg = lambda GA, DY: ar.dot(R(GA).T, R(DY))
    grads = [wg(x, g3), ar.colsum(g3), wg(k['hw'], dwa), ar.colsum(dwa), wg(k['xw'], g2), ar.colsum(g2),
             wg(k['h'], dza), ar.colsum(dza), wg(k['wz'], g1), ar.colsum(g1), wg(k['hd'], dl), ar.colsum(dl)]
    out['grads'] = grads
    return out, k


# -------------------------------------------------------------------------------------------------------- reference --
def reference(P, x, xp, onehot, eps_w, eps_z, prior, class_weight, kl_weight, w_kl_weight, use_x_prev, target=None,
              need_grads=True, bf16_mode=False):
    """the fp64 reference: outputs, their bounds ('b_' + name, grads: 'b_grads') and flags.  Inputs are fp32 values."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    P = [f(t) for t in P]
    x, xp, onehot, eps_w, eps_z, target = map(f, (x, xp, onehot, eps_w, eps_z, target))
    r, k = _values(_F64(), P, x, xp, onehot, eps_w, eps_z, prior, class_weight, kl_weight, w_kl_weight, use_x_prev, target,
                   need_grads, bf16_mode)
    A, sq = np.abs, np.square
    B, D = x.shape
    C1, L = P[2].shape[1] // 2, P[6].shape[1] // 2
    C = C1 + 1
    Khw, bhw, Kwa, bwa, Kh, bh, Kza, bza, Kd, bd, Ko, bo = P
    flags = {}
    R = bf16 if bf16_mode else (lambda a: a)

    def operand(a, v, name=None):
        """(rounded operand, its variance) -- bf16: exact unless a midpoint lies within the bound"""
        if not bf16_mode:
            return a, v
        b = KAPPA * np.sqrt(v)
        lo, hi = bf16(a - b), bf16(a + b)
        flip = lo != hi
        if name:
            flags['bf16_' + name] = int(flip.sum())
        ulp = np.ldexp(1.0, np.frexp(A(a) + b)[1] - 8)            # a bf16 ulp at the top of the interval
        return bf16(a), np.where(flip, v + sq(ulp), 0.0)

    def dense(a, va, K, bias, name, T=False):
        """variance of a . K (+ bias): the operand's through K, the dot's own roundings"""
        ar, var = operand(a, va, name)
        Kr = R(K.T if T else K)
        n = Kr.shape[0] + 1
        loc = U * (A(ar) @ A(Kr) + (A(bias) if bias is not None else 0.0))
        return var @ sq(Kr) + sq(loc) * n / 3.0 + sq(U * A(ar @ Kr))

    def expv(xv, vx):
        """variance of exp(x) relative to exp(x)^2: the argument's and the budget"""
        return vx + sq((EXP_ULP + A(xv)) * U)

    # ---- forward ----
    v_ahw = dense(x, np.zeros_like(x), Khw, bhw, None)
    flags['relu_hw'] = A(k['a_hw']) <= KAPPA * np.sqrt(v_ahw)
    cut = lambda v, a, edge: np.where((a > 0) | edge, v, 0.0)       # relu: 1-Lipschitz; a cut unit is exactly 0
    v_hw = cut(v_ahw, k['a_hw'], flags['relu_hw'])
    v_wa = dense(k['hw'], v_hw, Kwa, bwa, 'hw')
    m, lv, sdw, s, w, S = k['m'], k['lv'], k['sdw'], k['s'], k['w'], k['S']
    vm, vlv = v_wa[:, :C1], v_wa[:, C1:]
    ew = eps_w
    # s = m + sd eps_w, sd = exp(lv / 2)
    v_s = vm + sq(sdw * ew) * expv(0.5 * lv, 0.25 * vlv) + sq(U * A(sdw * ew)) + sq(U * A(s))
    v_se = np.concatenate([v_s + sq((EXP_ULP + A(s)) * U), np.zeros((B, 1))], 1)    # + the exp of s
    # w = softmax([s, 0]): dw_j = w_j (ds_j - sum_k w_k ds_k); S's sum and the reciprocal, the product
    tot = (sq(w) * v_se).sum(1, keepdims=True)
    v_w = sq(w) * ((1 - 2 * w) * v_se + tot) + sq(w * U) * (C / 3.0 + RCP_ULP ** 2 + 1)
    v_w = np.maximum(v_w, 0.0)
    # kl_w = -0.5 sum_j (1 - prior + lv - sd^2 / ep - m^2 / ep)
    ep = np.exp(prior)
    terms = A(1 - prior) + A(lv) + sdw * sdw / ep + m * m / ep
    v_klw = 0.25 * ((4 * sq(m / ep) * vm + sq(1 - sdw * sdw / ep) * vlv).sum(1)
                    + (sq(U * 4 * terms) + sq(2 * (EXP_ULP + 0.5 * A(lv)) * U * sdw * sdw / ep)).sum(1)
                    + sq(U * terms.sum(1)) * C1 / 3.0
                    + sq((EXP_ULP + A(prior)) * U * ((sdw * sdw + m * m) / ep).sum(1)))
    b_row = np.zeros((B, 3))
    b_row[:, 0] = KAPPA * np.sqrt(v_klw)
    # w_rec: n = (w + 1e-10) / sum; through s (the softmax's errors are correlated), plus each w's own rounding
    n, qs, oh = k['n'], k['qs'], k['oh']
    rel_n = np.sqrt(v_w) / (w + W2) + 3 * U                          # relative error of n
    b_n = KAPPA * n * rel_n
    if onehot is not None:
        nc = np.clip(n, O.EPS_K, 1 - O.EPS_K)
        # the clip points in fp32: 1e-7 -> float32(1e-7), 1 - 1e-7 -> 1 - 2^-23
        near_lo = A(n - O.EPS_K) <= b_n + A(O.EPS_K - EPS_LO32)
        near_hi = (n >= EPS_HI32 - b_n) & (n <= 1 - O.EPS_K + b_n)
        flags['clip_w'] = (near_lo | near_hi) & (oh != 0)
        ins = k['ins']
        g = np.where(ins, -C1 * oh / nc, 0.0)                        # d w_rec / d n
        # d w_rec / d s_k = sum_j g_j dn_j/ds_k: dn_j/ds_k ~ n_j (delta_jk - n_k) (renormalised softmax)
        gs = n * (g - (g * n).sum(1, keepdims=True))
        v_wrec = (sq(gs) * v_se).sum(1) + (sq(g * n * U) * (C / 3.0 + RCP_ULP ** 2 + 4)).sum(1)
        loc = C1 * A(oh) * (LOG_ABS * U + 2 * U * A(np.log(nc)) + U)
        v_wrec += (sq(loc)).sum(1) + sq(U * (C1 * A(oh * np.log(nc))).sum(1)) * C / 3.0
        # a flagged clip: the term may be clipped or not -- the difference of the two
        fl = flags['clip_w']
        v_wrec += (np.where(fl, sq(C1 * A(oh) * (A(np.log(np.maximum(n, 1e-300))) - A(np.log(nc))) + C1 * U * 4), 0.0)).sum(1)
        b_row[:, 1] = KAPPA * np.sqrt(v_wrec)
        # near ties of the arg max (hit)
        order = np.argsort(-w, 1, kind='stable')
        top = np.take_along_axis(w, order[:, :2], 1)
        bw = KAPPA * np.sqrt(np.take_along_axis(v_w, order[:, :2], 1)).sum(1)
        gap = top[:, 0] - top[:, 1]
        flags['tie'] = (gap > 0) & (gap <= bw)
    else:
        flags['clip_w'] = np.zeros((B, C), bool)
        flags['tie'] = np.zeros(B, bool)
    # h = relu([x, w] Kh + bh): x exact
    v_xw = np.concatenate([np.zeros_like(x), v_w], 1)
    v_ah = dense(k['xw'], v_xw, Kh, bh, 'xw')
    flags['relu_h'] = A(k['a_h']) <= KAPPA * np.sqrt(v_ah)
    v_hh = cut(v_ah, k['a_h'], flags['relu_h'])
    v_za = dense(k['h'], v_hh, Kza, bza, 'h')
    zm, zlv, sdz, z = k['zm'], k['zlv'], k['sdz'], k['z']
    vzm, vzlv = v_za[:, :L], v_za[:, L:]
    v_z = vzm + sq(sdz * eps_z) * expv(0.5 * zlv, 0.25 * vzlv) + sq(U * A(sdz * eps_z)) + sq(U * A(z))
    tk = 1 + A(zlv) + zm * zm + sdz * sdz
    v_kl = 0.25 * ((4 * sq(zm) * vzm + sq(1 - sdz * sdz) * vzlv).sum(1)
                   + (sq(4 * U * tk) + sq(2 * (EXP_ULP + 0.5 * A(zlv)) * U * sdz * sdz)).sum(1)
                   + sq(U * tk.sum(1)) * L / 3.0)
    b_kl = KAPPA * np.sqrt(v_kl)
    v_wz = np.concatenate([v_w, np.zeros_like(xp), v_z] if use_x_prev else [v_w, v_z], 1)
    v_adh = dense(k['wz'], v_wz, Kd, bd, 'wz')
    flags['relu_dh'] = A(k['a_dh']) <= KAPPA * np.sqrt(v_adh)
    v_hd = cut(v_adh, k['a_dh'], flags['relu_dh'])
    v_l = dense(k['hd'], v_hd, Ko, bo, 'hd')
    b_l = KAPPA * np.sqrt(v_l)
    logits, l, el, y = r['logits'], k['l'], k['el'], k['y']
    lo, hi = O.LOGIT_CLIP_LO, O.LOGIT_CLIP_HI
    slack = 4e-6                                                     # the fp32 clip constants against the fp64 ones
    flags['clip_l'] = (A(logits - lo) <= b_l + slack) | (A(logits - hi) <= b_l + slack)
    inside = (logits >= lo) & (logits <= hi)
    sg = O.sigmoid(l)
    gl = np.where(inside | flags['clip_l'], A(sg - y), 0.0)          # d term / d logit
    tn = A(np.maximum(l, 0)) + A(np.log1p(el)) + A(l * y)
    v_nll = (sq(gl) * v_l).sum(1) + (sq(U * (2 * tn + LOG_ABS)) + sq(el / (1 + el) * (EXP_ULP + A(l)) * U)).sum(1) \
        + sq(U * tn.sum(1)) * D / 3.0
    b_nll = KAPPA * np.sqrt(v_nll)
    r.update(b_logits=b_l, b_w=KAPPA * np.sqrt(v_w), b_wargs=KAPPA * np.sqrt(v_wa), b_zargs=KAPPA * np.sqrt(v_za),
             b_rownll=b_nll, b_rowkl=b_kl, b_rowloss=b_row)
    r['flags'] = flags
    if not need_grads:
        return r
    # ---- backward ----
    inv_b = 1.0 / B
    # dl = inv_b (sigmoid(l) - y) inside the clip; flagged: it may be 0 or not
    v_dl = np.where(inside, sq(inv_b * sg * (1 - sg)) * v_l + sq(inv_b * sg * U * (RCP_ULP + EXP_ULP + A(l) + 2))
                    + sq(inv_b * U * A(sg - y)), 0.0)
    v_dl = v_dl + np.where(flags['clip_l'], sq(inv_b * A(sg - y)), 0.0)
    dl, g1, g2, g3 = k['dl'], k['g1'], k['g2'], k['g3']

    def masked(pre_var, pre, mask_edge):
        """variance of (product) * mask: 0 where masked off and not near the edge; near the edge the whole value"""
        return np.where(mask_edge, sq(A(pre)) + pre_var, np.where(pre != 0, pre_var, 0.0))

    v_g1p = dense(dl, v_dl, Ko, None, 'dl', T=True)
    g1p = R(dl) @ R(Ko).T
    v_g1 = np.where(flags['relu_dh'], sq(g1p) + v_g1p, np.where(k['a_dh'] > 0, v_g1p, 0.0))
    xo = D if use_x_prev else 0
    v_dwdec = dense(g1, v_g1, Kd[:C], None, 'g1', T=True)
    v_dz = dense(g1, v_g1, Kd[C + xo:], None, None, T=True)
    ks, dz = kl_weight * inv_b, k['dz']
    v_dzm = v_dz + sq(ks) * vzm + sq(U * (A(dz) + 2 * A(ks * zm)))
    t1 = dz * eps_z * 0.5 * sdz
    t2 = 0.5 * ks * (1 - sdz * sdz)
    v_dzlv = sq(eps_z * 0.5 * sdz) * v_dz + sq(0.5 * t1 + ks * 0.5 * sdz * sdz) * vzlv \
        + sq(U * (4 * A(t1) + 3 * A(t2) + A(ks) * sdz * sdz)) + sq((EXP_ULP + 0.5 * A(zlv)) * U * (A(t1) + A(ks) * sdz * sdz))
    v_dza = np.concatenate([v_dzm, v_dzlv], 1)
    g2p = R(k['dza']) @ R(Kza).T
    v_g2p = dense(k['dza'], v_dza, Kza, None, 'dza', T=True)
    v_g2 = np.where(flags['relu_h'], sq(g2p) + v_g2p, np.where(k['a_h'] > 0, v_g2p, 0.0))
    v_dw = v_dwdec + dense(g2, v_g2, Kh[D:], None, 'g2', T=True) + sq(U * A(k['dw']))
    # label backward: d = dw + cw inv_b (dn - dot) / qs; ds = w (d - sum d w); dwm, dwlv
    d, dsum = k['d'], k['dsum']
    cwb = class_weight * inv_b
    dn = k['dn']
    tcw = cwb * (dn - k['dot']) / qs
    v_t = sq(cwb * dn / qs) * sq(rel_n) + sq(U * 4 * (A(tcw) + A(cwb * dn / qs)))
    if onehot is not None:
        fl = flags['clip_w']                                          # dn may be 0 or -C1 / n there
        v_t = v_t + np.where(fl.any(1, keepdims=True), sq(cwb * (C1 * A(oh) / np.maximum(nc, O.EPS_K)).sum(1, keepdims=True) / qs) * 4, 0.0)
    v_d = v_dw + v_t + sq(U * A(d))
    totd = (sq(w) * v_d).sum(1, keepdims=True)
    v_ds = sq(w) * np.maximum((1 - 2 * w) * v_d + totd, 0.0)
    # through w (independent roundings of each w_j): d ds_j / d w_j = d_j - dsum - w_j d_j, d ds_j / d w_k = -w_j d_k
    tw = (sq(d) * v_w).sum(1, keepdims=True)
    v_ds += sq(d - dsum - w * d) * v_w + sq(w) * np.maximum(tw - sq(d) * v_w, 0.0)
    v_ds += sq(U * 2 * (A(w * (d - dsum)) + A(w) * (A(d * w)).sum(1, keepdims=True)))
    v_ds = v_ds[:, :C1]
    ds = k['ds']
    a1 = wkl = w_kl_weight * inv_b
    v_dwm = v_ds + sq(wkl / ep) * vm + sq(U * (A(ds) + 3 * A(wkl * m / ep)) + (EXP_ULP + A(prior)) * U * A(wkl * m / ep))
    u1 = ds * ew * 0.5 * sdw
    u2 = wkl * 0.5 * (1 - sdw * sdw / ep)
    v_dwlv = sq(ew * 0.5 * sdw) * v_ds + sq(0.5 * u1 + a1 * 0.5 * sdw * sdw / ep) * vlv \
        + sq(U * (4 * A(u1) + 4 * A(u2) + 2 * wkl * sdw * sdw / ep)) \
        + sq((EXP_ULP + 0.5 * A(lv)) * U * (A(u1) + wkl * sdw * sdw / ep) + (EXP_ULP + A(prior)) * U * wkl * sdw * sdw / ep)
    v_dwa = np.concatenate([v_dwm, v_dwlv], 1)
    g3p = R(k['dwa']) @ R(Kwa).T
    v_g3p = dense(k['dwa'], v_dwa, Kwa, None, 'dwa', T=True)
    v_g3 = np.where(flags['relu_hw'], sq(g3p) + v_g3p, np.where(k['a_hw'] > 0, v_g3p, 0.0))

    def wgrad(GA, vGA, DY, vDY, name):
        """variance of GA^T . DY (a dot over the B batch rows) and of DY's column sums (fp32, never rounded to bf16)"""
        ga, vga = operand(GA, vGA, name + '_ga')
        dy, vdy = operand(DY, vDY, name + '_dy')
        vk = vga.T @ sq(dy) + sq(ga).T @ vdy + sq(U * (A(ga).T @ A(dy))) * (B + 1) / 3.0
        vb = vDY.sum(0) + sq(U * A(DY).sum(0)) * (B + 1) / 3.0
        return vk, vb

    pairs = [(x, np.zeros_like(x), g3, v_g3, 'hw'), (k['hw'], v_hw, k['dwa'], v_dwa, 'wa'),
             (k['xw'], v_xw, g2, v_g2, 'h'), (k['h'], v_hh, k['dza'], v_dza, 'za'),
             (k['wz'], v_wz, g1, v_g1, 'dh'), (k['hd'], v_hd, dl, v_dl, 'o')]
    bg = []
    for GA, vGA, DY, vDY, name in pairs:
        vk, vb = wgrad(GA, vGA, DY, vDY, name)
        bg += [KAPPA * np.sqrt(vk), KAPPA * np.sqrt(vb)]
    r['b_grads'] = bg
    return r


def evaluate32(P, x, xp, onehot, eps_w, eps_z, prior, class_weight, kl_weight, w_kl_weight, use_x_prev, target=None,
               need_grads=True, bf16_mode=False, seed=0, faults=()):
    """an fp32 evaluation of the same contract (see F32); faults: planted faults for the sensitivity tests"""
    ar = F32(np.random.default_rng(seed))
    f = lambda a: None if a is None else np.asarray(a, np.float32)
    r, _ = _values(ar, [f(t) for t in P], f(x), f(xp), f(onehot), f(eps_w), f(eps_z), prior, class_weight, kl_weight,
                   w_kl_weight, use_x_prev, f(target), need_grads, bf16_mode, faults)
    return r


# ------------------------------------------------------------------------------------------------------- comparison --
def ratios(got, ref):
    """worst |got - ref| / bound per output (rowloss: the kl_w and w_rec columns; grads: each of the 12 tensors); NaN in
    got gives inf"""
    def one(g, rf, b):
        e = np.abs(np.asarray(g, np.float64) - rf)
        q = np.where(e == 0, 0.0, e / np.maximum(b, 1e-300))
        return float(np.nan_to_num(q, nan=np.inf).max()) if q.size else 0.0
    out = {k: one(got[k], ref[k], ref['b_' + k]) for k in OUTPUTS if k != 'rowloss' and k in got}
    if 'rowloss' in got:
        out['rowloss'] = one(np.asarray(got['rowloss'])[:, :2], ref['rowloss'][:, :2], ref['b_rowloss'][:, :2])
    if 'grads' in got and 'grads' in ref:
        for i, nm in enumerate(NAMES):
            out['grad ' + nm] = one(got['grads'][i], ref['grads'][i], ref['b_grads'][i])
    return out


def violations(got, ref):
    """[(output, worst ratio)] of the outputs whose worst error exceeds its bound, plus ('hit', rows) where hit differs
    outside the flagged near-tie rows"""
    bad = [(k, v) for k, v in ratios(got, ref).items() if not v <= 1.0]
    hit = np.asarray(got['rowloss'], np.float64)[:, 2]
    rows = np.flatnonzero(~ref['flags']['tie'] & (hit != ref['rowloss'][:, 2]))
    if rows.size:
        bad.append(('hit', rows[:8].tolist()))
    return bad


def flag_counts(ref):
    return {k: int(np.sum(v)) for k, v in ref['flags'].items()}


# ------------------------------------------------------------------------------------------------------------ cases --
def make_case(seed, B, D, H, Hc, C, L, use_x_prev, target=False, onehot=True, prior=0.3, weights=(1.0, 0.7, 1.3, 0.9)):
    """a step's inputs, all fp32 values: glorot-uniform kernels, small random biases, 0/1 frames (~15 % notes), one-hot
    labels, standard normal eps; target: a next frame unlike x.  weights = class_weight, kl_weight, w_kl_weight, 1/B-free
    scale of the biases."""
    rng = np.random.default_rng(seed)
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    P = []
    for s in shapes(D, H, Hc, C, L, use_x_prev):
        if len(s) == 2:
            a = np.sqrt(6.0 / (s[0] + s[1]))
            P.append(f(rng.uniform(-a, a, s)))
        else:
            P.append(f(rng.standard_normal(s) * 0.1 * weights[3]))
    frames = lambda: (rng.random((B, D)) < 0.15).astype(np.float64)
    x, xp = frames(), frames()
    return dict(P=P, x=x, xp=xp, target=frames() if target else None,
                onehot=np.eye(C)[rng.integers(0, C, B)] if onehot else None,
                eps_w=f(rng.standard_normal((B, C - 1))), eps_z=f(rng.standard_normal((B, L))), prior=prior,
                class_weight=weights[0], kl_weight=weights[1], w_kl_weight=weights[2], use_x_prev=use_x_prev)


def edge_case(B=34, D=20, H=24, Hc=12, C=5, L=3, use_x_prev=True):
    """logits past both clip points (two output columns), a w_rec row in the lower clip, an exact tie in w and in onehot
    (identical fp32 computations: a row without notes and eps_w = 0, onehot with two equal entries)"""
    case = make_case(5, B, D, H, Hc, C, L, use_x_prev, target=True)
    P = [t.copy() for t in case['P']]
    P[11][0], P[11][1] = 60.0, -60.0                  # x_decoded_mean bias: column 0 above BCE_CLIP_HI, column 1 below LO
    P[3][:] = 0.0                                     # wargs bias 0, the x-free row's wargs are exactly 0 ...
    P[1][:] = -np.abs(P[1])                           # ... because h_w = relu(bias <= 0) = 0 there
    x, ew, oh = case['x'].copy(), case['eps_w'].copy(), case['onehot'].copy()
    x[2], ew[2] = 0.0, 0.0                            # row 2: w = 1/C in every class exactly
    oh[2] = 0.0
    oh[2, 1] = oh[2, 3] = 1.0                         # a tie in onehot too: first index 1 against w's first index 0 -> hit 0
    x[3], ew[3] = 0.0, 0.0
    ew[3, 0] = -60.0                                  # row 3: w[0] ~ e^-60 -> n below 1e-7, the true class
    oh[3] = np.eye(C)[0]
    return dict(case, P=P, x=x, eps_w=ew, onehot=oh)


def call(fn, case, **kw):
    """fn (reference / evaluate32) on a make_case dict"""
    c = dict(case)
    return fn(c.pop('P'), c.pop('x'), c.pop('xp'), c.pop('onehot'), c.pop('eps_w'), c.pop('eps_z'), c.pop('prior'),
              c.pop('class_weight'), c.pop('kl_weight'), c.pop('w_kl_weight'), c.pop('use_x_prev'), target=c.pop('target'),
              **kw)
