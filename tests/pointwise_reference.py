"""fp64 reference of the entry points of csrc/pointwise.hip (all but clv_gather_rows_multi), with per-element bounds, flags,
the case tables that tests/test_pointwise_reference.py (no GPU) and tests/test_gpu_pointwise.py share, and an fp32 evaluation
of the same contracts in which faults can be planted.

Written from the contracts of include/clvae.h, not from the kernels' structure, out of oracle/clvae_oracle.py pieces:

  label_fwd   w = O.logistic_normal; rowloss = (O.kl_w_prior row term, O.cce_keras(w, onehot, C - 1), hit by the first-index
              argmax rule of O.categorical_accuracy); without onehot columns 1 and 2 are zero
  label_bwd   d = dw + class_weight inv_b dcce(w); (ds, dlv) = O.logistic_normal_bwd(w, d); + w_kl_weight inv_b dkl_w
  gauss_*     z = mean + exp(lv / 2) eps, rowkl and its derivatives from O.kl_gauss
  bernoulli   O.bce_from_logits_keras with the float32 clip points O.LOGIT_CLIP_LO / HI
  the rest    sums, means, column sums, copies and the elementwise formulas as the header states them.

Inputs are rounded to fp32 first; every ref_* function returns {output: (want, bound, flags)}.

bounds      A sum or dot gets  BOUND_K 2^-24 sum |terms|  (label_reference.py's form, BOUND_K = 32), and the bounds of a
            stage's inputs are carried through its first derivative.  The elementwise outputs have derived budgets, in
            U = 2^-24:
              * an ordinary fp32 operation: one ulp of its result, 2 U relative -- twice the half ulp of a correctly rounded
                one, so that a product and sum may be fused or not and a division may be a reciprocal and a product (OP);
              * __expf(x) = v_exp_f32(x log2 e): the rounded exponent costs |x| U, the instruction one ulp: (|x| + 2) U;
              * __logf and v_rcp_f32: one ulp of their result, 2 U relative; the product with ln 2 inside __logf is an OP;
              * __logf(1 + e) for e -> 0: 1 + e rounds, an absolute 2^-23 = 2 U.
              * expf / logf of the device library (label and gauss kernels): one ulp.
            gauss z and dzargs and the last stages of label_bwd (d, ds, dmean, dlogvar) are counted out in these units in
            the code; only what is a sum over a row (S, Q, dot, dsum, kl_w, w_rec, rowkl) keeps the BOUND_K form.
            So  sigmoid = rcp(1 + e) [* e],  e = __expf(-|x|):  s ((1 - s)(|x| + 2) U + 3 OP)   (1 + e, rcp, the product);
            softplus(l) - l t per element: s(-|l|)(|l| + 2) U + 2 OP log1p(e) + 2 U + OP (|softplus| + |l t| + |term|).
flags       bernoulli: logits within BOUND_K U |clip| of a clip point (the fp32 constants of the kernel against the fp64
            ones of the oracle) -- their dlogits may be zero or not; label_bwd: rows in which a renormalised probability
            that carries weight lies within its bound of 1e-7 or 1 - 1e-7; label_fwd: rows whose two largest w lie within
            their bounds of each other but are not equal (hit).  An exact fp64 tie is not flagged: first index wins.
exact       bound None: the 32 bits are compared (scale_temper, the samplers, take_frame, gather_rows, act_grad NONE / RELU);
            bound 0: equal as numbers (lerp_rows at alpha 0 and 1, dropout_rows with beta 0, hit, the masked-out elements).
"""
import numpy as np

from helpers import CANARY
from oracle import clvae_oracle as O

U = 2.0 ** -24
BOUND_K = 32
OP = 2 * U                      # an ordinary fp32 operation, relative to its result
f32, f64 = np.float32, np.float64
A = np.abs


def _b(*terms):
    return BOUND_K * U * sum(terms)


def r32(a):
    return None if a is None else np.asarray(a, f32).astype(f64)


# ------------------------------------------------------------------------------------------------------------ checker --
def check(name, got, want, bound, flags=None):
    """every element of got within its bound of want, flagged elements excepted (they must still be finite).  Returns the
    worst error / bound ratio (0 where bound = 0 and got = want); raises naming the first offending index."""
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
        raise AssertionError("%s%s: got %.9g, expected %.9g, error %.3g = %.3g x its bound %.3g (%d of %d elements off)"
                             % (name, list(i), got[i], want[i], err[i], ratio[i], bound[i], len(bad), want.size))
    return float(ratio.max()) if ratio.size else 0.0


def check_bits(name, got, want):
    """got and want as fp32, bit for bit (uint8 / integer arrays: equal)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (name, got.shape, want.shape)
    g = got.astype(f32).view(np.uint32) if got.dtype.kind == 'f' else got
    w = want.astype(f32).view(np.uint32) if want.dtype.kind == 'f' else want
    bad = np.argwhere(g != w)
    if bad.size:
        i = tuple(int(x) for x in bad[0])
        raise AssertionError("%s%s: got %r, expected %r bit for bit (%d of %d elements off)"
                             % (name, list(i), got[i], want[i], len(bad), want.size))
    return 0.0


def check_all(name, got, ref):
    """{output: array} against {output: (want, bound, flags)}; bound None: bit for bit.  Returns {output: ratio}."""
    assert set(got) == set(ref), (name, sorted(got), sorted(ref))
    return {k: check_bits(name + ' ' + k, got[k], ref[k][0]) if ref[k][1] is None
            else check(name + ' ' + k, got[k], *ref[k]) for k in sorted(ref)}


# ---------------------------------------------------------------------------------------------- fp32 building blocks --
def exp32(x):
    """correctly rounded fp32 exp (numpy's own float32 exp differs between builds)"""
    return np.exp(np.asarray(x, f32).astype(f64)).astype(f32)


def log32(x):
    return np.log(np.asarray(x, f32).astype(f64)).astype(f32)


def sum32(x, axis=-1, order='forward'):
    """fp32 sum along axis in a fixed order: 'forward', 'reversed' (sequential) or 'pairwise' (halving tree)"""
    x = np.moveaxis(np.asarray(x, f32), axis, -1)
    if order == 'pairwise':
        n = 1
        while n < x.shape[-1]:
            n *= 2
        y = np.zeros(x.shape[:-1] + (n,), f32)
        y[..., :x.shape[-1]] = x
        while n > 1:
            n //= 2
            y = y[..., :n] + y[..., n:2 * n]
        return y[..., 0]
    if order == 'reversed':
        x = x[..., ::-1]
    else:
        assert order == 'forward', order
    if x.shape[-1] == 0:
        return np.zeros(x.shape[:-1], f32)
    return np.cumsum(x, axis=-1, dtype=f32)[..., -1]


ORDERS = ('forward', 'reversed', 'pairwise')


# -------------------------------------------------------------------------------------------------------------- label --
def _label_w_bound(m, lv, eps, W):
    sd = np.exp(0.5 * lv)
    b_s = np.concatenate([_b(A(m), sd * A(eps)), np.zeros((m.shape[0], 1))], 1)
    return W * (b_s + (W * b_s).sum(1, keepdims=True)) + _b(W)


def ref_label_fwd(mean, logvar, eps, onehot, prior, rowloss=True, **_):
    m, lv, eps, onehot = r32(mean), r32(logvar), r32(eps), r32(onehot)
    prior = float(f32(prior))
    B, C1 = m.shape
    W = O.logistic_normal(m, lv, eps)
    bW = _label_w_bound(m, lv, eps, W)
    out = dict(w=(W, bW, None))
    if not rowloss:
        return out
    sd2, ep = np.exp(lv), np.exp(prior)
    rl, b = np.zeros((B, 3)), np.zeros((B, 3))
    flags = np.zeros((B, 3), bool)
    rl[:, 0] = O.kl_w_prior(m, lv, prior)[0]
    b[:, 0] = 0.5 * _b(A(1 - prior) + A(lv) + sd2 / ep + m * m / ep).sum(1)
    if onehot is not None:
        rl[:, 1] = O.cce_keras(W, onehot, C1)[0]
        q = W + O.W2_SHIFT
        Q = q.sum(1, keepdims=True)
        n = q / Q
        bn = n * (bW / q + bW.sum(1, keepdims=True) / Q) + _b(n)
        lo = np.maximum(n - bn, O.EPS_K)
        nc = np.clip(n, O.EPS_K, 1 - O.EPS_K)
        b[:, 1] = C1 * (A(onehot) * (bn / lo + _b(A(np.log(nc))) + U)).sum(1)
        rl[:, 2] = np.argmax(onehot, 1) == np.argmax(W, 1)              # np.argmax: the first index on ties
        top = -np.sort(-W, 1)
        it = np.argsort(-W, 1, kind='stable')
        gap = top[:, 0] - top[:, 1] if C1 > 0 else np.ones(B)
        flags[:, 2] = (gap > 0) & (gap <= np.take_along_axis(bW, it[:, :2], 1).sum(1))
    out['rowloss'] = (rl, b, flags)
    return out


def ref_label_bwd(mean, logvar, eps, onehot, w, dw, prior, class_weight, w_kl_weight, inv_b, **_):
    """w [B,C] is an INPUT here (what a forward left behind), exact like the others"""
    m, lv, eps, onehot, W, dw = r32(mean), r32(logvar), r32(eps), r32(onehot), r32(w), r32(dw)
    prior, cw, wkl, inv_b = (float(f32(x)) for x in (prior, class_weight, w_kl_weight, inv_b))
    C1 = m.shape[1]
    k1, k2 = cw * inv_b, wkl * inv_b
    _, drec = O.cce_keras(W, onehot, C1)
    d = dw + k1 * drec
    ds, dlv_s = O.logistic_normal_bwd(W, d, lv, eps)
    _, dm_kl, dlv_kl = O.kl_w_prior(m, lv, prior)
    dmean, dlogvar = ds + k2 * dm_kl, dlv_s + k2 * dlv_kl
    # bounds, stage by stage
    q = W + O.W2_SHIFT
    Q = q.sum(1, keepdims=True)
    n = q / Q
    nc = np.clip(n, O.EPS_K, 1 - O.EPS_K)
    inside = (n >= O.EPS_K) & (n <= 1 - O.EPS_K)
    dn = np.where(inside, -C1 * onehot / nc, 0.0)
    b_n = _b(n)
    b_dn = A(dn) * (b_n / nc + OP)
    dot = (dn * n).sum(1, keepdims=True)
    b_dot = (b_dn * n + A(dn) * b_n).sum(1, keepdims=True) + _b((A(dn) * n).sum(1, keepdims=True))
    # (dn - dot) / Q: the difference, the quotient, and Q itself, a sum of C terms
    b_drec = (b_dn + b_dot) / Q + 2 * OP * (A(dn) + A(dot)) / Q + _b(A(drec))
    # dw + (class_weight inv_b) drec: two products and the sum
    b_d = A(k1) * b_drec + 2 * OP * A(k1 * drec) + OP * A(d)
    dsum = (d * W).sum(1, keepdims=True)
    b_dsum = (b_d * W).sum(1, keepdims=True) + _b((A(d) * W).sum(1, keepdims=True))
    b_ds = (W * (b_d + b_dsum) + 2 * OP * W * (A(d) + A(dsum)))[:, :C1]                  # w (d - dsum): the difference, the product
    sd, ep = np.exp(0.5 * lv), np.exp(prior)
    EP = (A(prior) + 2) * U                                                               # __expf(prior), relative
    # ds + (w_kl_weight inv_b) (m / ep): ep, the quotient, two products; the sum
    b_dm = b_ds + A(k2 * m / ep) * (EP + 3 * OP) + OP * A(dmean)
    # ds eps 0.5 sd (expf, two products) + k2 (-0.5 (1 - sd sd / ep)): sd twice, the square, ep, the quotient; the difference; two
    # products; the sum
    t1, v, t2 = ds * eps * 0.5 * sd, sd * sd / ep, k2 * dlv_kl
    b_dlv = b_ds * A(eps) * 0.5 * sd + 3 * OP * A(t1) + A(k2) * 0.5 * ((4 * OP + EP) * v + OP * A(1 - v)) + 2 * OP * A(t2) + \
        OP * A(dlogvar)
    near = (A(n - O.EPS_K) <= b_n) | (n >= 1 - O.EPS_K - b_n - 2 * U)
    flag = ((onehot != 0) & near).any(1, keepdims=True)
    return dict(dmean=(dmean, b_dm, flag), dlogvar=(dlogvar, b_dlv, flag))


def f32_label_fwd(mean, logvar, eps, onehot, prior, rowloss=True, order='forward', fault=None, **_):
    m, lv, eps = (np.asarray(x, f32) for x in (mean, logvar, eps))
    prior = f32(prior)
    B, C1 = m.shape
    sd = exp32(f32(0.5) * lv)
    e = np.concatenate([exp32(m + sd * eps), np.ones((B, 1), f32)], 1)
    W = (e / sum32(e, 1, order)[:, None]).astype(f32)
    out = dict(w=W)
    if not rowloss:
        return out
    ep = exp32(prior)
    terms = f32(1) - prior + lv - sd * sd / ep - m * m / ep
    if fault == 'kl_w without the prior':
        terms = f32(1) + lv - sd * sd - m * m
    rl = np.zeros((B, 3), f32)
    rl[:, 0] = f32(-0.5) * sum32(terms, 1, order)
    if onehot is not None:
        y = np.asarray(onehot, f32)
        q = W + f32(O.W2_SHIFT)
        n = q / sum32(q, 1, order)[:, None]
        nc = np.clip(n, f32(O.EPS_K), f32(1) - f32(O.EPS_K))
        rl[:, 1] = f32(C1) * sum32(-y * log32(nc), 1, order)
        am = W.shape[1] - 1 - np.argmax(W[:, ::-1], 1) if fault == 'last-index argmax' else np.argmax(W, 1)
        rl[:, 2] = np.argmax(y, 1) == am
    out['rowloss'] = rl
    return out


def f32_label_bwd(mean, logvar, eps, onehot, w, dw, prior, class_weight, w_kl_weight, inv_b, order='forward', fault=None, **_):
    m, lv, eps, y, W, dw = (np.asarray(x, f32) for x in (mean, logvar, eps, onehot, w, dw))
    prior, cw, wkl, inv_b = f32(prior), f32(class_weight), f32(w_kl_weight), f32(inv_b)
    C1 = m.shape[1]
    q = W + f32(O.W2_SHIFT)
    Q = sum32(q, 1, order)[:, None]
    n = q / Q
    lo, hi = f32(O.EPS_K), f32(1) - f32(O.EPS_K)
    inside = (n >= lo) & (n <= hi)
    dn = np.where(inside, -f32(C1) * y / np.clip(n, lo, hi), f32(0)).astype(f32)
    dot = sum32(dn * n, 1, order)[:, None]
    d = dw + cw * inv_b * ((dn - dot) / Q)
    dsum = sum32(d * W, 1, order)[:, None]
    ds = (W * (d - dsum))[:, :C1]
    sd, ep = exp32(f32(0.5) * lv), exp32(prior)
    half = f32(1.0 if fault == 'dlogvar without its half' else 0.5)
    return dict(dmean=ds + wkl * inv_b * (m / ep),
                dlogvar=ds * eps * half * sd + wkl * inv_b * (f32(-0.5) * (f32(1) - sd * sd / ep)))


# -------------------------------------------------------------------------------------------------------------- gauss --
def ref_gauss_fwd(zargs, eps, rowkl=True, **_):
    za, eps = r32(zargs), r32(eps)
    L = eps.shape[1]
    m, lv = za[:, :L], za[:, L:]
    sd = np.exp(0.5 * lv)
    z = m + sd * eps
    out = dict(z=(z, 2 * OP * sd * A(eps) + OP * A(z), None))               # expf (one ulp) and the product; the sum
    if rowkl:
        out['rowkl'] = (O.kl_gauss(m, lv)[0], 0.5 * _b(1 + A(lv) + m * m + sd * sd).sum(1), None)
    return out


def ref_gauss_bwd(zargs, eps, dz, kl_scale, **_):
    za, eps, dz = r32(zargs), r32(eps), r32(dz)
    kls = float(f32(kl_scale))
    L = eps.shape[1]
    m, lv = za[:, :L], za[:, L:]
    sd = np.exp(0.5 * lv)
    _, dm, dlv = O.kl_gauss(m, lv)
    want = np.concatenate([dz + kls * dm, dz * eps * 0.5 * sd + kls * dlv], 1)
    # dz + kls m: the product, the sum.  dz eps 0.5 sd: expf and two products; 0.5 kls (1 - sd sd): sd twice and the square,
    # the difference, two products; then the difference of the two
    t1, t2 = dz * eps * 0.5 * sd, kls * dlv
    bound = np.concatenate([OP * (A(kls * m) + A(want[:, :L])),
                            3 * OP * A(t1) + 0.5 * A(kls) * (3 * OP * sd * sd + OP * A(1 - sd * sd)) + 2 * OP * A(t2) +
                            OP * A(want[:, L:])], 1)
    return dict(dzargs=(want, bound, None))


def f32_gauss_fwd(zargs, eps, rowkl=True, order='forward', fault=None, **_):
    za, eps = np.asarray(zargs, f32), np.asarray(eps, f32)
    L = eps.shape[1]
    m, lv = za[:, :L], za[:, L:]
    sd = exp32(f32(0.5) * lv)
    out = dict(z=m + sd * eps)
    if rowkl:
        term = f32(1) + lv - m * m - sd * sd
        if fault == '32 lanes' and L > 32:
            term = term[:, :32]
        if fault == 'lane L-1 only':
            term = term[:, L - 1:]
        out['rowkl'] = f32(-0.5) * sum32(term, 1, order)
    return out


def f32_gauss_bwd(zargs, eps, dz, kl_scale, **_):
    za, eps, dz, kls = np.asarray(zargs, f32), np.asarray(eps, f32), np.asarray(dz, f32), f32(kl_scale)
    L = eps.shape[1]
    m, lv = za[:, :L], za[:, L:]
    sd = exp32(f32(0.5) * lv)
    return dict(dzargs=np.concatenate([dz + kls * m, dz * eps * f32(0.5) * sd - f32(0.5) * kls * (f32(1) - sd * sd)], 1))


# ---------------------------------------------------------------------------------------------------------- bernoulli --
def _sigmoid_bound(s, x):
    """rcp(1 + e) [* e] with e = __expf(-|x|), relative to s = sigmoid(x): see the module's docstring"""
    return s * ((1 - s) * (A(x) + 2) * U + 3 * OP)


def ref_bernoulli_nll(logits, y, scale, rownll=True, dlogits=True, **_):
    a, y = r32(logits), r32(y)
    scale = float(f32(scale))
    loss, g = O.bce_from_logits_keras(a, y)
    lo, hi = O.LOGIT_CLIP_LO, O.LOGIT_CLIP_HI
    l = np.clip(a, lo, hi)
    out = {}
    if rownll:
        e = np.exp(-A(l))
        lg = np.log1p(e)
        sp = np.maximum(l, 0) + lg
        term = sp - l * y
        b_el = e / (1 + e) * (A(l) + 2) * U + 2 * OP * lg + 2 * U + OP * (sp + A(l * y) + A(term))
        # a clipped logit is the kernel's fp32 clip constant, half an ulp from the oracle's: |d term / d l| <= 1 + |y|
        clipped = (a <= lo + _b(A(lo))) | (a >= hi - _b(A(hi)))
        b_el = b_el + clipped * U * A(l) * (1 + A(y))
        out['rownll'] = (loss, b_el.sum(1) + _b(A(term).sum(1)), None)
    if dlogits:
        s = O.sigmoid(l)
        b = A(scale) * (_sigmoid_bound(s, l) + OP * A(s - y)) + OP * A(scale * (s - y))
        flags = (A(a - lo) <= _b(A(lo))) | (A(a - hi) <= _b(A(hi)))
        out['dlogits'] = (scale * g, b, flags)
    return out


def f32_bernoulli_nll(logits, y, scale, rownll=True, dlogits=True, order='forward', fault=None, **_):
    a, y, scale = np.asarray(logits, f32), np.asarray(y, f32), f32(scale)
    lo, hi = f32(O.LOGIT_CLIP_LO), f32(16.118 if fault == 'symmetric clip' else O.LOGIT_CLIP_HI)
    l = np.clip(a, lo, hi)
    e = exp32(-A(l))
    out = {}
    if rownll:
        out['rownll'] = sum32(np.maximum(l, f32(0)) + log32(f32(1) + e) - l * y, 1, order)
    if dlogits:
        r1 = f32(1) / (f32(1) + e)
        sg = np.where(l >= 0, r1, e * r1).astype(f32)
        inside = (a >= lo) & (a <= hi) if fault != 'gradient outside the clip' else np.ones(a.shape, bool)
        out['dlogits'] = np.where(inside, scale * (sg - y), f32(0)).astype(f32)
    return out


# --------------------------------------------------------------------------------------------------------- reductions --
def ref_sum_strided(x, n, stride, scale, **_):
    v = r32(x)[:(n - 1) * stride + 1:stride]
    s = float(f32(scale))
    return dict(out=(np.array([s * v.sum()]), np.array([_b(A(s) * A(v).sum())]), None))


def f32_sum_strided(x, n, stride, scale, order='forward', fault=None, **_):
    v = np.asarray(x, f32)[:(n - 1) * stride + 1:stride]
    if fault == 'elements from 1024 on ignored':
        v = v[:1024]
    return dict(out=np.array([sum32(v, 0, order) * f32(scale)], f32))


def ref_loss_sums(terms, **_):
    """terms: five (flat array, n, stride); out[k] = the mean of term k's n strided elements"""
    vs = [r32(x)[:(n - 1) * st + 1:st] for x, n, st in terms]
    return dict(out=(np.array([v.sum() / v.size for v in vs]), np.array([_b(A(v).sum()) / v.size for v in vs]), None))


def f32_loss_sums(terms, order='forward', fault=None, **_):
    out = []
    for x, n, st in terms:
        x = np.asarray(x, f32)
        v = x[:n] if fault == 'strided term read contiguously' else x[:(n - 1) * st + 1:st]
        if fault == 'tail dropped' and st == 1:
            v = v[:4 * (n // 4)]
        den = 4 * (n // 4) if fault == 'divided by 4 (n / 4)' else n
        with np.errstate(divide='ignore', invalid='ignore'):
            out.append(sum32(v, 0, order) / f32(den))
    return dict(out=np.array(out, f32))


def ref_colsum(X, beta, out0, **_):
    X, beta = r32(X), float(f32(beta))
    base = beta * r32(out0) if beta != 0 else np.zeros(X.shape[1])
    return dict(out=(base + X.sum(0), _b(A(X).sum(0), A(base)), None))


def f32_colsum(X, beta, out0, order='forward', fault=None, **_):
    X, beta = np.asarray(X, f32), f32(beta)
    M = X.shape[0]
    rows = np.arange(M)
    if fault == 'small: rows 16..31 dropped' and M <= 1024:
        X = X[rows % 32 < 16]
    if fault == 'two-stage: ragged last chunk dropped' and M > 1024:
        X = X[:64 * (M // 64)]
    if fault == 'beta ignored':
        beta = f32(0)
    base = beta * np.asarray(out0, f32) if beta != 0 else np.zeros(X.shape[1], f32)
    return dict(out=base + sum32(X, 0, order))


# -------------------------------------------------------------------------------------------------------- elementwise --
def ref_axpy(alpha, x, y, **_):
    al, x, y = float(f32(alpha)), r32(x), r32(y)
    want = y + al * x
    return dict(y=(want, OP * (A(al * x) + A(want)), None))


def f32_axpy(alpha, x, y, **_):
    return dict(y=np.asarray(y, f32) + f32(alpha) * np.asarray(x, f32))


ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2          # CLV_ACT_* of include/clvae.h (asserted against _lib by the tests)


def ref_act_grad(act, y, dy, **_):
    v, g = r32(y), r32(dy)
    if act == ACT_SIGMOID:
        want = g * v * (1 - v)
        return dict(dpre=(want, 3 * OP * A(want), None))
    return dict(dpre=(np.where(v > 0, g, 0.0) if act == ACT_RELU else g, None, None))


def f32_act_grad(act, y, dy, **_):
    v, g = np.asarray(y, f32), np.asarray(dy, f32)
    return dict(dpre=g * v * (f32(1) - v) if act == ACT_SIGMOID else np.where(v > 0, g, f32(0)).astype(f32) if act == ACT_RELU else g)


def ref_scale_temper(alpha, x, **_):
    return dict(x=((float(f32(alpha)) * r32(x)).astype(f32), None, None))           # the fp64 product of two fp32 is exact


def f32_scale_temper(alpha, x, **_):
    return dict(x=f32(alpha) * np.asarray(x, f32))


def ref_sigmoid_temper(alpha, x, **_):
    v = (float(f32(alpha)) * r32(x)).astype(f32).astype(f64)                          # one rounding of the product
    xc = np.clip(v, -30.0, 30.0)
    s = O.sigmoid(xc)
    return dict(x=(s, _sigmoid_bound(s, xc), None))


def f32_sigmoid_temper(alpha, x, **_):
    xc = np.clip(f32(alpha) * np.asarray(x, f32), f32(-30), f32(30))
    return dict(x=f32(1) / (f32(1) + exp32(-xc)))


def ref_bernoulli_sample(p, u, **_):
    return dict(x=((np.asarray(u, f32) <= np.asarray(p, f32)).astype(f32), None, None))


def f32_bernoulli_sample(p, u, **_):
    return dict(x=ref_bernoulli_sample(p, u)['x'][0])


def f32_bernoulli_sample_clamped(p, u, clamp, counter, S, fault=None, **_):
    """p, u [R, D]; clamp [R, nsteps, D] uint8; step counter - S of the roll where it lies in [0, nsteps): bytes 0 / 1 force"""
    x = (np.asarray(u, f32) <= np.asarray(p, f32)).astype(f32)
    k = counter - S + (1 if fault == 'step c - S + 1' else 0)
    if 0 <= k < clamp.shape[1]:
        cb = clamp[:, k, :]
        x = np.where(cb <= (2 if fault == 'byte 2 clamps' else 1), np.minimum(cb, 1).astype(f32), x).astype(f32)
    return dict(x=x)


def ref_bernoulli_sample_clamped(p, u, clamp, counter, S, **_):
    return dict(x=(f32_bernoulli_sample_clamped(p, u, clamp, counter, S)['x'], None, None))


def f32_take_frame(src, step, out0, fault=None, **_):
    """src [R, T, D]; out0 [R, D]: what out held before"""
    src = np.asarray(src, f32)
    if 0 <= step < src.shape[1]:
        return dict(out=src[:, step, :].copy())
    return dict(out=np.zeros(out0.shape, f32) if fault == 'zeros outside the range' else np.asarray(out0, f32).copy())


def ref_take_frame(src, step, out0, **_):
    return dict(out=(f32_take_frame(src, step, out0)['out'], None, None))


def ref_lerp_rows(a, ia, b, ib, alpha, **_):
    """out[r] = (1 - alpha[r]) a[ia[r]] + alpha[r] b[ib[r]]; bound 0 (then bit for bit a's or b's row) where alpha is 0 or 1"""
    al = r32(alpha)[:, None]
    av, bv = r32(a)[ia], r32(b)[ib]
    want = (1 - al) * av + al * bv
    bound = OP * (A(al * av) + A((1 - al) * av) + A(al * bv) + A(want))
    want = np.where(al == 0, av, np.where(al == 1, bv, want))
    return dict(out=(want, np.where((al == 0) | (al == 1), 0.0, bound), None))


def f32_lerp_rows(a, ia, b, ib, alpha, fault=None, **_):
    al = np.asarray(alpha, f32)[:, None]
    av, bv = np.asarray(a, f32)[ia], np.asarray(b, f32)[ib]
    if fault == 'b dropped inside (0, 1)':
        bv = np.where(al == 1, bv, f32(0)).astype(f32)
    return dict(out=av + al * (bv - av) if fault == 'a + al (b - a)' else (av - al * av) + al * bv)


def f32_dropout_rows(X, Um, T, rate, beta, out0, fault=None, **_):
    """X [R, n], Um [R / T, n] uniforms, out0 [R, n]"""
    X, Um, rate, beta = np.asarray(X, f32), np.asarray(Um, f32), f32(rate), f32(beta)
    inv_keep = f32(1) / (f32(1) - rate)
    rows = np.arange(X.shape[0])
    u = Um[rows % Um.shape[0] if fault == 'mask row r' else rows // T]
    keep = u > rate if fault == 'mask >' else u >= rate
    v = X * np.where(keep, inv_keep, f32(0)).astype(f32)
    return dict(out=beta * np.asarray(out0, f32) + v if beta != 0 else v)


def ref_dropout_rows(X, Um, T, rate, beta, out0, **_):
    v = f32_dropout_rows(X, Um, T, rate, 0.0, out0)['out'].astype(f64)          # the mask decision and fl32(X m): exact
    beta = float(f32(beta))
    if beta == 0:
        return dict(out=(v, np.zeros(v.shape), None))
    want = beta * r32(out0) + v
    return dict(out=(want, OP * (A(beta * r32(out0)) + A(v) + A(want)), None))


def f32_gather_rows(src, idx, chunk, out_ld, fault=None, **_):
    """src [nsrc, row_elems]; returns [rows * pieces, out_ld] with CANARY in the columns a gather leaves alone"""
    src = np.asarray(src, f32)
    row_elems = src.shape[1]
    if chunk <= 0:
        chunk = out_ld = row_elems
    pieces = row_elems // chunk
    flat = np.full(len(idx) * pieces * out_ld, CANARY, f32)
    ld = chunk if fault == 'piece stride chunk' else out_ld
    for r, i in enumerate(idx):
        for j in range(pieces):
            o = (r * pieces + j) * ld
            flat[o:o + chunk] = src[i, j * chunk:(j + 1) * chunk]
    return dict(out=flat.reshape(len(idx) * pieces, out_ld))


def ref_gather_rows(src, idx, chunk, out_ld, **_):
    return dict(out=(f32_gather_rows(src, idx, chunk, out_ld)['out'], None, None))


REF = dict(label_fwd=ref_label_fwd, label_bwd=ref_label_bwd, gauss_fwd=ref_gauss_fwd, gauss_bwd=ref_gauss_bwd,
           bernoulli_nll=ref_bernoulli_nll, sum_strided=ref_sum_strided, loss_sums=ref_loss_sums, colsum=ref_colsum,
           axpy=ref_axpy, act_grad=ref_act_grad, scale_temper=ref_scale_temper, sigmoid_temper=ref_sigmoid_temper,
           bernoulli_sample=ref_bernoulli_sample, bernoulli_sample_clamped=ref_bernoulli_sample_clamped,
           take_frame=ref_take_frame, lerp_rows=ref_lerp_rows, dropout_rows=ref_dropout_rows, gather_rows=ref_gather_rows)
F32 = dict(label_fwd=f32_label_fwd, label_bwd=f32_label_bwd, gauss_fwd=f32_gauss_fwd, gauss_bwd=f32_gauss_bwd,
           bernoulli_nll=f32_bernoulli_nll, sum_strided=f32_sum_strided, loss_sums=f32_loss_sums, colsum=f32_colsum,
           axpy=f32_axpy, act_grad=f32_act_grad, scale_temper=f32_scale_temper, sigmoid_temper=f32_sigmoid_temper,
           bernoulli_sample=f32_bernoulli_sample, bernoulli_sample_clamped=f32_bernoulli_sample_clamped,
           take_frame=f32_take_frame, lerp_rows=f32_lerp_rows, dropout_rows=f32_dropout_rows, gather_rows=f32_gather_rows)
REDUCTIONS = ('sum_strided', 'loss_sums', 'colsum')           # called twice by the GPU tests: bitwise equal results

# the planted faults of the fp32 evaluation, by kernel
FAULTS = dict(
    bernoulli_nll=('symmetric clip', 'gradient outside the clip'),
    label_bwd=('dlogvar without its half',),
    label_fwd=('kl_w without the prior', 'last-index argmax'),
    gauss_fwd=('32 lanes', 'lane L-1 only'),
    colsum=('small: rows 16..31 dropped', 'two-stage: ragged last chunk dropped', 'beta ignored'),
    loss_sums=('tail dropped', 'divided by 4 (n / 4)', 'strided term read contiguously'),
    sum_strided=('elements from 1024 on ignored',),
    dropout_rows=('mask >', 'mask row r'),
    bernoulli_sample_clamped=('step c - S + 1', 'byte 2 clamps'),
    take_frame=('zeros outside the range',),
    lerp_rows=('a + al (b - a)', 'b dropped inside (0, 1)'),
    gather_rows=('piece stride chunk',))


# -------------------------------------------------------------------------------------------------------- case tables --
# A case is a dict of small parameters; inputs(kernel, case) builds its arrays (fp32-representable float64 or integer
# arrays) from the case's own seed.  Layout parameters (pad_*, ld*, misaligned) only concern the GPU harness.
BCE_POINTS = (15.9, 15.94, 15.95, 16.0, 16.1, 16.2, 30.0, -15.95, -16.0, -16.1, -16.12, -16.2, -30.0, 0.0, 3.0, -3.0)
ELEMENTWISE_N = (1, 255, 256, 257, 1000)


def _label_cases():
    c = [dict(B=1, C=2, prior=0.0, pad_in=0, pad_out=0),
         dict(B=63, C=3, prior=0.3, pad_in=3, pad_out=0),
         dict(B=64, C=10, prior=-1.0, pad_in=0, pad_out=5),
         dict(B=65, C=32, prior=0.3, pad_in=2, pad_out=2),
         dict(B=130, C=10, prior=0.0, pad_in=0, pad_out=0, onehot=False),
         dict(B=130, C=3, prior=-1.0, pad_in=1, pad_out=0, rowloss=False),
         dict(B=65, C=2, prior=0.3, pad_in=0, pad_out=3),
         dict(B=130, C=32, prior=-1.0, pad_in=0, pad_out=0),
         dict(B=37, C=10, prior=0.3, pad_in=0, pad_out=0),                 # test_gpu_ops.test_label_gauss_bernoulli's shape
         dict(B=6, C=10, prior=0.3, pad_in=0, pad_out=1, hand=True),
         dict(B=6, C=3, prior=0.0, pad_in=2, pad_out=0, hand=True)]
    return [dict(dict(onehot=True, rowloss=True, hand=False, seed=100 + i), **x) for i, x in enumerate(c)]


def _gauss_cases():
    out = []
    for i, L in enumerate((1, 2, 3, 5, 8, 12, 17, 32, 33, 64)):          # 12: the 16-lane instantiation
        for k, R in enumerate((1, 7, 257)):
            out.append(dict(L=L, R=R, pad_z=2 * ((i + k) % 2), pad_dz=(0, 3, 1)[(i + k) % 3], rowkl=(i + 2 * k) % 4 != 3,
                            kl_scale=0.25 * ((i + k + 1) % 2), seed=200 + 3 * i + k))
    out.append(dict(L=3, R=101, pad_z=2, pad_dz=0, rowkl=True, kl_scale=0.25, seed=299))     # test_label_gauss_bernoulli's
    return out


def _bernoulli_cases():
    out = []
    for i, D in enumerate((1, 63, 64, 65, 88, 130)):
        for k, R in enumerate((1, 4, 5, 7)):
            j = 4 * i + k
            out.append(dict(D=D, R=R, pad_y=4 * (j % 2), scale=(1.0, 0.5)[(j // 2) % 2], rownll=j % 5 != 3, dlogits=j % 5 != 1,
                            points=False, fractional=j % 3 == 0, seed=300 + j))
    out.append(dict(D=88, R=2, pad_y=0, scale=1.0, rownll=True, dlogits=True, points=True, fractional=False, seed=398))
    out.append(dict(D=88, R=101, pad_y=0, scale=0.5, rownll=True, dlogits=True, points=False, fractional=False, seed=399))
    return out


def _colsum_cases():
    out, j = [], 0
    for M in (1, 15, 16, 17, 32, 33, 47, 1024, 1025, 1217, 2049, 2113):
        for N in (1, 64, 65, 90):
            out.append(dict(M=M, N=N, pad_x=(0, 3)[j % 2], beta=(0.0, 1.0, 0.5)[j % 3], seed=500 + j))
            j += 1
    return out


# loss_sums terms: (kind, n) with kind 'c' contiguous and 16-byte aligned, 's' stride 3, 'm' contiguous, one float off
LOSS_LAUNCHES = ((('c', 1), ('c', 3), ('s', 29), ('c', 4099), ('m', 7201)),
                 (('c', 4), ('c', 5), ('s', 3073), ('c', 12292), ('c', 28695)),
                 (('s', 7200), ('c', 12292), ('s', 29), ('m', 7201), ('c', 5)),
                 (('c', 5000), ('c', 37), ('s', 29), ('s', 29), ('s', 29)))         # test_gpu_ops.test_loss_sums' shapes


def _dropout_cases():
    out, j = [], 0
    for T in (1, 3):
        for rate in (0.0, 0.25, 0.5):
            for beta in (0.0, 1.0):
                out.append(dict(R=12, T=T, n=37, rate=rate, beta=beta, pads=(0, 0, 0) if j % 3 == 0 else (1, 2, 3), seed=700 + j))
                j += 1
    return out


CASES = dict(
    label=_label_cases(),
    gauss=_gauss_cases(),
    bernoulli_nll=_bernoulli_cases(),
    sum_strided=[dict(n=n, stride=st, scale=(1.0 / n, 0.37)[i % 2], seed=400 + 2 * i + st)
                 for i, n in enumerate((1, 63, 1024, 1025, 5000, 3000)) for st in (1, 3)],
    loss_sums=[dict(terms=t, seed=450 + i) for i, t in enumerate(LOSS_LAUNCHES)],
    colsum=_colsum_cases(),
    axpy=[dict(n=n, alpha=(0.37, -1.5)[i % 2], seed=600 + i) for i, n in enumerate(ELEMENTWISE_N)],
    act_grad=[dict(n=n, act=act, seed=610 + 3 * i + act) for i, n in enumerate(ELEMENTWISE_N) for act in (0, 1, 2)],
    scale_temper=[dict(n=n, alpha=(0.0, 0.7, 1.3)[i % 3], seed=630 + i) for i, n in enumerate(ELEMENTWISE_N + (88,))],
    sigmoid_temper=[dict(n=n, alpha=(0.5, 4.0)[i % 2], seed=640 + i) for i, n in enumerate(ELEMENTWISE_N)],
    bernoulli_sample=[dict(n=n, seed=650 + i) for i, n in enumerate(ELEMENTWISE_N)],
    dropout_rows=_dropout_cases(),
    bernoulli_sample_clamped=[dict(R=5, D=D, nsteps=3, S=2, counter=c, seed=720 + 10 * i + c)
                              for i, D in enumerate((3, 88)) for c in (1, 2, 4, 5)],
    take_frame=[dict(R=5, T=4, D=D, step=s, seed=750 + 10 * i + s + 1) for i, D in enumerate((3, 88)) for s in (-1, 0, 3, 4)],
    lerp_rows=[dict(n=n, seed=770 + i) for i, n in enumerate((1, 88, 257))],
    gather_rows=[dict(rows=7, nsrc=11, row_elems=352, chunk=88, out_ld=96, misaligned=False, perm=False, seed=780),
                 dict(rows=9, nsrc=9, row_elems=135, chunk=45, out_ld=48, misaligned=True, perm=True, seed=781),
                 dict(rows=6, nsrc=4, row_elems=90, chunk=0, out_ld=0, misaligned=False, perm=False, seed=782),
                 dict(rows=5, nsrc=5, row_elems=88, chunk=0, out_ld=0, misaligned=False, perm=True, seed=783),
                 dict(rows=300, nsrc=40, row_elems=176, chunk=88, out_ld=88, misaligned=False, perm=False, seed=784)])

LABEL_HAND_ROWS = dict(clip_out=0, tie_hit=1, tie_miss=2, near_tie=3)          # rows of a hand-built label case


def label_inputs(c):
    rng = np.random.default_rng(c['seed'])
    B, C = c['B'], c['C']
    C1 = C - 1
    m, lv = r32(rng.standard_normal((B, C1)) * 0.7), r32(rng.standard_normal((B, C1)) * 0.7)
    eps, dw = r32(rng.standard_normal((B, C1))), r32(rng.standard_normal((B, C)))
    cls = rng.integers(0, C, B)
    if c['hand']:
        h = LABEL_HAND_ROWS
        r = h['clip_out']               # the true class 18 below the appended zero: its renormalised probability < 1e-7
        m[r], eps[r], cls[r] = 0.0, 0.0, 0
        m[r, 0] = -18.0
        for r, k in ((h['tie_hit'], 0), (h['tie_miss'], C - 1)):          # mean = eps = 0: every w equal, exactly
            m[r], eps[r], cls[r] = 0.0, 0.0, k
        r = h['near_tie']               # the largest logit 2^-23 above the appended zero's: w[0] - w[C-1] = 1.2e-7 w[0]
        m[r], eps[r], cls[r] = -1.0, 0.0, C - 1
        m[r, 0] = 2.0 ** -23
    onehot = np.eye(C)[cls] if c['onehot'] else None
    d = dict(mean=m, logvar=lv, eps=eps, onehot=onehot, prior=c['prior'], rowloss=c['rowloss'], dw=dw, class_weight=0.7,
             w_kl_weight=0.9, inv_b=float(f32(1.0 / B)))
    d['w'] = r32(O.logistic_normal(m, lv, eps))          # label_bwd's input: what an exact forward leaves, rounded
    return d


def gauss_inputs(c):
    rng = np.random.default_rng(c['seed'])
    R, L = c['R'], c['L']
    return dict(zargs=r32(rng.standard_normal((R, 2 * L))), eps=r32(rng.standard_normal((R, L))),
                dz=r32(rng.standard_normal((R, L))), kl_scale=c['kl_scale'], rowkl=c['rowkl'])


def bernoulli_inputs(c):
    rng = np.random.default_rng(c['seed'])
    R, D = c['R'], c['D']
    a = r32(rng.standard_normal((R, D)) * 6)
    y = r32(rng.random((R, D))) if c['fractional'] else (rng.random((R, D)) < 0.2).astype(f64)
    if c['points']:
        a[:] = 0.0
        a[:, :len(BCE_POINTS)] = r32(BCE_POINTS)
        y[0], y[1] = 0.0, 1.0
    return dict(logits=a, y=y, scale=c['scale'], rownll=c['rownll'], dlogits=c['dlogits'])


def loss_terms(c):
    """five (flat array, n, stride); the flat array of a strided term holds n * 3 floats of which every third counts, NaN between"""
    rng = np.random.default_rng(c['seed'])
    terms = []
    for kind, n in c['terms']:
        st = 3 if kind == 's' else 1
        x = r32(rng.standard_normal(n * st) + 0.25)
        x[np.arange(n * st) % st != 0] = np.nan
        terms.append((x, n, st))
    return dict(terms=terms)


def elementwise_inputs(kernel, c):
    rng = np.random.default_rng(c['seed'])
    n = c['n']
    if kernel == 'axpy':
        return dict(alpha=c['alpha'], x=r32(rng.standard_normal(n)), y=r32(rng.standard_normal(n)))
    if kernel == 'act_grad':
        y = r32(rng.standard_normal(n) * 0.5 + 0.5)
        sp = np.array([0.0, -0.0, 1.0])[:min(n, 3)]
        y[:sp.size] = sp
        if n == 1:
            y[0] = (0.0, -0.0, 1.0)[c['act']]
        return dict(act=c['act'], y=y, dy=r32(rng.standard_normal(n)))
    if kernel == 'scale_temper':
        return dict(alpha=c['alpha'], x=r32(rng.standard_normal(n)))
    if kernel == 'sigmoid_temper':
        return dict(alpha=c['alpha'], x=r32(rng.standard_normal(n) * 10))
    assert kernel == 'bernoulli_sample'
    p, u = r32(rng.random(n)), r32(rng.random(n))
    u[::3] = p[::3]
    return dict(p=p, u=u)


def dropout_inputs(c):
    rng = np.random.default_rng(c['seed'])
    R, T, n = c['R'], c['T'], c['n']
    X = r32(rng.standard_normal((R, n)) + 3.0)                   # no zeros: a wrong mask decision always shows
    Um = r32(rng.random((R // T, n)))
    rate = f32(c['rate'])
    Um[:, 0] = rate
    Um[:, 5] = rate
    if c['rate'] > 0:
        Um[:, 1] = np.nextafter(rate, f32(0))
        Um[:, 2] = np.nextafter(rate, f32(1))
    return dict(X=X, Um=Um, T=T, rate=c['rate'], beta=c['beta'], out0=r32(rng.standard_normal((R, n))))


def clamped_inputs(c):
    rng = np.random.default_rng(c['seed'])
    R, D = c['R'], c['D']
    p, u = r32(rng.random((R, D))), r32(rng.random((R, D)))
    clamp = np.array([0, 1, 2, 255], np.uint8)[rng.integers(0, 4, (R, c['nsteps'], D))]
    return dict(p=p, u=u, clamp=clamp, counter=c['counter'], S=c['S'])


def take_frame_inputs(c):
    rng = np.random.default_rng(c['seed'])
    return dict(src=r32(rng.standard_normal((c['R'], c['T'], c['D']))), step=c['step'],
                out0=r32(rng.standard_normal((c['R'], c['D']))))


def lerp_inputs(c):
    rng = np.random.default_rng(c['seed'])
    n = c['n']
    a = r32(rng.standard_normal((6, n)) * 1e6)                    # rows of very different magnitude: a + (b - a) is not b
    b = r32(rng.standard_normal((7, n)) * 1e-3)
    a[4:], b[5:] = r32(rng.standard_normal((2, n))), r32(rng.standard_normal((2, n)))          # ... and of the same: both products count
    alpha = r32([0.0, 1.0, 0.5, 1.0 / 3, 0.0, 1.0, 0.5, 1.0 / 3, 0.9, 0.5, 1.0 / 3, 0.9, 0.25, 0.0, 1.0])
    return dict(a=a, ia=np.array([0, 1, 2, 3, 3, 3, 0, 2, 1, 4, 5, 4, 5, 4, 5], np.int32), b=b,
                ib=np.array([4, 0, 0, 2, 1, 3, 4, 4, 2, 5, 6, 6, 5, 5, 6], np.int32), alpha=alpha)


def gather_inputs(c):
    rng = np.random.default_rng(c['seed'])
    idx = rng.permutation(c['nsrc'])[:c['rows']] if c['perm'] else rng.integers(0, c['nsrc'], c['rows'])
    return dict(src=r32(rng.standard_normal((c['nsrc'], c['row_elems']))), idx=idx.astype(np.int64), chunk=c['chunk'],
                out_ld=c['out_ld'])


def colsum_inputs(c):
    rng = np.random.default_rng(c['seed'])
    return dict(X=r32(rng.standard_normal((c['M'], c['N'])) + 0.25), beta=c['beta'], out0=r32(rng.standard_normal(c['N'])))


def sum_strided_inputs(c):
    rng = np.random.default_rng(c['seed'])
    x = r32(rng.standard_normal(c['n'] * c['stride']) + 0.25)
    x[np.arange(x.size) % c['stride'] != 0] = np.nan               # NaN between the elements that count
    return dict(x=x, n=c['n'], stride=c['stride'], scale=c['scale'])


def runs(kernels=None):
    """every (kernel, case, inputs) of the tables: the label and gauss cases give a forward and a backward run each"""
    for fam, cases in CASES.items():
        for c in cases:
            if fam == 'label':
                d = label_inputs(c)
                todo = [('label_fwd', d)] + ([('label_bwd', d)] if c['onehot'] else [])
            elif fam == 'gauss':
                d = gauss_inputs(c)
                todo = [('gauss_fwd', d), ('gauss_bwd', d)]
            else:
                d = (bernoulli_inputs(c) if fam == 'bernoulli_nll' else loss_terms(c) if fam == 'loss_sums' else
                     colsum_inputs(c) if fam == 'colsum' else sum_strided_inputs(c) if fam == 'sum_strided' else
                     dropout_inputs(c) if fam == 'dropout_rows' else clamped_inputs(c) if fam == 'bernoulli_sample_clamped' else
                     take_frame_inputs(c) if fam == 'take_frame' else lerp_inputs(c) if fam == 'lerp_rows' else
                     gather_inputs(c) if fam == 'gather_rows' else elementwise_inputs(fam, c))
                todo = [(fam, d)]
            for k, d in todo:
                if kernels is None or k in kernels:
                    yield k, c, d
