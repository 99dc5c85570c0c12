"""fp64 reference of the fp32 GEMM family (include/clvae.h: clv_gemm_f32, clv_gemm_grouped_tn, clv_gemm_grouped_tn_small2,
clv_gemm_bce_f32; the deferred reduction of clv_splitk_reduce_multi computes what the immediate one does).

Written from the header's contract, not from the kernels' structure:

  gemm      C = act(alpha * op(A) . op(B) + bias + beta * C0); act none / relu / sigmoid / maskpos (aux > 0 keeps).
  grouped   C_p = beta * C0_p + A_p'^T . B, where row k of A_p' is row k - a_shift of A_p, zero when
            k % a_zero_period == 0; ones == 1: A_p' is one row of ones; ones == 2: the last row of C_p is the column sums
            of B (A_p' = [A_p | 1]).  small2 is two such sets with beta = 0.
  bce       a = A . B + bias; logits = a; l = clip(a, CLIP_LO, CLIP_HI) (the fp32 clip constants of the kernels);
            rownll = sum_j softplus(l) - l y; dlogits = scale (sigmoid(l) - y) [CLIP_LO <= a <= CLIP_HI].
  bounds    beside every output, the rounding budget of an fp32 evaluation of the same contract:
                BOUND_K * 2^-24 * (|alpha| sum_k |a_k b_k| + |bias| + |beta C0|)
            carried through the act (relu is 1-Lipschitz: either side of 0 is accepted by the same bound; sigmoid: a
            quarter of it plus the sigmoid's own rounding; maskpos: the exact mask from aux).  bce carries the logits'
            bound through the NLL (|d/da| <= 1) and its gradient (|d/da| <= 1/4), plus the rounding of expf / logf.
  flags     relu_edge: fp64 pre-activation within its bound of 0; clip_edge (bce): a within its bound of a clip point --
            there dlogits may be either the inside value or 0.
  exact     int_operands: small integers (|x| <= 4) with alpha = 0.75, beta = 0.5: every product and partial sum is exact
            in fp32 up to K = 32768 in any order, so for acts none / relu / maskpos every path must match bit for bit.
            fma_chain: the fp32 accumulator of an fmaf chain in k order (v_mfma_f32_16x16x4_f32 is bitwise such a chain),
            emulated exactly in numpy (this Python has no math.fma).
"""
import numpy as np

from oracle import clvae_oracle as O

U = 2.0 ** -24
BOUND_K = 32        # fp32 unit roundoffs per |term|, as in tests/label_reference.py (worst ratios: tests/test_gpu_gemm.py -s)
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_MASKPOS = 0, 1, 2, 3
# the kernels' clip constants are the fp32 roundings of the oracle's (csrc/common.h: BCE_CLIP_LO / BCE_CLIP_HI)
CLIP_LO = float(np.float32(O.LOGIT_CLIP_LO))
CLIP_HI = float(np.float32(O.LOGIT_CLIP_HI))
INT_ALPHA, INT_BETA = 0.75, 0.5


def _b(mag):
    return BOUND_K * U * mag


def sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def gemm(opA, opB, alpha=1.0, bias=None, beta=0.0, C0=None, act=ACT_NONE, aux=None):
    """opA [M,K], opB [K,N] (the logical operands, fp32 values in fp64); bias [N]; C0 / aux [M,N].
    Returns dict(out, pre, bound, relu_edge)."""
    A = np.asarray(opA, np.float64)
    B = np.asarray(opB, np.float64)
    M, N = A.shape[0], B.shape[1]
    pre = alpha * (A @ B)
    mag = abs(alpha) * (np.abs(A) @ np.abs(B))
    if bias is not None:
        pre = pre + np.asarray(bias, np.float64)[None, :]
        mag = mag + np.abs(bias)[None, :]
    if beta != 0.0:
        pre = pre + beta * np.asarray(C0, np.float64)
        mag = mag + np.abs(beta * np.asarray(C0, np.float64))
    bnd = _b(mag) + np.zeros((M, N))
    edge = np.zeros((M, N), bool)
    if act == ACT_RELU:
        out = np.maximum(pre, 0.0)
        edge = np.abs(pre) <= bnd
    elif act == ACT_SIGMOID:
        out = sigmoid(pre)
        bnd = 0.25 * bnd + _b(out)
    elif act == ACT_MASKPOS:
        keep = np.asarray(aux) > 0
        out = np.where(keep, pre, 0.0)
        bnd = np.where(keep, bnd, 0.0)
    else:
        out = pre
    return dict(out=out, pre=pre, bound=bnd, relu_edge=edge)


def grouped_operand(A, K, M, shift=0, zero_period=0, ones=0):
    """op(A_p)^T as a dense [K, M] matrix: A is [>= K - shift rows, >= M (ones == 2: M - 1) columns] (row-major, the
    physical layout without its padding columns)."""
    out = np.zeros((K, M))
    if ones == 1:
        out[:, 0] = 1.0
        return out
    ncol = M - 1 if ones == 2 else M
    k = np.arange(K)
    live = np.ones(K, bool) if zero_period <= 0 else (k % zero_period != 0)
    src = k - shift
    if (src[live] < 0).any():
        raise ValueError("row k - a_shift < 0 outside the zero-period rows")
    A = np.asarray(A, np.float64)
    out[live, :ncol] = A[src[live], :ncol]
    if ones == 2:
        out[:, M - 1] = 1.0
    return out


def grouped(probs, B, beta=0.0):
    """probs: list of dict(A, M, shift, zero_period, ones, C0); B [K,N].  Returns one gemm() dict per problem."""
    B = np.asarray(B, np.float64)
    K = B.shape[0]
    res = []
    for p in probs:
        Ap = grouped_operand(p.get('A'), K, p['M'], p.get('shift', 0), p.get('zero_period', 0), p.get('ones', 0))
        res.append(gemm(Ap.T, B, 1.0, None, beta, p.get('C0'), ACT_NONE))
    return res


def bce(A, B, bias, Y, scale):
    """the output head with the fused Bernoulli NLL: dict(logits, rownll, dlogits, b_logits, b_rownll, b_dlogits,
    clip_edge, dl_alt).  dl_alt: the other side's dlogits on clip_edge elements (0 inside, the inside value outside)."""
    g = gemm(A, B, 1.0, bias)
    a, ba = g['out'], g['bound']
    Y = np.asarray(Y, np.float64)
    l = np.clip(a, CLIP_LO, CLIP_HI)
    sp = np.maximum(l, 0.0) + np.log1p(np.exp(-np.abs(l)))
    term = sp - l * Y
    inside = (a >= CLIP_LO) & (a <= CLIP_HI)
    sg = sigmoid(l)
    dl_in = scale * (sg - Y)
    dl = np.where(inside, dl_in, 0.0)
    # the clip is 1-Lipschitz and |softplus' - y| <= 1: the logits' bound passes through; + expf / logf rounding
    # (absolute ~ 2^-24 from 1 + e, relative on the terms)
    b_row = (ba + _b(np.abs(sp) + np.abs(l * Y) + 1.0)).sum(1)
    b_dl = np.abs(scale) * (0.25 * ba + _b(sg + np.abs(Y)))
    edge = (np.abs(a - CLIP_LO) <= ba) | (np.abs(a - CLIP_HI) <= ba)
    dl_alt = np.where(inside, 0.0, dl_in)
    return dict(logits=a, rownll=term.sum(1), dlogits=dl, b_logits=ba, b_rownll=b_row, b_dlogits=b_dl, clip_edge=edge,
                dl_alt=dl_alt)


# ---------------------------------------------------------------- checks --
def ratio(got, ref, bound):
    """worst |got - ref| / bound (0 / 0 = 0); NaN in got -> inf"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    err = np.where(np.isnan(got), np.inf, err)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def within(got, ref, bound, what="", alt=None, alt_mask=None):
    """assert every element within its bound (alt / alt_mask: an other accepted value on flagged elements); returns the
    worst ratio"""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    err = np.where(np.isnan(got), np.inf, err)
    ok = err <= bound
    if alt is not None:
        ok |= alt_mask & (np.abs(got - alt) <= bound)
    if not ok.all():
        i = np.argwhere(~ok)[0]
        t = tuple(int(x) for x in i)
        raise AssertionError("%s: %d elements outside the bound, first %s: got %r ref %r bound %r" %
                             (what, int((~ok).sum()), t, got[t], ref[t], bound[t]))
    return ratio(np.where(ok & (err > bound), ref, got), ref, bound)


def exact(got, ref, what=""):
    """bit for bit (fp32 values compared as fp64: both are exact)"""
    got = np.asarray(got, np.float64)
    bad = ~(got == ref)
    if bad.any():
        i = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError("%s: %d elements differ, first %s: got %r want %r" % (what, int(bad.sum()), i, got[i], ref[i]))


def int_operands(rng, *shape, lim=4):
    """small integers in [-lim, lim] as fp64 (exact in fp32)"""
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64)


# ----------------------------------------------------- exact fp32 fma chain --
def _round_fp32(s, e):
    """fp32 rounding (nearest even) of the exact value s + e, where s = fl64(s + e) and |e| <= ulp64(s) / 2"""
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    d = s - r64
    # s exactly halfway between r and its neighbour on s's side: the exact value lies beyond s by e's sign
    toward = np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)
    nb = np.nextafter(r, toward)
    mid = (d != 0) & (np.abs(nb.astype(np.float64) - s) == np.abs(d))
    go = mid & (((d > 0) & (e > 0)) | ((d < 0) & (e < 0)))
    # e pulling back towards r leaves r the nearest; e == 0 is a true tie, which the cast already rounded to even
    return np.where(go, nb, r)


def fmaf(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise (a, b, c fp32 arrays or scalars, finite, normal range)"""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    p = a * b                                   # exact: 24 + 24 bits
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)               # TwoSum: p + c == s + e exactly
    return _round_fp32(s, e)


def fma_chain(opA, opB):
    """acc = fmaf(a_k, b_k, acc) for k = 0 .. K-1 from acc = 0: [M,K] x [K,N] -> fp32 [M,N]"""
    A = np.asarray(opA, np.float32)
    B = np.asarray(opB, np.float32)
    acc = np.zeros((A.shape[0], B.shape[1]), np.float32)
    for k in range(A.shape[1]):
        acc = fmaf(A[:, k:k + 1], B[k:k + 1, :], acc)
    return acc
