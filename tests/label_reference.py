"""fp64 reference of the cl_vrnn label head (include/clvae.h: clv_vrnn_label_fwd, clv_vrnn_label_fwd_x with and without a
clv_label_stage, clv_vrnn_label_fwd_parts, the label rows of the front launch, clv_vrnn_label_bwd).

Written from the header's contract, not from the kernels' structure, out of oracle/clvae_oracle.py pieces:

  forward   hW = relu(X . Kh + bh) (or hW given); wargs = hW . Ka + ba; W = O.logistic_normal(mean, log_var, eps);
            rowloss[:, 0] = the kl_w row term of O.kl_w_prior, rowloss[:, 1] = O.cce_keras(W, onehot, C - 1),
            rowloss[:, 2] = hit by O.categorical_accuracy's argmax rule (first index on ties; 0 without onehot);
            rb_enc = W . Kenc_w + benc, rb_dec = W . Kdec_w + bdec -- all in the kernels' layouts.
  bounds    beside every output, the rounding budget of an fp32 evaluation of the same contract: a dot product gets
                BOUND_K * 2^-24 * sum |terms|   (e.g. |X| . |Kh| + |bh| for hW)
            and every output also carries the bounds of its inputs through its first derivative (wargs from hW, W from
            wargs, ...), so that each element is judged against its own budget, not against a tensor's largest entry.
            w_rec also carries 2^-24 (C - 1) per unit of onehot: the fp32 clip constants (1e-7 and 1 - 1e-7 rounded to fp32).
  flags     relu_edge [B,D]: hW entries whose fp64 pre-activation lies within its bound of 0 (dhW is masked by hW > 0);
            tie [B]: rows whose two largest W lie within their bounds of each other but are not equal -- there hit may
            legitimately differ.  An EXACT fp64 tie is not flagged: the first-index rule decides it (the tests build such
            ties from identical fp32 computations, Ka = ba = eps = 0, which are exact in fp32 too).
  assembly  stage_rows / assemble: what a clv_label_stage leaves behind, exactly, from the byte stores, tables, idx, row0 and
            the batch cursor (batch j = (step - step0) mod period, the mathematical modulo).
  backward  pair_reference.label_backward (re-exported here), and pair_reference.assert_close_sliced.
"""
import numpy as np

from oracle import clvae_oracle as O
from pair_reference import assert_close_sliced, label_backward  # noqa: F401  (the label head's tests take them from here)

U = 2.0 ** -24
BOUND_K = 32        # fp32 unit roundoffs per |term|: covers C <= 32 sums, expf / logf, the hW sums of 16 wave partials
                    # (the observed worst error / bound ratios are printed by tests/test_gpu_label_head.py)


def _b(*terms):
    return BOUND_K * U * sum(terms)


def forward(Ka, ba, eps, onehot, prior, Kenc_w, benc, Kdec_w, bdec, hW=None, X=None, Kh=None, bh=None, dtype=np.float64):
    """the label head's forward.  Either hW [B,D] (clv_vrnn_label_fwd) or X [B,nx], Kh [nx,D], bh [D] (the others).
    onehot [B,C] or None.  dtype float32: the same contract evaluated in fp32 (no bounds, no flags)."""
    cast = lambda a: None if a is None else np.asarray(a, np.float64).astype(dtype)
    Ka, ba, eps, onehot, Kenc_w, benc, Kdec_w, bdec, hW, X, Kh, bh = map(
        cast, (Ka, ba, eps, onehot, Kenc_w, benc, Kdec_w, bdec, hW, X, Kh, bh))
    C = Kenc_w.shape[0]
    C1 = C - 1
    r = {}
    if hW is None:
        r['a_hW'] = (X @ Kh + bh).astype(dtype)
        hW = np.maximum(r['a_hW'], 0).astype(dtype)
    r['hW'] = hW
    wargs = (hW @ Ka + ba).astype(dtype)
    m, lv = wargs[:, :C1], wargs[:, C1:]
    W = O.logistic_normal(m, lv, eps).astype(dtype)
    B = W.shape[0]
    rowloss = np.zeros((B, 3), dtype)
    rowloss[:, 0] = O.kl_w_prior(m, lv, prior)[0]
    if onehot is not None:
        rowloss[:, 1] = O.cce_keras(W, onehot, C1)[0]
        rowloss[:, 2] = [O.categorical_accuracy(onehot[b:b + 1], W[b:b + 1]) for b in range(B)]
    r.update(wargs=wargs, W=W, rowloss=rowloss, rb_enc=(W @ Kenc_w + benc).astype(dtype),
             rb_dec=(W @ Kdec_w + bdec).astype(dtype))
    if dtype != np.float64:
        return r
    # ---- bounds ----
    A = np.abs
    if X is not None:
        b_a = _b(A(X) @ A(Kh), A(bh))
        r['relu_edge'] = A(r['a_hW']) <= b_a
    else:
        b_a = np.zeros_like(hW)
        r['relu_edge'] = np.zeros(hW.shape, bool)
    r['b_hW'] = b_a                                       # relu is 1-Lipschitz
    b_wa = b_a @ A(Ka) + _b(A(hW) @ A(Ka), A(ba))
    r['b_wargs'] = b_wa
    bm, blv = b_wa[:, :C1], b_wa[:, C1:]
    sd = np.exp(0.5 * lv)
    b_s = np.concatenate([bm + 0.5 * sd * A(eps) * blv + _b(A(m), sd * A(eps)), np.zeros((B, 1))], 1)
    r['b_W'] = W * (b_s + (W * b_s).sum(1, keepdims=True)) + _b(W)
    b_row = np.zeros((B, 3))
    ep = np.exp(prior)
    b_row[:, 0] = 0.5 * (2 * A(m) / ep * bm + A(1 - sd * sd / ep) * blv).sum(1) + \
        0.5 * _b(A(1 - prior) + A(lv) + sd * sd / ep + m * m / ep).sum(1)
    if onehot is not None:
        q = W + 1e-10
        Q = q.sum(1, keepdims=True)
        n = q / Q
        bn = n * (r['b_W'] / q + r['b_W'].sum(1, keepdims=True) / Q) + _b(n)
        lo = np.maximum(n - bn, O.EPS_K)
        nc = np.clip(n, O.EPS_K, 1 - O.EPS_K)
        b_row[:, 1] = C1 * (A(onehot) * (bn / lo + _b(A(np.log(nc))) + U)).sum(1)
    r['b_rowloss'] = b_row
    r['b_rb_enc'] = r['b_W'] @ A(Kenc_w) + _b(A(W) @ A(Kenc_w), A(benc))
    r['b_rb_dec'] = r['b_W'] @ A(Kdec_w) + _b(A(W) @ A(Kdec_w), A(bdec))
    top = np.sort(W, 1)[:, ::-1]
    it = np.argsort(-W, 1, kind='stable')
    gap = top[:, 0] - top[:, 1]
    bw = np.take_along_axis(r['b_W'], it[:, :2], 1).sum(1)
    r['tie'] = (gap > 0) & (gap <= bw)
    return r


OUTPUTS = ('hW', 'wargs', 'W', 'rb_enc', 'rb_dec')


def bound_ratios(got, ref):
    """worst |got - ref| / bound per output (rowloss: kl_w and w_rec columns); NaN in got gives inf"""
    out = {}
    for k in OUTPUTS:
        e = np.abs(np.asarray(got[k], np.float64) - ref[k])
        out[k] = float(np.nan_to_num(e / np.maximum(ref['b_' + k], 1e-300), nan=np.inf).max())
    e = np.abs(np.asarray(got['rowloss'], np.float64)[:, :2] - ref['rowloss'][:, :2])
    out['rowloss'] = float(np.nan_to_num(e / np.maximum(ref['b_rowloss'][:, :2], 1e-300), nan=np.inf).max())
    return out


def check_forward(got, ref, name='', sliced_rtol=1e-4):
    """every output of got (arrays in the kernels' layouts) against ref: per element within its bound, hit exactly outside the
    flagged near-tie rows, and per slice (batch row, column) with pair_reference.assert_close_sliced.  Returns the bound
    ratios."""
    ratios = bound_ratios(got, ref)
    for k, v in ratios.items():
        assert v <= 1.0, "%s %s: error %.3g x its bound" % (name, k, v)
    hit = np.asarray(got['rowloss'], np.float64)[:, 2]
    keep = ~ref['tie']
    bad = np.flatnonzero(keep & (hit != ref['rowloss'][:, 2]))
    assert bad.size == 0, "%s hit: rows %s" % (name, bad[:8].tolist())
    for k in OUTPUTS:
        a = np.asarray(got[k], np.float64)
        assert_close_sliced(a, ref[k], (0, 1), 1e-6 * max(np.abs(ref[k]).max(), 1e-30), sliced_rtol, name=name + k)
    return ratios


# ---- the mini-batch assembly of a clv_label_stage ----
def stage_rows(B, idx=None, row0=0, cursor=None):
    """source row sr of every batch row b: idx[base + b] (idx None: row0 + base + b), base = j * stride + offset with
    j = (step - step0) mod period for cursor = (step, step0, period, stride, offset) (None: base 0)"""
    base = 0
    if cursor is not None:
        step, step0, period, stride, offset = cursor
        base = ((step - step0) % period) * stride + offset         # Python's % is the mathematical modulo
    b = np.arange(B)
    return np.asarray(idx)[base + b] if idx is not None else row0 + base + b


def _rows(store, stride, offset, table, sr, n):
    r = np.asarray(table)[sr] if table is not None else sr
    return np.stack([store[int(x) * stride + offset:int(x) * stride + offset + n] for x in r])


def assemble(sr, nx, cur, hist=None, hist_chunk=None, hist_ld=None, w_src=None):
    """cur / hist = (flat uint8 store, stride, offset, table or None).  Returns X8 [B,nx] (uint8), X [B,nx] (float),
    Xh8 / Xh: the history rows as bytes [B,nx] and widened in pieces, Xh [B * nx / hist_chunk, hist_ld] with NaN in the
    columns the stage does not write; w_out = w_src[sr]."""
    r = dict(X8=_rows(cur[0], cur[1], cur[2], cur[3], sr, nx))
    r['X'] = r['X8'].astype(np.float64)
    if hist is not None:
        r['Xh8'] = _rows(hist[0], hist[1], hist[2], hist[3], sr, nx)
        if hist_chunk is not None:
            B, pieces = len(sr), nx // hist_chunk
            Xh = np.full((B * pieces, hist_ld), np.nan)
            Xh[:, :hist_chunk] = r['Xh8'].reshape(B * pieces, hist_chunk)
            r['Xh'] = Xh
    if w_src is not None:
        r['w_out'] = np.asarray(w_src, np.float64)[sr]
    return r
