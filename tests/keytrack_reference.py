"""fp64 reference of key tracking (include/clvae.h: clv_key_track_windows, clv_key_track_smooth), written from the header's
contract, not from the kernels.

  windows   windows(piece, T, hop): window j of a piece = its frames [j hop, j hop + T) by plain slicing, flattened, for
            j < max(0, (P - T) // hop + 1).
  head      head(X, Kh, bh, Ka, ba): label_reference.forward on those rows -> wargs and its element-wise bound b_wargs
            (label_reference's BOUND_K budget as it stands).
  logp      K = 0: logp0(wargs, b_wargs) = log softmax([mean, 0]) and the bound
                |d logp_c| <= b_c + sum_i w_i b_i + BOUND_K 2^-24 (|s_c| + |lse| + 1)
            (s = [mean, 0], w = softmax(s), b = b_wargs of the means and 0 for the appended class: d logp_c / d s_i =
            [i == c] - w_i; the last term is the fp32 evaluation of the shift, expf, the sum, logf and the subtraction).
            K >= 1: logpK(wargs, eps) with the DEVICE's wargs (exact inputs, so no input bound) and the eps the device drew:
            per sample label_reference's b_W with b_mean = b_log_var = 0, i.e. b_s = BOUND_K 2^-24 (|m| + sd |eps|) (+ sd times
            the tolerance of the normals themselves),
            b_W = W (b_s + sum W b_s) + BOUND_K 2^-24 W; logp = log mean_k W_k, bound mean_k b_W / mean_k W + BOUND_K 2^-24.
  hmm       smooth(logp, log_prior, log_trans, kappa): log-space forward-backward and Viterbi in numpy, emission
            kappa * logp[j]; path_score: the log score of any path; brute(): all C^J paths enumerated.
"""
import itertools

import numpy as np

import label_reference as L

U, BOUND_K = L.U, L.BOUND_K
KEY_STREAM = 0xFFFFFFFB


def n_windows(P, T, hop):
    return max(0, (P - T) // hop + 1)


def windows(piece, T, hop):
    """-> (X [J, T*D] float64, starts [J])"""
    piece = np.asarray(piece, np.float64)
    J = n_windows(piece.shape[0], T, hop)
    starts = np.arange(J) * hop
    X = np.stack([piece[t:t + T].reshape(-1) for t in starts]) if J else np.zeros((0, T * piece.shape[1]))
    return X, starts


def head(X, Kh, bh, Ka, ba):
    """wargs [J, 2(C-1)] and b_wargs of the rows X through label_reference.forward"""
    C = Ka.shape[1] // 2 + 1
    z = np.zeros((C, 1))
    r = L.forward(Ka, ba, np.zeros((X.shape[0], C - 1)), None, 0.0, z, np.zeros(1), z, np.zeros(1), X=X, Kh=Kh, bh=bh)
    return r['wargs'], r['b_wargs']


def logsumexp(a, axis=-1):
    m = np.max(a, axis=axis, keepdims=True)
    return (m + np.log(np.sum(np.exp(a - m), axis=axis, keepdims=True))).squeeze(axis)


def logp0(wargs, b_wargs):
    """-> (logp [J, C], bound [J, C])"""
    wargs = np.asarray(wargs, np.float64)
    C1 = wargs.shape[1] // 2
    J = wargs.shape[0]
    s = np.concatenate([wargs[:, :C1], np.zeros((J, 1))], 1)
    b = np.concatenate([np.asarray(b_wargs, np.float64)[:, :C1], np.zeros((J, 1))], 1)
    lse = logsumexp(s)[:, None]
    logp = s - lse
    w = np.exp(logp)
    bound = b + (w * b).sum(1, keepdims=True) + BOUND_K * U * (np.abs(s) + np.abs(lse) + 1)
    return logp, bound


def logpK(wargs, eps, eps_tol=0.0):
    """wargs [J, 2(C-1)] (the device's, taken as exact), eps [K, J, C-1] -> (logp [J, C], bound [J, C]); eps_tol: how far
    the eps handed in may be from the ones the kernel used (b_s gains sd * eps_tol)"""
    wargs, eps = np.asarray(wargs, np.float64), np.asarray(eps, np.float64)
    K, J, C1 = eps.shape
    m, lv = wargs[:, :C1], wargs[:, C1:]
    sd = np.exp(0.5 * lv)
    acc, bacc = np.zeros((J, C1 + 1)), np.zeros((J, C1 + 1))
    for k in range(K):
        s = np.concatenate([m + sd * eps[k], np.zeros((J, 1))], 1)
        W = np.exp(s - logsumexp(s)[:, None])
        b_s = np.concatenate([BOUND_K * U * (np.abs(m) + sd * np.abs(eps[k])) + sd * eps_tol, np.zeros((J, 1))], 1)
        acc += W
        bacc += W * (b_s + (W * b_s).sum(1, keepdims=True)) + BOUND_K * U * W
    return np.log(acc / K), (bacc / K) / (acc / K) + BOUND_K * U


def eps_index(piece, t, c):
    """the Philox index of class c of the window that starts at frame t of global piece `piece`"""
    return (((int(piece) << 24) + int(t)) * 32) + int(c)


# ---- the HMM -----------------------------------------------------------------------------------------------------------
def _lp(log_prior, C):
    return np.full(C, -np.log(C)) if log_prior is None else np.asarray(log_prior, np.float64)


def smooth(logp, log_prior, log_trans, kappa):
    """one piece: logp [J, C] -> dict(post [J, C], path [J], log_evidence, piece_post [C], best = the optimal path's score)"""
    logp = np.asarray(logp, np.float64)
    J, C = logp.shape
    lp, lt = _lp(log_prior, C), np.asarray(log_trans, np.float64)
    if J == 0:
        return dict(post=np.zeros((0, C)), path=np.zeros(0, np.int64), log_evidence=0.0, piece_post=np.exp(lp - logsumexp(lp)),
                    best=0.0)
    le = kappa * logp
    fwd = np.zeros((J, C))
    fwd[0] = lp + le[0]
    for j in range(1, J):
        fwd[j] = logsumexp(fwd[j - 1][:, None] + lt, axis=0) + le[j]
    bwd = np.zeros((J, C))
    for j in range(J - 2, -1, -1):
        bwd[j] = logsumexp(lt + (le[j + 1] + bwd[j + 1])[None, :], axis=1)
    ev = logsumexp(fwd[-1])
    post = np.exp(fwd + bwd - ev)
    d = np.zeros((J, C))
    bp = np.zeros((J, C), np.int64)
    d[0] = lp + le[0]
    for j in range(1, J):
        v = d[j - 1][:, None] + lt
        bp[j] = np.argmax(v, axis=0)               # first index on ties
        d[j] = v.max(axis=0) + le[j]
    path = np.zeros(J, np.int64)
    path[-1] = np.argmax(d[-1])
    for j in range(J - 1, 0, -1):
        path[j - 1] = bp[j, path[j]]
    z = lp + kappa * logp.sum(axis=0)
    return dict(post=post, path=path, log_evidence=float(ev), piece_post=np.exp(z - logsumexp(z)), best=float(d[-1].max()))


def path_score(path, logp, log_prior, log_trans, kappa):
    logp = np.asarray(logp, np.float64)
    J, C = logp.shape
    lp, lt = _lp(log_prior, C), np.asarray(log_trans, np.float64)
    path = np.asarray(path, np.int64)
    assert path.shape == (J,) and (path >= 0).all() and (path < C).all()
    s = lp[path[0]] + kappa * logp[0, path[0]]
    for j in range(1, J):
        s += lt[path[j - 1], path[j]] + kappa * logp[j, path[j]]
    return float(s)


def brute(logp, log_prior, log_trans, kappa):
    """all C^J paths: dict(post, log_evidence, best)"""
    logp = np.asarray(logp, np.float64)
    J, C = logp.shape
    paths = list(itertools.product(range(C), repeat=J))
    sc = np.array([path_score(p, logp, log_prior, log_trans, kappa) for p in paths])
    ev = logsumexp(sc)
    w = np.exp(sc - ev)
    post = np.zeros((J, C))
    for p, wi in zip(paths, w):
        for j, c in enumerate(p):
            post[j, c] += wi
    return dict(post=post, log_evidence=float(ev), best=float(sc.max()))


def sticky(C, hop, expected_segment):
    leave = hop / float(expected_segment)
    A = np.full((C, C), leave / (C - 1))
    A[np.diag_indices(C)] = 1 - leave
    return A


def segments_cover(segs, P):
    """whether [(key, first, n), ...] covers frames 0 .. P exactly, in order, without empty segments"""
    at = 0
    for _, f, n in segs:
        if f != at or n < 1:
            return False
        at += n
    return at == P
