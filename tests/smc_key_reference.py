"""fp64 numpy reference of the key-inferring particle filter of DESIGN.md 12 (TEST ORACLE): the particles' label rows
drawn from a prior over the key, the per-step posterior over the key and the label of each returned path.  Built on
tests/smc_reference.py: the filter itself is unchanged, a particle's row only travels with its state.

Layouts follow csrc/smc.hip: G melodies x P particles, global row r = m * P + p, label rows wr [R, C]."""
import numpy as np

import smc_reference as SR
from oracle import philox as OP

SMC_W_STREAM = 0xFFFFFFFC


def key_uniforms(seed, m0, G):
    """the allocation uniforms of melodies m0 .. m0+G-1 (stream SMC_W_STREAM, step 0, index = global melody)"""
    return OP.uniform(G, seed, step=0, stream_id=SMC_W_STREAM, first_index=m0).astype(np.float64)


def allocate_keys(probs_row, P, u0):
    """systematic draw of P keys from one melody's probs: particle p takes the first class c with P * cum_c > u0 + p
    (cum the inclusive sums in class order; the last class if none).  Returns (keys [P], P * cum)"""
    cum = np.cumsum(np.asarray(probs_row, np.float64))
    grid = P * cum
    idx = np.searchsorted(grid, u0 + np.arange(P, dtype=np.float64), side='right')
    return np.minimum(idx, len(cum) - 1), grid


def init_categorical(probs, P, seed, m0=0):
    """one-hot label rows [G * P, C] (float64) and the keys [G, P] of the categorical prior probs [G, C]"""
    probs = np.asarray(probs, np.float64)
    G, C = probs.shape
    u = key_uniforms(seed, m0, G)
    keys = np.stack([allocate_keys(probs[m], P, u[m])[0] for m in range(G)])
    return np.eye(C)[keys.reshape(-1)], keys


def init_logistic_normal(mean, log_var, P, seed, m0=0):
    """label rows [G * P, C] of the logistic-normal prior mean, log_var [G, C-1]: s = mean + exp(log_var / 2) * eps with
    eps the float32 Philox normals of stream SMC_W_STREAM, step 1, index r * (C-1) + c at the global row r, then
    softmax([s, 0]); everything after the draw in fp64"""
    mean, log_var = np.asarray(mean, np.float64), np.asarray(log_var, np.float64)
    G, C1 = mean.shape
    eps = OP.normal(G * P * C1, seed, step=1, stream_id=SMC_W_STREAM, first_index=m0 * P * C1).astype(np.float64)
    s = np.repeat(mean, P, axis=0) + np.exp(np.repeat(log_var, P, axis=0) / 2) * eps.reshape(G * P, C1)
    s = np.concatenate([s, np.zeros((G * P, 1))], axis=1)
    e = np.exp(s - s.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def w_posterior(logW, wr):
    """sum_p exp(logW[m, p]) * wr[m * P + p, :] for normalized log weights logW [G, P] and rows wr [G * P, C]: [G, C]"""
    G, P = logW.shape
    return np.einsum('mp,mpc->mc', np.exp(np.asarray(logW, np.float64)), np.asarray(wr, np.float64).reshape(G, P, -1))


def posterior_from_increments(ell_sum, wr):
    """identity 2 (no resampling): the softmax-weighted mean of the rows by the accumulated increments ell_sum [G, P]"""
    a = np.asarray(ell_sum, np.float64)
    w = np.exp(a - a.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    G, P = a.shape
    return np.einsum('mp,mpc->mc', w, np.asarray(wr, np.float64).reshape(G, P, -1))


def take_w(wr, picks, P):
    """w_out [G, n_out, C]: the row of the particle picks [G, n_out] each returned path was drawn from"""
    picks = np.asarray(picks)
    rows = np.arange(picks.shape[0])[:, None] * P + picks
    return np.asarray(wr)[rows]


class KeyFilter(SR.Filter):
    """SR.Filter whose particles carry label rows wr [R, C]: step() permutes them by the step's ancestors, like one more
    buffer of clv_smc_gather, and records the posterior over the key from the weights and rows the next step starts from"""

    def __init__(self, G, P, nsteps, tau, seed, wr, m0=0):
        super().__init__(G, P, nsteps, tau, seed, m0)
        self.wr = np.array(wr, np.float64)
        self.w_post = np.zeros((G, nsteps, self.wr.shape[1]))

    def step(self, ell, step, k):
        a = super().step(ell, step, k)
        self.wr = self.wr[a]
        self.w_post[:, k] = w_posterior(self.logW, self.wr)
        return a


def pooled_estimates(logZ, post_last, logZ_scale=0.0):
    """The two unbiased-in-the-numerator summaries of G independent filters: with Z_m = exp(logZ_m -
    logZ_scale) and q_mc = w_posterior[m, last, c],
      joint_c = mean_m Z_m q_mc                (estimates p(constraints, key = c) / exp(logZ_scale) without bias)
      ratio_c = sum_m Z_m q_mc / sum_m Z_m     (estimates p(key = c | constraints); a ratio of two unbiased means)
    with their standard errors: joint_c's from the sample variance, ratio_c's by the delta method,
      var(ratio_c) ~ sum_m (Z_m (q_mc - ratio_c))^2 / (sum_m Z_m)^2.
    Returns (joint [C], se_joint [C], ratio [C], se_ratio [C])."""
    Z = np.exp(np.asarray(logZ, np.float64) - logZ_scale)
    q = np.asarray(post_last, np.float64)
    G = len(Z)
    zq = Z[:, None] * q
    joint = zq.mean(axis=0)
    se_joint = zq.std(axis=0, ddof=1) / np.sqrt(G)
    ratio = zq.sum(axis=0) / Z.sum()
    se_ratio = np.sqrt(((Z[:, None] * (q - ratio[None])) ** 2).sum(axis=0)) / Z.sum()
    return joint, se_joint, ratio, se_ratio
