"""fp64 numpy reference of particle Gibbs (TEST ORACLE) on top of tests/smc_reference.py: the seed rule of the
sweeps, the two pins, conditional multinomial resampling (uniforms from oracle/philox.py, stream GIBBS_STREAM, one per
GLOBAL row), the backtracking of the retained path, and a driver that runs K sweeps on any frame model.

Layouts follow csrc/smc.hip: G melodies x P particles, global row r = m * P + p; row m * P is the pinned particle."""
import numpy as np

import smc_reference as SR
from oracle import philox as OP

GIBBS_STREAM = 0xFFFFFFFA
SEED_STEP = 0x9E3779B97F4A7C15


def sweep_seed(seed, s):
    """the Philox key of sweep s: (seed + s * 0x9E3779B97F4A7C15) mod 2^64"""
    return (int(seed) + int(s) * SEED_STEP) % 2 ** 64


def gibbs_uniforms(seed, step, m0, G, P):
    """[G, P]: the uniform of every row of melodies m0 .. m0+G-1 at chain step `step` (index = global row)"""
    return OP.uniform(G * P, seed, step=step, stream_id=GIBBS_STREAM, first_index=m0 * P).astype(np.float64).reshape(G, P)


def conditional_multinomial(logW, u):
    """ancestors of one melody from its normalized log weights logW [P] and the rows' uniforms u [P]: particle 0 keeps
    itself; particle p >= 1 takes the first q with C_q > u_p (C the cumulative weights), the last one if none.  Returns
    (indices, C)."""
    C = np.cumsum(np.exp(np.asarray(logW, np.float64)))
    idx = np.minimum(np.searchsorted(C, np.asarray(u, np.float64), side='right'), len(C) - 1)
    idx[0] = 0
    return idx, C


class ConditionalFilter(SR.Filter):
    """SR.Filter whose resampling is the conditional one, like clv_smc_resample_conditional: the weights, log Z, ESS and the
    rule ess < tau * P are the filter's."""

    def step(self, ell, step, k):
        """SR.Filter.step with the conditional draw, all melodies at once (SR.reweight and conditional_multinomial along
        axis 1)"""
        G, P = self.G, self.P
        lw = self.logW + np.asarray(ell, np.float64).reshape(G, P)
        M = lw.max(axis=1, keepdims=True)
        a = np.exp(lw - M)
        s1, s2 = a.sum(axis=1), (a * a).sum(axis=1)
        lse = M[:, 0] + np.log(s1)
        w, e = lw - lse[:, None], s1 * s1 / s2
        self.logZ += lse
        self.ess[:, k] = e
        res = e < self.tau * P
        u = gibbs_uniforms(self.seed, step, self.m0, G, P)
        C = np.cumsum(np.exp(w), axis=1)
        idx = np.minimum((C[:, None, :] <= u[:, :, None]).sum(axis=-1), P - 1)       # the first q with C_q > u_p
        idx[:, 0] = 0
        near = np.abs(C[:, None, :] - u[:, :, None]).min(axis=-1) < 1e-9
        near[:, 0] = False
        own = np.tile(np.arange(P), (G, 1))
        base = (np.arange(G) * P)[:, None]
        self.anc[k] = (base + np.where(res[:, None], idx, own)).reshape(-1)
        self.near[k] = (near & res[:, None]).reshape(-1)
        self.logW = np.where(res[:, None], -np.log(float(P)), w)
        self.nres += res
        self.resampled[k] = res
        return self.anc[k]


def pin_z(z, z_ref, step, P):
    """z [R, L] with rows m * P replaced by z_ref[m, step] (z_ref [G, T, L]); any other step: unchanged"""
    z = np.array(z)
    if 0 <= step < z_ref.shape[1]:
        z[::P] = z_ref[:, step]
    return z


def pin_frame(x, hist, x_ref, bridge, step, S, P):
    """(x [R, D], hist [nsteps, R, D]) after the frame pin of chain step `step`: at k = step - S in [0, nsteps) rows m * P
    of x and of hist[k] become x_ref[m, k]; at step S - 1 (S > 0, bridge given) rows m * P of x become bridge[m]"""
    x, hist = np.array(x), np.array(hist)
    k = step - S
    if 0 <= k < x_ref.shape[1]:
        x[::P] = x_ref[:, k]
        hist[k, ::P] = x_ref[:, k]
    elif k == -1 and S > 0 and bridge is not None:
        x[::P] = bridge
    return x, hist


def backtrack_path(picks, anc, hist, zhist, bridge_rows, P, S):
    """The lineage of particle picks [G] walked back through anc [nsteps, R] as the next retained path: x_ref [G, nsteps, D]
    uint8 = hist[k, r_k], z_ref [G, S + nsteps, L] = zhist[S + k, r_k] (the seed steps from the root r_0), b_ref [G, D] =
    bridge_rows[r_0] (None without), renewed [G, nsteps] = r_k != m * P."""
    nsteps, R, D = hist.shape
    G = R // P
    T, L = zhist.shape[0], zhist.shape[2]
    x_ref, z_ref = np.zeros((G, nsteps, D), np.uint8), np.zeros((G, T, L), zhist.dtype)
    renewed = np.zeros((G, nsteps), bool)
    first = np.arange(G) * P
    r = first + np.asarray(picks, np.int64)
    for k in range(nsteps - 1, -1, -1):
        r = np.asarray(anc[k], np.int64)[r]
        x_ref[:, k] = hist[k, r]
        z_ref[:, S + k] = zhist[S + k, r]
        renewed[:, k] = r != first
    for t in range(S):
        z_ref[:, t] = zhist[t, r]
    b_ref = None if bridge_rows is None else np.array(bridge_rows[r])
    return x_ref, z_ref, b_ref, renewed


def final_picks(logW, seed, step, m0=0):
    """the particle SR.backtrack(n_out=1) draws per melody from the final normalized logW [G, P], all melodies at once"""
    G, P = logW.shape
    C = np.cumsum(np.exp(np.asarray(logW, np.float64)), axis=1)
    u = SR.smc_uniforms(seed, step, m0, G)
    return np.minimum((C <= u[:, None]).sum(axis=1), P - 1)


def run_sweeps(xhat_of, x0, roll, G, P, K, tau, seed, rng):
    """K sweeps of particle Gibbs on a model without latents or seed steps whose frame probabilities are xhat_of(previous
    frames [R, D]) -> [R, D] float32, from the frame x0 [D], under roll [nsteps, D] (the same for every melody).  The frame
    uniforms come from rng, the resampling uniforms from Philox under sweep_seed(seed, s).  Returns (paths [K, G, nsteps, D]
    uint8, logZ [K, G], renewed [K, G, nsteps], filters: the K Filter objects)."""
    nsteps, D = roll.shape
    R = G * P
    rows = np.repeat(roll[None], R, axis=0)
    paths, logZ, renewed, filters = [], [], [], []
    x_ref = None
    zhist = np.zeros((nsteps, R, 0))
    for s in range(K):
        key = sweep_seed(seed, s)
        filt = (ConditionalFilter if s else SR.Filter)(G, P, nsteps, tau, key)
        hist = np.zeros((nsteps, R, D), np.uint8)
        prev = np.tile(np.asarray(x0, np.float64), (R, 1))
        for k in range(nsteps):
            xhat = xhat_of(prev)
            u = rng.random((R, D)).astype(np.float32)
            x = SR.sample_frame(xhat, u, rows[:, k])
            ell = SR.increment(xhat, rows[:, k])
            hist[k] = x
            if s:
                x, hist = pin_frame(x, hist, x_ref, None, k, 0, P)
            a = filt.step(ell, k, k)
            prev = x[a]
        x_ref, _, _, ren = backtrack_path(final_picks(filt.logW, key, nsteps), filt.anc, hist, zhist, None, P, 0)
        paths.append(x_ref)
        logZ.append(filt.logZ.copy())
        renewed.append(ren if s else np.ones_like(ren))
        filters.append(filt)
    return np.stack(paths), np.stack(logZ), np.stack(renewed), filters
