"""fp64 numpy reference of the particle filter of DESIGN.md 11 (TEST ORACLE): the frame's weight increment, the per-melody
reweighting, ESS and systematic resampling (uniforms from oracle/philox.py, stream SMC_STREAM), lineage and backtrack.

Layouts follow csrc/smc.hip: G melodies x P particles, global row r = m * P + p; ancestors anc [nsteps, R] hold rows;
the uint8 frame history hist [nsteps, R, D] is stored before each step's resampling."""
import numpy as np

from oracle import philox as OP

SMC_STREAM = 0xFFFFFFFD
CLIP_LO = np.float32(1e-7)
CLIP_HI = np.float32(1.0) - np.float32(1e-7)       # float32(1 - 1e-7) = 1 - 2^-23, as the Keras float32 BCE clips


def smc_uniforms(seed, step, m0, G):
    """the resampling uniforms of melodies m0 .. m0+G-1 at generation step `step` (float64 of the float32 draw)"""
    return OP.uniform(G, seed, step=step, stream_id=SMC_STREAM, first_index=m0).astype(np.float64)


def sample_frame(xhat, u, roll_rows):
    """x = [u <= x_hat] (float32 comparison), then bytes 0 / 1 of roll_rows [R, D] force the note"""
    x = (np.asarray(u, np.float32) <= np.asarray(xhat, np.float32)).astype(np.float64)
    c = np.asarray(roll_rows)
    return np.where(c <= 1, c.astype(np.float64), x)


def increment(xhat, roll_rows):
    """l_r = sum over the clamped notes of log q: q = clip(x_hat) (float32) forced on, 1 - clip(x_hat) forced off"""
    q = np.clip(np.asarray(xhat, np.float32), CLIP_LO, CLIP_HI).astype(np.float64)
    c = np.asarray(roll_rows)
    return (np.where(c == 1, np.log(q), 0.0) + np.where(c == 0, np.log(1.0 - q), 0.0)).sum(axis=-1)


def reweight(logW, ell):
    """one frame of one melody: (normalized logW', logsumexp increment of log Z, ESS) in fp64"""
    lw = np.asarray(logW, np.float64) + np.asarray(ell, np.float64)
    M = lw.max()
    a = np.exp(lw - M)
    s1, s2 = a.sum(), (a * a).sum()
    lse = M + np.log(s1)
    return lw - lse, lse, s1 * s1 / s2


def systematic(logW, n, u0):
    """n systematic draws from the normalized log weights logW: draw i takes the first p with n * C_p > u0 + i (C the
    cumulative weights; the last particle if none).  Returns (indices, n * C) -- the latter for near-tie checks."""
    C = np.cumsum(np.exp(np.asarray(logW, np.float64)))
    grid = n * C
    idx = np.searchsorted(grid, u0 + np.arange(n, dtype=np.float64), side='right')
    return np.minimum(idx, len(C) - 1), grid


class Filter:
    """The filter's state over G melodies; step(ell, step, k) applies one frame's update like clv_smc_resample."""

    def __init__(self, G, P, nsteps, tau, seed, m0=0):
        self.G, self.P, self.nsteps, self.tau, self.seed, self.m0 = G, P, nsteps, float(tau), seed, m0
        self.logW = np.full((G, P), -np.log(float(P)))
        self.logZ = np.zeros(G)
        self.ess = np.zeros((G, nsteps))
        self.nres = np.zeros(G, np.int64)
        self.anc = np.zeros((nsteps, G * P), np.int64)
        self.near = np.zeros((nsteps, G * P), bool)      # ancestor decided by a cumulative weight within 1e-9 of the grid
        self.resampled = np.zeros((nsteps, G), bool)

    def step(self, ell, step, k):
        ell = np.asarray(ell, np.float64).reshape(self.G, self.P)
        u = smc_uniforms(self.seed, step, self.m0, self.G)
        P = self.P
        for m in range(self.G):
            w, lse, e = reweight(self.logW[m], ell[m])
            self.logZ[m] += lse
            self.ess[m, k] = e
            rows = m * P + np.arange(P)
            if e < self.tau * P:
                idx, grid = systematic(w, P, u[m])
                self.anc[k, rows] = m * P + idx
                pts = u[m] + np.arange(P)
                self.near[k, rows] = np.abs(grid[None, :] - pts[:, None]).min(axis=1) < 1e-9 * P
                self.logW[m] = -np.log(float(P))
                self.nres[m] += 1
                self.resampled[k, m] = True
            else:
                self.anc[k, rows] = rows
                self.logW[m] = w
        return self.anc[k]


def backtrack(logW, anc, hist, n_out, seed, step, m0=0):
    """n_out systematic draws per melody from the final normalized logW [G, P] (uniform at `step`, index m0 + m), each
    walked back through anc [nsteps, R]: frames [G, n_out, nsteps, D] (float64) and the drawn particles [G, n_out]"""
    G, P = logW.shape
    nsteps, R, D = hist.shape
    u = smc_uniforms(seed, step, m0, G)
    out = np.zeros((G, n_out, nsteps, D))
    picks = np.zeros((G, n_out), np.int64)
    for m in range(G):
        idx, _ = systematic(logW[m], n_out, u[m])
        picks[m] = idx
        for o, p in enumerate(idx):
            r = m * P + p
            for k in range(nsteps - 1, -1, -1):
                r = anc[k, r]
                out[m, o, k] = hist[k, r]
    return out, picks
