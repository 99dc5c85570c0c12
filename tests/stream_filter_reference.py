"""numpy reference of a filter stream's bookkeeping (TEST ORACLE): which pending frames are final after a
chunk (commit), the forced pick of a collapse, and a driver that keeps the pending steps of G melodies as plain lists.

Per melody the pending steps are anc [T, P] (LOCAL particle indices: anc[j, p] = the particle that row p descends from at
step j, oldest step first) and hist [T, P, D] (every particle's frame before step j's resampling), as csrc/smc.hip's anc
and hist hold them for global rows."""
import numpy as np

import filter_reference as FR
import smc_reference as SR
from oracle import philox as OP

COLLAPSE_STREAM = 0xFFFFFFF8
CHUNKINGS = ((12,), (1,) * 12, (5, 4, 3), (7, 5))
PARTICLES = (1, 2, 5, 64)
G, STEPS = 3, 12


def lineages(pending_anc):
    """a [T, P]: a[j, p] = the particle lineage p passes through at pending step j (a_{T-1} = anc_{T-1}, a_j =
    anc_j[a_{j+1}])"""
    anc = np.asarray(pending_anc, np.int64)
    T, P = anc.shape
    a, cur = np.zeros((T, P), np.int64), np.arange(P)
    for j in range(T - 1, -1, -1):
        cur = anc[j][cur]
        a[j] = cur
    return a


def commit(pending_anc, pending_hist):
    """One melody.  Step j is coalesced when all P lineages pass through one particle at it; coalesced steps form a prefix.
    Returns (ncommit, the prefix's frames [ncommit, D], rest = (anc [T - ncommit, P], hist [T - ncommit, P, D]))."""
    anc, hist = np.asarray(pending_anc, np.int64), np.asarray(pending_hist)
    T = anc.shape[0]
    a = lineages(anc)
    one = (a == a[:, :1]).all(axis=1)
    ncommit = T if one.all() else int(np.argmin(one))
    assert one[:ncommit].all() and not one[ncommit:].any(), "coalesced steps form a prefix"
    frames = np.stack([hist[j, a[j, 0]] for j in range(ncommit)]) if ncommit else np.zeros((0,) + hist.shape[2:], hist.dtype)
    return ncommit, frames, (anc[ncommit:], hist[ncommit:])


def lineage_frames(pending_anc, pending_hist, p):
    """the frames [T, D] of the pending steps along the lineage of current particle p"""
    a = lineages(pending_anc)
    hist = np.asarray(pending_hist)
    return np.stack([hist[j, a[j, p]] for j in range(a.shape[0])]) if a.shape[0] else np.zeros((0,) + hist.shape[2:], hist.dtype)


def collapse_pick(logW, seed, t, m0):
    """the particle a collapse draws from one melody's normalized log weights logW [P]: systematic_pick with n = 1 and the
    Philox uniform of COLLAPSE_STREAM at step t, index m0 (the GLOBAL melody)"""
    u0 = OP.uniform(1, seed, step=t, stream_id=COLLAPSE_STREAM, first_index=m0).astype(np.float64)[0]
    return int(SR.systematic(np.asarray(logW, np.float64), 1, u0)[0][0])


def table(P, D=5, start=0):
    """STEPS steps of ancestors [STEPS, G * P] (global rows; filter_reference.ancestor_maps: per melody a cycle, fixed
    points, everything onto one particle and a random many-to-one map in turn, shifted by one per step) and frames
    [STEPS, G * P, D] uint8"""
    rng = np.random.default_rng(1000 * P + D + start)
    anc = np.stack([FR.ancestor_maps(rng, G, P, start=start + k) for k in range(STEPS)])
    hist = (rng.random((STEPS, G * P, D)) < 0.4).astype(np.uint8)
    return anc, hist


class Pending:
    """the pending steps of G melodies as lists; feed() appends a chunk (global rows) and commits"""

    def __init__(self, G, P, D):
        self.G, self.P, self.D = G, P, D
        self.anc = [np.zeros((0, P), np.int64) for _ in range(G)]
        self.hist = [np.zeros((0, P, D), np.uint8) for _ in range(G)]

    def feed(self, anc, hist):
        """anc [n, G * P] global rows, hist [n, G * P, D] -> (counts [G], the committed frames per melody)"""
        P = self.P
        counts, frames = np.zeros(self.G, np.int64), []
        for m in range(self.G):
            rows = slice(m * P, (m + 1) * P)
            a = np.concatenate([self.anc[m], np.asarray(anc, np.int64)[:, rows] - m * P])
            h = np.concatenate([self.hist[m], np.asarray(hist)[:, rows]])
            counts[m], f, (self.anc[m], self.hist[m]) = commit(a, h)
            frames.append(f)
        return counts, frames

    def pending(self):
        return np.array([a.shape[0] for a in self.anc], np.int64)

    def take(self, m, p):
        """melody m collapses onto (or finishes on) particle p: its pending lineage, and nothing pending"""
        f = lineage_frames(self.anc[m], self.hist[m], p)
        self.anc[m], self.hist[m] = np.zeros((0, self.P), np.int64), np.zeros((0, self.P, self.D), np.uint8)
        return f


def schedule(anc, P, chunks):
    """the counts [len(chunks), G] a stream emits after each chunk of the one-call ancestor table anc [nsteps, G * P]"""
    Gm = anc.shape[1] // P
    pend = Pending(Gm, P, 1)
    out, k = [], 0
    for n in chunks:
        out.append(pend.feed(anc[k:k + n], np.zeros((n, Gm * P, 1), np.uint8))[0])
        k += n
    return np.stack(out)
