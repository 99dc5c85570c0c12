"""fp64 reference of sampling a frame given how many of its notes sound (csrc/voices.hip).

One row and one returned frame: p [D] the float32 probabilities the frame chain forms, u [D] its float32 uniforms, the
frame's roll row (bytes 0 / 1 force a note, any other byte leaves it free) and its pair (lo, hi).
  q_j = clip(p_j, 1e-7, 1 - 1e-7) in float32, widened to double; for the recursion 0 where the roll forces the note off, 1
  where it forces it on.
  table   B[D][c] = [lo <= c <= hi];  B[j][c] = (1 - q_j) B[j+1][c] + q_j B[j+1][c+1],  B[.][hi+1] = 0
  draw    notes ascending, c = 0: a forced note takes its value; a free one a = q_j B[j+1][c+1], b = (1 - q_j) B[j+1][c];
          x_j = 0 if a == 0, 1 if b == 0, else [(double) u_j <= a / B[j][c]]; c += x_j
  weight  ell = (sum over forced notes of log q, smc_reference.increment) + log B[0][0]
The pair (0, 255) leaves the frame free: smc_reference.sample_frame and increment alone."""
import numpy as np

import smc_reference as SR

FREE = 255
FREE_PAIR = (0, 255)
MAX_COUNT = 15


def clipped(p):
    """q: the filter's clip of the float32 probabilities, widened"""
    return np.clip(np.asarray(p, np.float32), SR.CLIP_LO, SR.CLIP_HI).astype(np.float64)


def recursion_q(p, roll_row=None):
    q = clipped(p)
    if roll_row is not None:
        c = np.asarray(roll_row)
        q = np.where(c == 0, 0.0, np.where(c == 1, 1.0, q))
    return q


def table(q, lo, hi):
    """B [D+1, hi+2] of one frame; B[0, 0] = P(lo <= count <= hi)"""
    D = len(q)
    B = np.zeros((D + 1, hi + 2))
    B[D, lo:hi + 1] = 1.0
    for j in range(D - 1, -1, -1):
        B[j, :hi + 1] = (1.0 - q[j]) * B[j + 1, :hi + 1] + q[j] * B[j + 1, 1:hi + 2]
    return B


def draw(p, u, lo, hi, roll_row=None):
    """(x [D] float64, log B[0][0], margin): margin = the smallest |u_j - a / B[j][c]| over the free notes that compared
    their uniform (inf if none did)"""
    p, u = np.asarray(p, np.float32), np.asarray(u, np.float32).astype(np.float64)
    D = len(p)
    forced = np.full(D, FREE) if roll_row is None else np.asarray(roll_row)
    q = recursion_q(p, roll_row)
    B = table(q, lo, hi)
    x, c, margin = np.zeros(D), 0, np.inf
    for j in range(D):
        if forced[j] <= 1:
            x[j] = float(forced[j])
        else:
            a, b = q[j] * B[j + 1, c + 1], (1.0 - q[j]) * B[j + 1, c]
            if a == 0.0:
                x[j] = 0.0
            elif b == 0.0:
                x[j] = 1.0
            else:
                r = a / B[j, c]
                margin = min(margin, abs(u[j] - r))
                x[j] = float(u[j] <= r)
        c += int(x[j])
        if c > hi:                                  # only an infeasible row gets here: the host refuses those
            raise ValueError("the roll forces more than hi = %d notes on" % hi)
    with np.errstate(divide='ignore'):
        return x, float(np.log(B[0, 0])), margin


def outcome_probability(p, x, lo, hi, roll_row=None):
    """the probability that draw() returns x, from the chain's own conditionals"""
    D = len(p)
    forced = np.full(D, FREE) if roll_row is None else np.asarray(roll_row)
    q = recursion_q(p, roll_row)
    B = table(q, lo, hi)
    c, pr = 0, 1.0
    for j in range(D):
        if forced[j] <= 1:
            if x[j] != forced[j]:
                return 0.0
        else:
            a, b = q[j] * B[j + 1, c + 1], (1.0 - q[j]) * B[j + 1, c]
            r = 0.0 if a == 0.0 else 1.0 if b == 0.0 else a / B[j, c]
            pr *= r if x[j] else 1.0 - r
        c += int(x[j])
        if c > hi:
            return 0.0
    return pr


def is_free(pair):
    return int(pair[0]) == FREE_PAIR[0] and int(pair[1]) == FREE_PAIR[1]


def sample_frame(xhat, u, roll_rows, pairs):
    """rows [R, D] of one frame: (x [R, D] float64, ell [R], logb [R], margin).  roll_rows [R, D] or None; pairs [R, 2]"""
    xhat, u = np.asarray(xhat, np.float32), np.asarray(u, np.float32)
    R, D = xhat.shape
    rows = np.full((R, D), FREE, np.uint8) if roll_rows is None else np.asarray(roll_rows)
    x = SR.sample_frame(xhat, u, rows)
    ell, logb, margin = SR.increment(xhat, rows), np.zeros(R), np.inf
    for r in range(R):
        if not is_free(pairs[r]):
            x[r], logb[r], m = draw(xhat[r], u[r], int(pairs[r][0]), int(pairs[r][1]), rows[r])
            margin = min(margin, m)
    return x, ell + logb, logb, margin


def frames(xhat, u, roll, voices):
    """the frame loop of both families' samplers given what the device chain hands to its draw: xhat, u [N, T, D] (the
    returned, unconstrained probabilities and the uniforms of Philox stream 1 at each frame's step), roll [N, T, D] or
    None, voices [N, T, 2].  Returns (Xs [N, T, D], ell [N, T], margin).  The models' forward passes are those of the
    existing reference loops (test_gpu_smc._vrnn_xhat_along / _vae_xhat_along), or the device's own x_hat."""
    N, T, D = np.shape(xhat)
    Xs, ell, margin = np.zeros((N, T, D)), np.zeros((N, T)), np.inf
    for t in range(T):
        Xs[:, t], ell[:, t], _, m = sample_frame(xhat[:, t], u[:, t], None if roll is None else roll[:, t], voices[:, t])
        margin = min(margin, m)
    return Xs, ell, margin


def feasible(roll_row, lo, hi):
    c = np.asarray(roll_row)
    on, free = int((c == 1).sum()), int((c > 1).sum())
    return on <= hi and on + free >= lo


# --------------------------------------------------------------------------- the GPU kernel test's own inputs
KERNEL_PAIRS = [(0, 0), (1, 1), (4, 4), (3, 4), (0, 15), (15, 15), FREE_PAIR]
SPECIAL = np.array([0.0, 1.0, 1e-7, np.float32(1) - np.float32(1e-7), 1e-9, 1 - 1e-9, 5e-8, 0.5], np.float32)


def kernel_case(R, P, nsteps, with_roll, seed):
    """direct inputs of the two kernels for R rows (R / P melodies): xhat, u [R, 88] float32, roll [R/P, nsteps, 88] or
    None, voices [R/P, nsteps, 2].  Probabilities hold both clip points and values beyond them; every frame is feasible."""
    rng = np.random.default_rng(seed)
    D, G = 88, R // P
    xhat = (1.0 / (1.0 + np.exp(-rng.normal(-2.5, 2.0, (R, D))))).astype(np.float32)
    xhat[:, 20:20 + len(SPECIAL)] = SPECIAL
    u = rng.random((R, D)).astype(np.float32)
    voices = np.zeros((G, nsteps, 2), np.uint8)
    for g in range(G):
        for k in range(nsteps):
            voices[g, k] = KERNEL_PAIRS[(g * nsteps + k + seed) % len(KERNEL_PAIRS)]
    roll = None
    if with_roll:
        roll = np.full((G, nsteps, D), FREE, np.uint8)
        for g in range(G):
            for k in range(nsteps):
                lo, hi = (int(v) for v in voices[g, k])
                n_on = 0 if is_free(voices[g, k]) else int(rng.integers(0, min(hi, 3) + 1))
                idx = rng.permutation(D)
                roll[g, k, idx[:n_on]] = 1
                roll[g, k, idx[n_on:n_on + int(rng.integers(0, 30))]] = 0
                assert is_free(voices[g, k]) or feasible(roll[g, k], lo, hi)
    return xhat, u, roll, voices
