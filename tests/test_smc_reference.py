"""CPU: the fp64 particle-filter reference (tests/smc_reference.py) on a small Markov chain whose histories can be
enumerated.  Its log Z must average to the exact evidence and its paths must approach the exact posterior marginals as P
grows; this checks the reference itself, against which tests/test_gpu_smc.py checks the kernels."""
import itertools

import numpy as np
import pytest

import smc_reference as SR

T = 5
A = np.array([[0.0, 0.0], [4.0, 0.0]])      # p(note 1 at t+1) = sigmoid(4 x_0(t) - 2): note 0 steers the clamped note 1
B = np.array([0.0, -2.0])
X0 = np.array([0.0, 0.0])
ROLL = np.array([[255, 1], [255, 1], [255, 0], [255, 1], [255, 1]], np.uint8)    # note 0 free, note 1 given


def xhat_of(prev):
    return (1.0 / (1.0 + np.exp(-(prev @ A.T + B)))).astype(np.float32)


def exact():
    """p(constraints) and p(note 0 at t | constraints) by enumerating the 2^T paths of note 0"""
    Z, marg = 0.0, np.zeros(T)
    for path in itertools.product((0.0, 1.0), repeat=T):
        prev, p = X0, 1.0
        for t in range(T):
            q = xhat_of(prev[None])[0].astype(np.float64)
            p *= q[0] if path[t] else 1 - q[0]
            p *= q[1] if ROLL[t, 1] else 1 - q[1]
            prev = np.array([path[t], float(ROLL[t, 1])])
        Z += p
        marg += p * np.array(path)
    return Z, marg / Z


def ancestral_marginals():
    """p(note 0 at t) under clamped ancestral sampling (no look-ahead): the P = 1 filter's target"""
    marg = np.zeros(T)
    for path in itertools.product((0.0, 1.0), repeat=T):
        prev, p = X0, 1.0
        for t in range(T):
            q = xhat_of(prev[None])[0].astype(np.float64)
            p *= q[0] if path[t] else 1 - q[0]
            prev = np.array([path[t], float(ROLL[t, 1])])
        marg += p * np.array(path)
    return marg


def run(P, G, tau, seed, rng):
    R = G * P
    filt = SR.Filter(G, P, T, tau, seed)
    hist = np.zeros((T, R, 2), np.uint8)
    prev = np.tile(X0, (R, 1))
    rows = np.repeat(ROLL[None], R, axis=0)
    ell_sum = np.zeros(R)
    for k in range(T):
        xhat = xhat_of(prev)
        u = rng.random((R, 2)).astype(np.float32)
        x = SR.sample_frame(xhat, u, rows[:, k])
        ell = SR.increment(xhat, rows[:, k])
        ell_sum += ell
        hist[k] = x
        a = filt.step(ell, k, k)
        prev = x[a]
    out, picks = SR.backtrack(filt.logW, filt.anc, hist, 1, seed, T)
    return filt, out[:, 0], ell_sum


def test_increment_clips_like_the_float32_bce():
    xhat = np.array([[0.0, 1.0, 0.25, 1e-9, 1 - 1e-9, 0.5]], np.float32)
    on = SR.increment(xhat, np.ones((1, 6), np.uint8))
    off = SR.increment(xhat, np.zeros((1, 6), np.uint8))
    free = SR.increment(xhat, np.full((1, 6), 255, np.uint8))
    lo, hi = np.float64(np.float32(1e-7)), np.float64(np.float32(1) - np.float32(1e-7))
    assert hi == 1 - 2.0 ** -23
    exp_on = np.log([lo, hi, 0.25, lo, hi, 0.5]).sum()
    exp_off = np.log(1 - np.array([lo, hi, 0.25, lo, hi, 0.5])).sum()
    np.testing.assert_allclose(on, [exp_on], rtol=1e-15)
    np.testing.assert_allclose(off, [exp_off], rtol=1e-15)
    assert free[0] == 0.0


def test_uniform_weights_never_resample_and_tau_zero_never_does():
    for P in (1, 3, 64, 1000):
        w, lse, e = SR.reweight(np.full(P, -np.log(P)), np.zeros(P))
        assert lse == 0.0 and e == P and np.all(w == -np.log(P))
    f = SR.Filter(4, 16, 3, 1.0, seed=1)
    for k in range(3):
        a = f.step(np.zeros(64), k, k)
        assert np.array_equal(a, np.arange(64))
    assert f.nres.sum() == 0 and np.all(f.logZ == 0.0)
    rng = np.random.default_rng(0)
    g = SR.Filter(4, 16, 3, 0.0, seed=1)
    for k in range(3):
        g.step(rng.standard_normal(64) * 5, k, k)
    assert g.nres.sum() == 0


def test_systematic_resampling_counts():
    rng = np.random.default_rng(1)
    for P in (1, 2, 7, 64):
        lw = rng.standard_normal(P) * 2
        lw -= np.log(np.exp(lw).sum())
        idx, _ = SR.systematic(lw, P, 0.37)
        counts = np.bincount(idx, minlength=P)
        W = np.exp(lw)
        assert np.all(np.abs(counts - P * W) < 1 + 1e-9)         # each particle gets floor or ceil of P W offspring
        assert np.all(np.diff(idx) >= 0)


def test_one_particle_is_clamped_ancestral_sampling():
    rng = np.random.default_rng(2)
    filt, paths, ell_sum = run(1, 50, 0.5, 3, rng)
    np.testing.assert_allclose(filt.logZ, ell_sum, rtol=0, atol=1e-12)
    assert filt.nres.sum() == 0
    assert np.all(paths[:, :, 1] == ROLL[None, :, 1])


def test_evidence_is_unbiased_and_marginals_converge():
    Z, post = exact()
    anc = ancestral_marginals()
    assert np.abs(post - anc).max() > 0.2                 # the constraints carry information backwards in time
    rng = np.random.default_rng(5)
    G = 3000
    for P, tau in ((4, 0.5), (16, 1.0), (8, 0.0)):
        filt, _, _ = run(P, G, tau, 11 + P, rng)
        r = np.exp(filt.logZ - np.log(Z))
        assert abs(r.mean() - 1) < 4 * r.std() / np.sqrt(G), (P, tau, r.mean(), r.std())
    errs = {}
    for P in (1, 64):
        filt, paths, _ = run(P, 2000, 0.5, 7, rng)
        m = paths[:, :, 0].mean(axis=0)
        sig = np.sqrt(post * (1 - post) / 2000)
        errs[P] = np.abs(m - post) / sig
    assert errs[64].max() < 4, errs[64]
    assert errs[1].max() > 8, errs[1]
    assert paths[:, :, 1].tolist() == np.repeat(ROLL[None, :, 1], 2000, 0).tolist()
