"""CPU: the fp64 reference of the key-inferring particle filter (tests/smc_key_reference.py) on the small
Markov chain of tests/test_smc_reference.py, restated so that its transition depends on one of C = 3 keys.  The joint
p(constraints, key) can be enumerated; Z * posterior of the filter must average to it.  This checks the reference
itself, against which tests/test_gpu_smc_key.py checks the kernels."""
import itertools

import numpy as np

import smc_key_reference as KR
import smc_reference as SR

T = 5
C = 3
# p(note 1 at t+1 | key c) = sigmoid(A_c x_0(t) + B_c): under key 0 note 0 switches the clamped note 1 on, under key 1
# it barely matters, under key 2 it switches it off; note 0 is a fair coin under every key
A_KEY = np.array([4.0, 1.0, -4.0])
B_KEY = np.array([-2.0, -2.0, 0.5])
X0 = np.array([0.0, 0.0])
ROLL = np.array([[255, 1], [255, 1], [255, 0], [255, 1], [255, 1]], np.uint8)    # note 0 free, note 1 given
PRIOR = np.array([0.2, 0.5, 0.3])


def xhat_of(prev, key):
    """x_hat [R, 2] (float32, as the kernels hand it over) of rows with previous frame prev [R, 2] and key [R]"""
    z1 = A_KEY[key] * prev[:, 0] + B_KEY[key]
    return np.stack([np.full(len(prev), 0.5), 1.0 / (1.0 + np.exp(-z1))], axis=1).astype(np.float32)


def exact_joint():
    """p(constraints, key = c) [C] under PRIOR by enumerating the 2^T paths of note 0 for each key"""
    joint = np.zeros(C)
    for c in range(C):
        for path in itertools.product((0.0, 1.0), repeat=T):
            prev, p = X0, 1.0
            for t in range(T):
                q = xhat_of(prev[None], np.array([c]))[0].astype(np.float64)
                p *= q[0] if path[t] else 1 - q[0]
                p *= q[1] if ROLL[t, 1] else 1 - q[1]
                prev = np.array([path[t], float(ROLL[t, 1])])
            joint[c] += PRIOR[c] * p
    return joint


def run(P, G, tau, seed, rng, probs=PRIOR):
    R = G * P
    wr, keys = KR.init_categorical(np.tile(probs, (G, 1)), P, seed)
    filt = KR.KeyFilter(G, P, T, tau, seed, wr)
    hist = np.zeros((T, R, 2), np.uint8)
    prev = np.tile(X0, (R, 1))
    rows = np.repeat(ROLL[None], R, axis=0)
    ell_sum = np.zeros(R)
    for k in range(T):
        xhat = xhat_of(prev, np.argmax(filt.wr, axis=1))
        u = rng.random((R, 2)).astype(np.float32)
        x = SR.sample_frame(xhat, u, rows[:, k])
        ell = SR.increment(xhat, rows[:, k])
        ell_sum += ell
        hist[k] = x
        a = filt.step(ell, k, k)
        prev = x[a]
    out, picks = SR.backtrack(filt.logW, filt.anc, hist, 1, seed, T)
    return filt, out[:, 0], picks, ell_sum, wr


def test_systematic_key_allocation():
    rng = np.random.default_rng(0)
    rows = [PRIOR, np.array([0.0, 0.25, 0.0, 0.75, 0.0]), np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0]),
            rng.dirichlet(np.ones(10)), rng.dirichlet(np.full(25, 0.2))]
    for probs in rows:
        for P in (1, 7, 64, 1000):
            for u0 in (0.0, 0.37, 1 - 2.0 ** -25):
                keys, _ = KR.allocate_keys(probs, P, u0)
                counts = np.bincount(keys, minlength=len(probs))
                assert counts.sum() == P and np.all(np.diff(keys) >= 0)
                assert np.all(np.abs(counts - P * probs) < 1 + 1e-9), (probs, P, u0)     # floor or ceil of P * probs_c
                assert np.all(counts[probs == 0] == 0)
    # over many u0 the allocation is unbiased: the mean share of each key is its probability
    G, P = 20000, 7
    probs = rows[4]
    wr, keys = KR.init_categorical(np.tile(probs, (G, 1)), P, seed=9)
    share = wr.reshape(G, P, -1).mean(axis=1)
    se = share.std(axis=0, ddof=1) / np.sqrt(G)
    assert np.all(np.abs(share.mean(axis=0) - probs) < 4 * se + 1e-12), (share.mean(axis=0), probs)
    assert np.array_equal(np.argmax(wr, axis=1).reshape(G, P), keys)
    # the uniform is keyed by the global melody: a chunk starting at melody m0 draws what the whole batch draws there
    part, _ = KR.init_categorical(np.tile(probs, (50, 1)), P, seed=9, m0=100)
    assert np.array_equal(part, wr[100 * P:150 * P])


def test_one_hot_prior_gives_every_particle_that_key():
    for c in range(C):
        wr, keys = KR.init_categorical(np.tile(np.eye(C)[c], (40, 1)), 16, seed=3)
        assert np.all(keys == c) and np.array_equal(wr, np.tile(np.eye(C)[c], (640, 1)))


def test_logistic_normal_rows():
    rng = np.random.default_rng(1)
    G, P, C1 = 6, 5, 4
    mean, lv = rng.standard_normal((G, C1)), rng.standard_normal((G, C1)) - 1
    w = KR.init_logistic_normal(mean, lv, P, seed=4)
    assert w.shape == (G * P, C1 + 1) and np.all(w > 0)
    np.testing.assert_allclose(w.sum(axis=1), 1.0, rtol=0, atol=1e-15)
    # log(w_c / w_last) recovers s = mean + sd * eps; its moments over many particles are the prior's
    big = KR.init_logistic_normal(mean[:1], lv[:1], 40000, seed=5)
    s = np.log(big[:, :-1] / big[:, -1:])
    sd = np.exp(lv[0] / 2)
    assert np.all(np.abs(s.mean(axis=0) - mean[0]) < 4 * sd / np.sqrt(40000))
    assert np.all(np.abs(s.std(axis=0) / sd - 1) < 4 / np.sqrt(2 * 40000))
    part = KR.init_logistic_normal(mean[2:4], lv[2:4], P, seed=4, m0=2)
    assert np.array_equal(part, w[2 * P:4 * P])


def test_posterior_without_resampling_is_the_softmax_of_the_increments():
    rng = np.random.default_rng(2)
    filt, _, picks, ell_sum, wr = run(16, 30, 0.0, 5, rng)
    assert filt.nres.sum() == 0
    want = KR.posterior_from_increments(ell_sum.reshape(30, 16), wr)
    np.testing.assert_allclose(filt.w_post[:, -1], want, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(filt.w_post.sum(axis=2), 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(KR.take_w(filt.wr, picks, 16)[:, 0], filt.wr[np.arange(30) * 16 + picks[:, 0]])


def test_key_posterior_is_exact_on_the_enumerable_chain():
    joint = exact_joint()
    Z = joint.sum()
    post = joint / Z
    assert np.abs(post - PRIOR).max() >= 0.2, (post, PRIOR)     # a filter that ignored the weights would report PRIOR
    rng = np.random.default_rng(5)
    G = 3000
    for P, tau in ((8, 0.5), (32, 1.0), (16, 0.0)):
        filt, paths, picks, _, _ = run(P, G, tau, 11 + P, rng)
        est, se, ratio, se_r = KR.pooled_estimates(filt.logZ, filt.w_post[:, -1])
        assert np.all(np.abs(est - joint) < 4 * se + 1e-15), (P, tau, est, joint, se)    # + fp64 rounding of the sums
        assert np.all(np.abs(ratio - post) < 4 * se_r + 1e-12), (P, tau, ratio, post, se_r)
        r = np.exp(filt.logZ - np.log(Z))                       # the evidence with the key marginalised out
        assert abs(r.mean() - 1) < 4 * r.std() / np.sqrt(G), (P, tau, r.mean(), r.std())
        assert np.all(paths[:, :, 1] == ROLL[None, :, 1])
        # the keys of the returned paths follow the posterior (one draw per melody; the per-melody O(1/P) bias of the
        # ratio is below this resolution only for the larger P, so only the power side is asserted for all)
        drawn = np.bincount(np.argmax(KR.take_w(filt.wr, picks, P)[:, 0], axis=1), minlength=C) / G
        assert np.abs(drawn - PRIOR).max() > 0.1, (drawn, PRIOR)
    # power: the same summaries of a filter whose weights are ignored (every Z = 1, posterior = allocation) miss by far
    wr, _ = KR.init_categorical(np.tile(PRIOR, (G, 1)), 32, seed=43)
    flat = wr.reshape(G, 32, C).mean(axis=1)
    _, _, ratio0, se0 = KR.pooled_estimates(np.zeros(G), flat)
    assert np.abs(ratio0 - post).max() > 8 * se0.max() + 0.1
