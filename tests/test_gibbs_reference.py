"""CPU: the fp64 reference of particle Gibbs (tests/gibbs_reference.py) on the enumerable Markov chain of
tests/test_smc_reference.py.  M independent chains of P = 2 particles must reach the enumerated posterior after K sweeps,
where the plain filter at P = 2 (their own sweep 0) is far off; this checks the reference, against which
tests/test_gpu_gibbs.py checks the kernels and the engines, and it is where K is chosen."""
import numpy as np

import gibbs_reference as GR
import smc_reference as SR
import test_smc_reference as TS

M = 2000            # chains: a marginal's standard error is at most 0.5 / sqrt(M) = 0.0112, so a miss of 0.1 is 8.9 of them
P = 2
TAU = 1.0           # at P = 2 an ESS below 0.5 * P = 1 cannot happen: tau = 1 resamples whenever the two weights differ
K = 64              # chosen below
SEED = 17


def _errors(paths, post):
    """|marginal of note 0 - posterior| per frame in binomial standard errors, for paths [G, T, 2]"""
    sig = np.sqrt(post * (1 - post) / paths.shape[0])
    return np.abs(paths[:, :, 0].mean(axis=0) - post) / sig


def test_the_seed_rule():
    assert GR.sweep_seed(5, 0) == 5
    assert GR.sweep_seed(5, 1) == 5 + 0x9E3779B97F4A7C15
    assert GR.sweep_seed(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C15 - 1           # mod 2^64
    assert len({GR.sweep_seed(0, s) for s in range(1000)}) == 1000
    assert GR.GIBBS_STREAM == 0xFFFFFFFA != SR.SMC_STREAM


def test_conditional_multinomial_draw():
    lw = np.log(np.array([0.1, 0.2, 0.3, 0.4]))
    idx, C = GR.conditional_multinomial(lw, np.array([0.95, 0.05, 0.11, 0.999999]))
    assert idx.tolist() == [0, 0, 1, 3]                  # particle 0 keeps itself; the others the first C_q > u
    idx, _ = GR.conditional_multinomial(np.log(np.array([0.5, 0.5 - 1e-12])), np.array([0.0, 1.0 - 1e-13]))
    assert idx.tolist() == [0, 1]                        # past the last cumulative weight: the last particle
    # the vectorised filter step draws what the one-melody function draws
    rng = np.random.default_rng(0)
    G, Pn, seed, m0 = 5, 7, 123, 4
    f = GR.ConditionalFilter(G, Pn, 3, 1.0, seed, m0)
    g = SR.Filter(G, Pn, 3, 1.0, seed, m0)
    for k in range(3):
        ell = -rng.random(G * Pn) * 3
        before = f.logW.copy()
        a = f.step(ell, 10 + k, k)
        u = GR.gibbs_uniforms(seed, 10 + k, m0, G, Pn)
        for m in range(G):
            w, lse, e = SR.reweight(before[m], ell.reshape(G, Pn)[m])
            assert e < Pn and f.resampled[k, m]
            idx, _ = GR.conditional_multinomial(w, u[m])
            assert np.array_equal(a[m * Pn:(m + 1) * Pn], m * Pn + idx)
            np.testing.assert_allclose(f.ess[m, k], e, rtol=1e-14)
        g.step(ell, 10 + k, k)                           # the weights, log Z and ESS are the plain filter's
        np.testing.assert_allclose(f.logZ, g.logZ, rtol=1e-14)
        np.testing.assert_allclose(f.ess[:, k], g.ess[:, k], rtol=1e-14)
        assert np.all(f.logW == -np.log(Pn)) and np.array_equal(f.nres, g.nres)
    # one particle never resamples; tau = 0 never does
    one = GR.ConditionalFilter(3, 1, 2, 1.0, 1)
    assert np.array_equal(one.step(-rng.random(3), 0, 0), np.arange(3)) and one.nres.sum() == 0
    never = GR.ConditionalFilter(3, 4, 2, 0.0, 1)
    assert np.array_equal(never.step(-rng.random(12) * 9, 0, 0), np.arange(12)) and never.nres.sum() == 0


def test_pins_and_path_backtracking():
    rng = np.random.default_rng(1)
    G, Pn, nsteps, S, D, L = 3, 4, 5, 2, 6, 2
    R, T = G * Pn, S + nsteps
    x_ref = (rng.random((G, nsteps, D)) < 0.5).astype(np.uint8)
    z_ref = rng.standard_normal((G, T, L)).astype(np.float32)
    bridge = (rng.random((G, D)) < 0.5).astype(np.float32)
    z = rng.standard_normal((R, L)).astype(np.float32)
    for step in (0, S - 1, S, T - 1):
        got = GR.pin_z(z, z_ref, step, Pn)
        assert np.array_equal(got[::Pn], z_ref[:, step])
        keep = np.ones(R, bool)
        keep[::Pn] = False
        assert np.array_equal(got[keep], z[keep])
    assert np.array_equal(GR.pin_z(z, z_ref, T, Pn), z)
    x = (rng.random((R, D)) < 0.5).astype(np.float32)
    hist = np.full((nsteps, R, D), 7, np.uint8)
    gx, gh = GR.pin_frame(x, hist, x_ref, bridge, S + 3, S, Pn)
    assert np.array_equal(gx[::Pn], x_ref[:, 3]) and np.array_equal(gh[3, ::Pn], x_ref[:, 3])
    assert (gh != 7).sum() <= G * D and np.array_equal(gx[1::Pn], x[1::Pn])
    gx, gh = GR.pin_frame(x, hist, x_ref, bridge, S - 1, S, Pn)
    assert np.array_equal(gx[::Pn], bridge) and np.all(gh == 7)
    gx, gh = GR.pin_frame(x, hist, x_ref, bridge, 0, S, Pn)         # a seed step before the bridge: nothing
    assert np.array_equal(gx, x) and np.all(gh == 7)
    # the path: frames as SR.backtrack returns them, latents and bridge along the same lineage
    anc = (np.arange(R)[None] // Pn * Pn + rng.integers(0, Pn, (nsteps, R))).astype(np.int32)
    hist = (rng.random((nsteps, R, D)) < 0.5).astype(np.uint8)
    zhist = rng.standard_normal((T, R, L)).astype(np.float32)
    brows = rng.random((R, D)).astype(np.float32)
    lw = rng.standard_normal((G, Pn))
    lw -= np.log(np.exp(lw).sum(axis=1, keepdims=True))
    want, picks = SR.backtrack(lw, anc, hist, 1, 9, T)
    assert np.array_equal(GR.final_picks(lw, 9, T), picks[:, 0])
    xr, zr, br, ren = GR.backtrack_path(picks[:, 0], anc, hist, zhist, brows, Pn, S)
    assert np.array_equal(xr, want[:, 0].astype(np.uint8))
    for m in range(G):
        r = m * Pn + picks[m, 0]
        for k in range(nsteps - 1, -1, -1):
            r = anc[k, r]
            assert np.array_equal(zr[m, S + k], zhist[S + k, r]) and ren[m, k] == (r != m * Pn)
        assert np.array_equal(zr[m, :S], zhist[:S, r]) and np.array_equal(br[m], brows[r])
    assert ren.any() and not ren.all()


def test_two_particles_and_sweeps_reach_the_posterior():
    """M = 2000 chains, P = 2, tau = 1, one run of 2K = 128 sweeps (the path after every sweep is kept, so the same run
    shows K and 2K).  K was chosen here over the powers of two as the smallest for which the paths after K and after 2K
    sweeps both lie within 4 standard errors of the enumerated posterior in every frame: observed maxima 26.2 (4 sweeps),
    20.1 (8), 12.2 (16), 4.7 (32: fails), 1.35 (K = 64), 2.18 (2K = 128); sweep 0, the plain filter at P = 2: 33.9.
    Without ancestor sampling a sweep renews about 17% of a path's frames on this chain, hence the slow approach."""
    _, post = TS.exact()
    assert 0.1 / np.sqrt(post * (1 - post) / M).max() >= 8
    rng = np.random.default_rng(5 + SEED)
    paths, logZ, renewed, filters = GR.run_sweeps(TS.xhat_of, TS.X0, TS.ROLL, M, P, 2 * K, TAU, SEED, rng)
    assert np.all(paths[:, :, :, 1] == TS.ROLL[None, None, :, 1])          # every retained path obeys the roll
    e0, eK, e2K = _errors(paths[0], post), _errors(paths[K - 1], post), _errors(paths[2 * K - 1], post)
    assert eK.max() < 4, eK
    assert e2K.max() < 4, e2K
    assert e0.max() > 8, e0                                # the power check: one pass of two particles is far off
    # the pinned particle survives every resampling of every conditional sweep, and the sweeps do resample and renew
    for f in filters[1:]:
        assert f.resampled.any()
        assert np.array_equal(f.anc[:, ::P], np.tile(np.arange(M) * P, (TS.T, 1)))
    assert renewed[0].all() and 0.05 < renewed[1:].mean() < 0.95
    # sweep 0 is the plain filter under the call's seed: its evidence estimate is the unbiased one
    Z, _ = TS.exact()
    r = np.exp(logZ[0] - np.log(Z))
    assert abs(r.mean() - 1) < 4 * r.std() / np.sqrt(M)
