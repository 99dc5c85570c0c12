"""The tempered-sampling reference (tests/temper_reference.py) checked against itself and against the untempered helpers,
and the conditions on the INPUTS of tests/test_gpu_temperature.py that need no device: the power of its distribution and
particle-filter tests, and the flip cap of its fp64 frame-loop test."""
import numpy as np
import pytest

pytest.importorskip("torch")

import temper_reference as TR
import test_gpu_smc as TS

N_DRAWS = 65536            # sequences of GPU test 6


@pytest.fixture(scope="module", params=['cl_vrnn', 'cl_vae'])
def model(request):
    return request.param, TR.enumerable_params(request.param)


def test_neutral_temperature_reproduces_the_untempered_enumeration(model):
    which, p = model
    _, frames = TR.histories()
    if which == 'cl_vrnn':
        inputs = np.concatenate([np.zeros((len(frames), 1, TR.D)), frames[:, :-1]], 1)
        old = TS._vrnn_xhat_along(p, inputs, np.eye(10)[np.zeros(len(frames), int)], 0, 2)
    else:
        old = TS._vae_xhat_along(p, np.zeros((len(frames), TR.D)), frames, np.eye(4)[np.zeros(len(frames), int)], 0, 3)
    new = TR.xhat_of(which, p, 1.0)(frames)
    np.testing.assert_allclose(new[:, :, :2], old[:, :, :2], rtol=1e-13, atol=0)
    assert new[:, :, 2:].max() < 1e-12 and old[:, :, 2:].max() < 1e-12        # logit -40 (clipped to -30 by the routes)
    Z0, post0, anc0 = TS._exact(lambda f: old)
    Z1, post1, anc1 = TR.exact_constrained(TR.xhat_of(which, p, 1.0))
    np.testing.assert_allclose([Z1], [Z0], rtol=1e-12)
    np.testing.assert_allclose(post1, post0, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(anc1, anc0, rtol=1e-12, atol=1e-15)
    assert np.array_equal(TR.ROLL01, TS.ROLL01) and TR.T4 == TS.T4


@pytest.mark.parametrize("T", [0.5, 1.0, 2.0])
def test_enumerated_probabilities_sum_to_one(model, T):
    which, p = model
    pr, hs, p_other = TR.exact_free(which, p, T)
    assert abs(pr.sum() - 1) < 1e-12 and np.all(pr >= 0)
    cells = TR.free_cells(which, p, T)
    for t in range(TR.LAG[which], TR.T4):
        for a, b in ((0, 1), (1, 0)):
            assert abs(sum(cells['pair', t, a, b, va, vb] for va in (0, 1) for vb in (0, 1)) - 1) < 1e-12
    # notes 2..87: logit -40, so sigmoid(-30) after the routes' clip at T <= 1 and sigmoid(-20) = 2e-9 at T = 2
    assert p_other < 1e-12 if T <= 1 else 1e-9 < p_other < 3e-9


def test_temperature_moves_the_distribution_the_documented_way(model):
    which, p = model
    f = {T: TR.free_cells(which, p, T)['freq', 0, 1] for T in (0.5, 1.0, 2.0)}        # frame 0's note 1: logit -4
    np.testing.assert_allclose([f[1.0], f[2.0], f[0.5]], [1 / (1 + np.exp(4.0)), 1 / (1 + np.exp(2.0)), 1 / (1 + np.exp(8.0))],
                               rtol=1e-6)


@pytest.mark.parametrize("T", [0.5, 2.0])
def test_power_of_the_distribution_test(model, T):
    """GPU test 6 can tell T from T = 1: at least one tested cell moves by 8 standard errors or more"""
    which, p = model
    at_T, at_1 = TR.free_cells(which, p, T), TR.free_cells(which, p, 1.0)
    gap = max(abs(at_T[k] - at_1[k]) / TR.cell_se(at_T[k], N_DRAWS) for k in at_T)
    assert gap >= 8, gap


def test_power_of_the_particle_filter_test(model):
    """GPU test 8 at T = 2: exact posterior and clamped-ancestral marginals at least 0.2 apart on a free note"""
    which, p = model
    _, post, anc = TR.exact_constrained(TR.xhat_of(which, p, 2.0))
    assert np.abs(post - anc)[TR.ROLL01 > 1].max() >= 0.2


@pytest.mark.parametrize("which,run", [('cl_vrnn', r) for r in TR.ORACLE_RUNS] + [('cl_vae', r) for r in TR.ORACLE_RUNS_VAE])
def test_flip_cap_holds_on_the_gpu_tests_inputs(which, run):
    """GPU test 4's cap of 2 near flips per run is a condition on its inputs: the float32 run of the reference loop against
    its float64 run, on the very models, rolls and seeds the GPU test uses, stays within it (and within the window)"""
    T, Tz, seed = run
    fol = TR.flips_f32_against_f64(which, T, Tz, seed)
    print(which, run, "flips", fol.flips, "outside the window", fol.far)
    assert fol.clamp_wrong == 0 and fol.far == 0 and fol.flips <= TR.FLIP_CAP


def test_reference_loop_conventions():
    """Tz = 0 removes the dependence on eps; a clamped note is the roll's; T only rescales the logit"""
    p = TR.case_params('cl_vae')
    seeds, w, clamp = TR.vae_case_inputs()
    c = TR.VAE_CASE
    a, xa = TR.vae_generate(p, seeds, w, 1, 1, c['L'], None, 1.0, 0.0)
    b, xb = TR.vae_generate(p, seeds, w, 1, 2, c['L'], None, 1.0, 0.0)
    assert np.array_equal(xa, xb)
    _, xc = TR.vae_generate(p, seeds, w, 1, 2, c['L'], None, 1.0, 1.0)
    assert not np.array_equal(xb, xc)
    Xs, _ = TR.vae_generate(p, seeds, w, c['nsteps'], 3, c['L'], clamp, 0.5, 0.5)
    assert np.array_equal(Xs[clamp <= 1], clamp[clamp <= 1].astype(np.float64))
    _, x1 = TR.vae_generate(p, seeds, w, 1, 5, c['L'], None, 1.0, 0.7)
    _, x2 = TR.vae_generate(p, seeds, w, 1, 5, c['L'], None, 2.0, 0.7)
    logit = lambda q: np.log(q / (1 - q))
    np.testing.assert_allclose(logit(x2), logit(x1) / 2, rtol=1e-9, atol=1e-12)
