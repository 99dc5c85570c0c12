"""-m gpu: sampling at a temperature on every device sampler: the TP instances of the persistent kernels
(csrc/generate.hip, csrc/vae_generate.hip), the frame chains with clv_sigmoid_temper / clv_scale_temper, the particle filter
on the tempered model, the public calls and the sample tools.  The reference is tests/temper_reference.py; the conditions
on this file's inputs that need no device (power, flip cap) are asserted in tests/test_temper_reference.py."""
import importlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import smc_reference as SR
import temper_reference as TR
import test_gpu_clamped_generation as TC
import test_gpu_smc as TS
from helpers import make_synthetic_pickle

pytestmark = pytest.mark.gpu

FREE, D = 255, 88
TEMPS = [(T, Tz) for T in (0.5, 2.0) for Tz in (0.0, 0.5, 1.5)]


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. neutral values are today's results, bit for bit
NEUTRAL = dict(temperature=1.0, z_temperature=1.0)


@pytest.mark.parametrize("use_graph", [True, False])
def test_neutral_values_change_nothing_vrnn(dev, use_graph):
    from clvae_amd.engine_generate import WPrior
    eng = TC._vrnn(dev, 2)
    N, S, nsteps, seed = 3, 4, 7, 11
    x_seed, w = TC._inputs(dev, N, S, 10, 1)
    roll = TC._roll(N, nsteps, seed=2)
    for clamp in (None, roll):
        xh0, xh1 = (torch.zeros(N, S + nsteps, D, device=dev) for _ in range(2))
        a = eng.generate(x_seed, w, nsteps, seed=seed, xhat_out=xh0, clamp=clamp)
        b = eng.generate(x_seed, w, nsteps, seed=seed, xhat_out=xh1, clamp=clamp, **NEUTRAL)
        assert torch.equal(a, b) and torch.equal(xh0, xh1) and 0 < float(a.mean()) < 1
        a = eng.generate(x_seed, w, nsteps, seed=seed, persistent=False, use_graph=use_graph, clamp=clamp)
        b = eng.generate(x_seed, w, nsteps, seed=seed, persistent=False, use_graph=use_graph, clamp=clamp, **NEUTRAL)
        assert torch.equal(a, b) and 0 < float(a.mean()) < 1
    kw = dict(resample_threshold=0.6, n_out=2, seed=seed, use_graph=use_graph)
    a = eng.generate_smc(x_seed, w, nsteps, roll, 8, **kw)
    b = eng.generate_smc(x_seed, w, nsteps, roll, 8, **kw, **NEUTRAL)
    assert _same(a, b) and len(a) == 4
    prior = WPrior.uniform(N, 10)
    a = eng.generate_smc(x_seed, None, nsteps, roll, 8, w_prior=prior, **kw)
    b = eng.generate_smc(x_seed, None, nsteps, roll, 8, w_prior=prior, **kw, **NEUTRAL)
    assert _same(a, b) and len(a) == 6


@pytest.mark.parametrize("use_graph", [True, False])
def test_neutral_values_change_nothing_vae(dev, use_graph):
    from clvae_amd.engine_generate import WPrior
    eng = TC._vae(dev, B=64)
    N, nsteps, seed = 5, 9, 99
    x_seed, w = TC._inputs(dev, N, None, 4, 2)
    roll = TC._roll(N, nsteps, seed=3)
    for clamp in (None, roll):
        xh0, xh1 = (torch.zeros(N, nsteps, D, device=dev) for _ in range(2))
        a = eng.generate(x_seed, w, nsteps, seed=seed, xhat_out=xh0, clamp=clamp)
        b = eng.generate(x_seed, w, nsteps, seed=seed, xhat_out=xh1, clamp=clamp, **NEUTRAL)
        assert torch.equal(a, b) and torch.equal(xh0, xh1) and 0 < float(a.mean()) < 1
        a = eng.generate(x_seed, w, nsteps, seed=seed, persistent=False, use_graph=use_graph, clamp=clamp)
        b = eng.generate(x_seed, w, nsteps, seed=seed, persistent=False, use_graph=use_graph, clamp=clamp, **NEUTRAL)
        assert torch.equal(a, b) and 0 < float(a.mean()) < 1
    kw = dict(resample_threshold=0.6, n_out=2, seed=seed, use_graph=use_graph)
    a = eng.generate_smc(x_seed, w, nsteps, roll, 8, **kw)
    b = eng.generate_smc(x_seed, w, nsteps, roll, 8, **kw, **NEUTRAL)
    assert _same(a, b) and len(a) == 4
    prior = WPrior.uniform(N, 4)
    a = eng.generate_smc(x_seed, None, nsteps, roll, 8, w_prior=prior, **kw)
    b = eng.generate_smc(x_seed, None, nsteps, roll, 8, w_prior=prior, **kw, **NEUTRAL)
    assert _same(a, b) and len(a) == 6


# ------------------------------------------------------------------ 2. + 3. every free note is [u <= tempered x_hat]
# (N, L, use_x_prev, gate, z_prior, S, with a roll): narrow and wide latents, both gates, the prior, S = 0, no roll
VRNN_CONFIGS = [(3, 2, True, 'hard_sigmoid', False, 5, True), (2, 5, False, 'sigmoid', False, 0, True),
                (1, 16, True, 'hard_sigmoid', True, 5, False), (2, 32, True, 'hard_sigmoid', False, 0, False),
                (2, 19, False, 'sigmoid', True, 3, True), (2, 32, True, 'sigmoid', False, 4, True)]


@pytest.mark.parametrize("T,Tz", TEMPS)
@pytest.mark.parametrize("N,L,use_x_prev,gate,z_prior,S,with_roll", VRNN_CONFIGS)
def test_persistent_tempered_generation_vrnn(dev, N, L, use_x_prev, gate, z_prior, S, with_roll, T, Tz):
    from clvae_amd import ops
    from clvae_amd.ops import ACT_NONE
    Cn, nsteps, seed = 10, 9, 4242
    eng = TC._vrnn(dev, L, use_x_prev, gate, Cn)
    f = dict(dtype=torch.float32, device=dev)
    x_seed, w = TC._inputs(dev, N, S, Cn, L)
    clamp = TC._roll(N, nsteps, seed=L) if with_roll else None
    kw = dict(seed=seed, z_prior=z_prior, temperature=T, z_temperature=Tz)
    xhat = torch.zeros(N, S + nsteps, D, **f)
    Xs = eng.generate(x_seed, w, nsteps, xhat_out=xhat, clamp=clamp, **kw)
    torch.cuda.synchronize()
    fixed = TC._check_clamped(Xs, clamp) if with_roll else torch.zeros(N, nsteps, D, dtype=torch.bool, device=dev)
    assert not torch.isnan(xhat).any() and set(torch.unique(Xs).tolist()) <= {0.0, 1.0}
    # every free note is [u <= x_hat] with the documented uniform (step S+j, stream 1, index n*88+k) and the tempered x_hat
    for j in range(nsteps):
        drawn = (TC._uniform(dev, N, seed, S + j) <= xhat[:, S + j]).float()
        free = ~fixed[:, j]
        assert torch.equal(Xs[:, j][free], drawn[free])
    # the temperature is at work: the untempered x_hat of the same first step differs
    xh1 = torch.zeros(N, S + nsteps, D, **f)
    eng.generate(x_seed, w, nsteps, xhat_out=xh1, clamp=clamp, seed=seed, z_prior=z_prior)
    assert not torch.equal(xh1[:, 0], xhat[:, 0])
    # teacher-forcing each step's input (seed frames, the unconstrained bridge sample, the returned frames) reproduces x_hat
    if S > 0:
        x_bridge = (TC._uniform(dev, N, seed, S - 1) <= xhat[:, S - 1]).float().unsqueeze(1)
        forced = torch.cat([x_seed, x_bridge, Xs[:, :-1]], dim=1).contiguous()
    else:
        forced = torch.cat([torch.zeros(N, 1, D, **f), Xs[:, :-1]], dim=1).contiguous()
    xhat2 = torch.zeros(N, S + nsteps, D, **f)
    eng.generate(forced, w, 0, xhat_out=xhat2, **kw)
    torch.cuda.synchronize()
    assert torch.equal(xhat2, xhat)
    # 3. the host-driven single-step chain: 2e-5 covers this comparison untempered; a logit difference grows by 1 / T
    inv_T, tz = TR.factors(T, Tz)
    tol = 2e-5 * max(1.0, 1.0 / T)
    st = eng.new_state(N)
    eps, z = torch.zeros(N, L, **f), torch.zeros(N, L, **f)
    worst = 0.0
    for t in range(S + nsteps):
        x = forced[:, t].contiguous()
        eng.enc_step(x, w, st)
        ops.philox_normal(eps, N * L, seed, t, 0, 0)
        if z_prior:
            st['zargs'].zero_()
        ops.scale_temper(N * L, eps, float(tz))
        ops.gauss_fwd(N, L, st['zargs'], eps, z, L, None)
        eng.dec_step(z, x if use_x_prev else None, w, st, act=ACT_NONE)
        ops.sigmoid_temper(N * D, st['xhat'], float(inv_T))
        torch.cuda.synchronize()
        worst = max(worst, float((xhat[:, t] - st['xhat']).abs().max()))
    print("single-step chain against the persistent kernel: max |dx_hat| %.3e (bound %.1e)" % (worst, tol))
    assert worst <= tol


@pytest.mark.parametrize("T,Tz", TEMPS)
@pytest.mark.parametrize("N,L,use_x_prev,z_prior,with_roll", [(5, 3, True, False, True), (3, 32, True, True, False),
                                                               (4, 8, False, False, True)])
def test_persistent_tempered_generation_vae(dev, N, L, use_x_prev, z_prior, with_roll, T, Tz):
    nsteps, seed, C = 9, 77, 4
    eng = TC._vae(dev, L=L, C=C, use_x_prev=use_x_prev)
    x_seed, w = TC._inputs(dev, N, None, C, L)
    clamp = TC._roll(N, nsteps, seed=L) if with_roll else None
    kw = dict(seed=seed, z_prior=z_prior, temperature=T, z_temperature=Tz)
    xhat = torch.zeros(N, nsteps, D, device=dev)
    Xs = eng.generate(x_seed, w, nsteps, xhat_out=xhat, clamp=clamp, **kw)
    torch.cuda.synchronize()
    fixed = TC._check_clamped(Xs, clamp) if with_roll else torch.zeros(N, nsteps, D, dtype=torch.bool, device=dev)
    assert not torch.isnan(xhat).any() and set(torch.unique(Xs).tolist()) <= {0.0, 1.0}
    for t in range(nsteps):
        drawn = (TC._uniform(dev, N, seed, t) <= xhat[:, t]).float()
        free = ~fixed[:, t]
        assert torch.equal(Xs[:, t][free], drawn[free])
    xh1 = torch.zeros(N, nsteps, D, device=dev)
    eng.generate(x_seed, w, nsteps, xhat_out=xh1, clamp=clamp, seed=seed, z_prior=z_prior)
    assert not torch.equal(xh1[:, 0], xhat[:, 0])
    # teacher forcing = a roll that fixes every note to the generated frames: the same x_hat, bit for bit
    xhat2 = torch.zeros(N, nsteps, D, device=dev)
    Xs2 = eng.generate(x_seed, w, nsteps, xhat_out=xhat2, clamp=Xs.to(torch.uint8), **kw)
    torch.cuda.synchronize()
    assert torch.equal(Xs2, Xs) and torch.equal(xhat2, xhat)


# ------------------------------------------------------------------ 4. fp64 reference loops under a constraint roll
def _check_follow(fol, T):
    """clamped notes exact; a free note differs from the reference only within window(T) of its probability; at most
    FLIP_CAP such flips per run (a condition on the inputs: tests/test_temper_reference.py)"""
    print("T = %g: %d flips, %d outside the window of %.1e, %d clamped notes wrong" % (T, fol.flips, fol.far, fol.win,
                                                                                    fol.clamp_wrong))
    assert fol.clamp_wrong == 0
    assert fol.far == 0
    assert fol.flips <= TR.FLIP_CAP


@pytest.mark.parametrize("T,Tz,seed", TR.ORACLE_RUNS)
def test_vrnn_tempered_generation_matches_reference(dev, T, Tz, seed):
    from clvae_amd.cl_vrnn.model import generate_samples_device, get_model
    c = TR.VRNN_CASE
    model, _ = get_model(4, D, 88, c['L'], c['T_len'], c['C'], True, 'adam', seed=c['model_seed'])
    p = TR.case_params('cl_vrnn')
    model.engine.P.set_weights(p)
    seeds, w, clamp = TR.vrnn_case_inputs()
    out = generate_samples_device(model, seeds, c['nsteps'], w, seed=seed, clamp=clamp, temperature=T, z_temperature=Tz)
    assert out.shape == (c['N'], c['nsteps'], D)
    fol = TR.Follow(out, TR.window(T))
    TR.vrnn_generate(p, seeds, w, c['nsteps'], seed, c['L'], clamp, T, Tz, follow=fol)
    _check_follow(fol, T)
    ref1, _ = TR.vrnn_generate(p, seeds, w, c['nsteps'], seed, c['L'], clamp, 1.0, 1.0)       # and it is not the T = 1 path
    assert not np.array_equal(ref1, out)


@pytest.mark.parametrize("T,Tz,seed", TR.ORACLE_RUNS_VAE)
def test_vae_tempered_generation_matches_reference(dev, T, Tz, seed):
    from clvae_amd.cl_vae.model import generate_samples_device, get_model
    c = TR.VAE_CASE
    model, _ = get_model(8, D, (88, c['L']), (88, c['C']), 'adam', use_x_prev=True, seed=c['model_seed'])
    p = TR.case_params('cl_vae')
    model.engine.P.set_weights(p)
    seeds, w, clamp = TR.vae_case_inputs()
    out = generate_samples_device(model, seeds, c['nsteps'], w, seed=seed, clamp=clamp, temperature=T, z_temperature=Tz)
    fol = TR.Follow(out, TR.window(T))
    TR.vae_generate(p, seeds, w, c['nsteps'], seed, c['L'], clamp, T, Tz, follow=fol)
    _check_follow(fol, T)
    ref1, _ = TR.vae_generate(p, seeds, w, c['nsteps'], seed, c['L'], clamp, 1.0, 1.0)
    assert not np.array_equal(ref1, out)


# ------------------------------------------------------------------ 5. persistent kernel against the frame chain
def _agree_until_a_near_flip(dev, Xp, Xf, xhat, seed, step0, clamp, win):
    """test_gpu_clamped_generation's rule with the scaled window: the two routes give the same frames and may part only
    where a free draw lies within `win` of its probability"""
    TC._check_clamped(Xp, clamp)
    TC._check_clamped(Xf, clamp)
    N = Xp.shape[0]
    for j in range(Xp.shape[1]):
        diff = Xp[:, j] != Xf[:, j]
        if diff.any():
            u = TC._uniform(dev, N, seed, step0 + j)
            assert float((u - xhat[:, step0 + j]).abs()[diff].max()) < win
            return j
    return None


@pytest.mark.parametrize("T,Tz", [(0.5, 0.5), (2.0, 1.5), (0.8, 0.0)])
@pytest.mark.parametrize("L", [2, 19])
def test_vrnn_persistent_matches_frame_chain_at_a_temperature(dev, L, T, Tz):
    N, S, nsteps, seed = 4, 3, 8, 7
    eng = TC._vrnn(dev, L)
    x_seed, w = TC._inputs(dev, N, S, 10, 3)
    clamp = TC._roll(N, nsteps, seed=9)
    kw = dict(seed=seed, clamp=clamp, temperature=T, z_temperature=Tz)
    for xs, s0 in ((x_seed, S), (torch.zeros(N, 0, D, device=dev), 0)):           # S = 0: no bridge
        xhat = torch.zeros(N, s0 + nsteps, D, device=dev)
        Xp = eng.generate(xs, w, nsteps, xhat_out=xhat, **kw)
        Xf = eng.generate(xs, w, nsteps, persistent=False, **kw)
        Xe = eng.generate(xs, w, nsteps, persistent=False, use_graph=False, **kw)
        torch.cuda.synchronize()
        assert torch.equal(Xf, Xe)                  # the added launches are captured like the rest
        _agree_until_a_near_flip(dev, Xp, Xf, xhat, seed, s0, clamp, TR.window(T))


@pytest.mark.parametrize("T,Tz", [(0.5, 0.5), (2.0, 1.5), (0.8, 0.0)])
def test_vae_persistent_matches_frame_chain_at_a_temperature(dev, T, Tz):
    N, nsteps, seed = 6, 9, 5
    eng = TC._vae(dev)
    x_seed, w = TC._inputs(dev, N, None, 4, 4)
    clamp = TC._roll(N, nsteps, seed=11)
    kw = dict(seed=seed, clamp=clamp, temperature=T, z_temperature=Tz)
    xhat = torch.zeros(N, nsteps, D, device=dev)
    Xp = eng.generate(x_seed, w, nsteps, xhat_out=xhat, **kw)
    Xf = eng.generate(x_seed, w, nsteps, persistent=False, **kw)
    Xe = eng.generate(x_seed, w, nsteps, persistent=False, use_graph=False, **kw)
    torch.cuda.synchronize()
    assert torch.equal(Xf, Xe)
    _agree_until_a_near_flip(dev, Xp, Xf, xhat, seed, 0, clamp, TR.window(T))


# ------------------------------------------------------------------ 6. the distribution is the tempered one
N_DRAWS = 65536


@pytest.mark.parametrize("T", [2.0, 0.5])
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_distribution_is_the_tempered_one(dev, which, T):
    if which == 'cl_vrnn':
        eng, p = TS._enumerable_vrnn(dev, B=4)
        x_seed, C = torch.zeros(N_DRAWS, 0, D, device=dev), 10
    else:
        eng, p = TS._enumerable_vae(dev, B=4)
        x_seed, C = torch.zeros(N_DRAWS, D, device=dev), 4
    want, at_1 = TR.free_cells(which, p, T), TR.free_cells(which, p, 1.0)
    # power, from the enumeration alone: some tested cell tells T from T = 1 by 8 standard errors or more
    assert max(abs(want[k] - at_1[k]) / TR.cell_se(want[k], N_DRAWS) for k in want) >= 8
    w = torch.as_tensor(np.eye(C, dtype=np.float32)[np.arange(N_DRAWS) % C], device=dev)
    Xs = eng.generate(x_seed, w, TR.T4, seed=97, temperature=T)
    torch.cuda.synchronize()
    Xs = Xs.cpu().numpy()
    assert set(np.unique(Xs)) <= {0.0, 1.0}
    if T <= 1:              # logit -40: at T = 2 their probability is 2e-9 each over 22 M draws, not "never"
        assert np.all(Xs[:, :, 2:] == 0)
    got = TR.cell_counts(which, Xs)
    worst = max(want, key=lambda k: abs(got[k] - want[k]) / TR.cell_se(want[k], N_DRAWS))
    print("%s T = %g: worst cell %s: %.5f against %.5f (%.2f SE)" % (which, T, worst, got[worst], want[worst],
          abs(got[worst] - want[worst]) / TR.cell_se(want[worst], N_DRAWS)))
    for k in want:
        assert abs(got[k] - want[k]) < 4 * TR.cell_se(want[k], N_DRAWS), (k, got[k], want[k])


# ------------------------------------------------------------------ 7. z_temperature = 0 removes the latent noise
def test_zero_z_temperature_removes_the_latent_noise_vrnn(dev):
    eng = TC._vrnn(dev, 5)
    N, S = 3, 6
    x_seed, w = TC._inputs(dev, N, S, 10, 12)

    def xhat_of(seed, Tz):
        xh = torch.zeros(N, S, D, device=dev)
        eng.generate(x_seed, w, 0, seed=seed, xhat_out=xh, temperature=0.8, z_temperature=Tz)       # all frames given
        torch.cuda.synchronize()
        return xh
    assert torch.equal(xhat_of(1, 0.0), xhat_of(2, 0.0)) and not torch.equal(xhat_of(1, 1.0), xhat_of(2, 1.0))
    assert torch.equal(xhat_of(1, 1.0), xhat_of(1, 1.0))
    # the frame chain's x_hat buffer after step 0 of an unseeded run (its input is the zero frame)
    kept = {}
    real = eng.new_state
    eng.new_state = lambda B: kept.setdefault('st', real(B))
    x0 = torch.zeros(N, 0, D, device=dev)

    def chain_xhat(seed, Tz):
        kept.clear()
        eng.generate(x0, w, 1, seed=seed, persistent=False, use_graph=False, temperature=0.8, z_temperature=Tz)
        torch.cuda.synchronize()
        return kept['st']['xhat'].clone()
    try:
        assert torch.equal(chain_xhat(1, 0.0), chain_xhat(2, 0.0)) and not torch.equal(chain_xhat(1, 1.0), chain_xhat(2, 1.0))
    finally:
        del eng.new_state


def test_zero_z_temperature_removes_the_latent_noise_vae(dev):
    eng = TC._vae(dev, L=8)
    N = 5
    x_seed, w = TC._inputs(dev, N, None, 4, 13)

    def xhat_of(seed, Tz):
        xh = torch.zeros(N, 1, D, device=dev)
        eng.generate(x_seed, w, 1, seed=seed, xhat_out=xh, temperature=0.8, z_temperature=Tz)
        torch.cuda.synchronize()
        return xh
    assert torch.equal(xhat_of(1, 0.0), xhat_of(2, 0.0)) and not torch.equal(xhat_of(1, 1.0), xhat_of(2, 1.0))

    def chain_xhat(seed, Tz):
        eng.generate(x_seed, w, 1, seed=seed, persistent=False, use_graph=False, temperature=0.8, z_temperature=Tz)
        torch.cuda.synchronize()
        return eng.logits[:N].clone()
    assert torch.equal(chain_xhat(1, 0.0), chain_xhat(2, 0.0)) and not torch.equal(chain_xhat(1, 1.0), chain_xhat(2, 1.0))


# ------------------------------------------------------------------ 8. the particle filter on the tempered model
def _log_q_sum(xhats, roll):
    """fp64 sum of log q over the clamped notes of every frame, q from the float32 x_hat the chain handed to the filter"""
    return sum(SR.increment(xh, roll[:, j]) for j, xh in enumerate(xhats))


def test_one_particle_is_tempered_clamped_generation_vrnn(dev):
    from clvae_amd import ops
    from clvae_amd.ops import ACT_NONE
    eng, _ = TS._vrnn(dev)
    N, S, nsteps, seed, L, T, Tz = 5, 3, 7, 21, 2, 2.0, 0.5
    x_seed, w = TS._inputs(dev, N, S, 10, 1)
    roll = TS._roll(np.random.default_rng(2), N, nsteps)
    kw = dict(seed=seed, temperature=T, z_temperature=Tz)
    ref = eng.generate(x_seed, w, nsteps, persistent=False, clamp=roll, **kw)
    r = eng.generate_smc(x_seed, w, nsteps, roll, 1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(r.Xs[:, 0], ref)
    assert int(r.resamples.sum()) == 0 and bool((r.ess == 1.0).all())
    assert not torch.equal(ref, eng.generate(x_seed, w, nsteps, persistent=False, clamp=roll, seed=seed))
    # log Z = sum of log q along that path, q from the x_hat the same chain gives when it is fed the path
    inv_T, tz = TR.factors(T, Tz)
    f = dict(dtype=torch.float32, device=dev)
    st = eng.new_state(N)
    eps, z, x = torch.zeros(N, L, **f), torch.zeros(N, L, **f), torch.zeros(N, D, **f)
    xhats = []
    for t in range(S + nsteps):
        if t < S:
            x = x_seed[:, t].contiguous()
        eng.enc_step(x, w, st)
        ops.philox_normal(eps, N * L, seed, t, 0, 0)
        ops.scale_temper(N * L, eps, float(tz))
        ops.gauss_fwd(N, L, st['zargs'], eps, z, L, None)
        eng.dec_step(z, x, w, st, act=ACT_NONE)
        ops.sigmoid_temper(N * D, st['xhat'], float(inv_T))
        torch.cuda.synchronize()
        if t >= S:
            xhats.append(st['xhat'].cpu().numpy())
            x = ref[:, t - S].contiguous()
        else:                   # the sample of a seed step: only the bridge's (t = S - 1) is ever an input
            x = (TC._uniform(dev, N, seed, t) <= st['xhat']).float()
    np.testing.assert_allclose(r.log_evidence.cpu().numpy(), _log_q_sum(xhats, roll), rtol=1e-12, atol=0)


def test_one_particle_is_tempered_clamped_generation_vae(dev):
    from clvae_amd import ops
    from clvae_amd.ops import ACT_NONE
    eng, _ = TS._vae(dev)
    N, nsteps, seed, L, T, Tz = 6, 8, 13, 3, 2.0, 0.5
    x_seed, w = TS._inputs(dev, N, None, 4, 3)
    roll = TS._roll(np.random.default_rng(4), N, nsteps)
    kw = dict(seed=seed, temperature=T, z_temperature=Tz)
    ref = eng.generate(x_seed, w, nsteps, persistent=False, clamp=roll, **kw)
    r = eng.generate_smc(x_seed, w, nsteps, roll, 1, **kw)
    torch.cuda.synchronize()
    assert torch.equal(r.Xs[:, 0], ref)
    inv_T, tz = TR.factors(T, Tz)
    eps = torch.zeros(N, L, dtype=torch.float32, device=dev)
    x_in, hist, xhats = x_seed.clone(), x_seed.clone(), []
    for t in range(nsteps):
        eng.encode_z(x_in, w, N)
        ops.philox_normal(eps, N * L, seed, t, 0, 0)
        ops.scale_temper(N * L, eps, float(tz))
        ops.gauss_fwd(N, L, eng.zargs, eps, eng.z, L, None)
        eng.decode(w, eng.z, hist, N, act=ACT_NONE)
        ops.sigmoid_temper(N * D, eng.logits, float(inv_T))
        torch.cuda.synchronize()
        xhats.append(eng.logits[:N].cpu().numpy())
        hist, x_in = x_in, ref[:, t].contiguous()
    np.testing.assert_allclose(r.log_evidence.cpu().numpy(), _log_q_sum(xhats, roll), rtol=1e-12, atol=0)


def _check_exactness(gen, xhat_fn, G=256, P=64):
    """test_gpu_smc._check_exactness on a tempered x_hat function, without its "notes 2..87 are silent" assertion (at T = 2
    each sounds with probability 2e-9, which is not never; they feed nothing back)"""
    Z, post, ancm = TR.exact_constrained(xhat_fn)
    free = TR.ROLL01 > 1
    assert np.abs(post - ancm)[free].max() >= 0.2
    roll = np.full((G, TR.T4, D), FREE, np.uint8)
    roll[:, :, :2] = TR.ROLL01
    r = gen(roll, P)
    Xs, logZ = r.Xs[:, 0].cpu().numpy(), r.log_evidence.cpu().numpy()
    assert np.all(Xs[:, :, :2][:, ~free] == TR.ROLL01[~free])
    ratio = np.exp(logZ - np.log(Z))
    print("evidence ratio %.4f +- %.4f" % (ratio.mean(), ratio.std() / np.sqrt(G)))
    assert abs(ratio.mean() - 1) < 4 * ratio.std() / np.sqrt(G) + 1e-9, (ratio.mean(), ratio.std())
    sig = np.sqrt(np.maximum(post * (1 - post), 0.01) / G)
    m = Xs[:, :, :2].mean(0)
    assert np.all(np.abs(m - post)[free] < 4 * sig[free]), (m, post)
    r1 = gen(roll, 1)                                     # the power check: ancestral sampling is far off
    m1 = r1.Xs[:, 0, :, :2].cpu().numpy().mean(0)
    assert np.abs(m1 - post)[free].max() > 8 * sig[free][np.argmax(np.abs(m1 - post)[free])]
    assert np.all(np.isfinite(r1.log_evidence.cpu().numpy()))
    return Z


def test_exact_tempered_posterior_on_enumerable_vrnn(dev):
    eng, p = TS._enumerable_vrnn(dev, B=4)
    G, T = 256, 2.0
    x_seed = torch.zeros(G, 0, D, device=dev)
    w = torch.as_tensor(np.eye(10, dtype=np.float32)[np.arange(G) % 10], device=dev)
    Z = _check_exactness(lambda roll, P: eng.generate_smc(x_seed, w, TR.T4, roll, P, seed=41, temperature=T),
                         TR.xhat_of('cl_vrnn', p, T), G=G)
    Z1, _, _ = TR.exact_constrained(TR.xhat_of('cl_vrnn', p, 1.0))
    assert abs(np.log(Z) - np.log(Z1)) > 0.5            # the tempered model's evidence, not the trained model's


def test_exact_tempered_posterior_on_enumerable_vae(dev):
    eng, p = TS._enumerable_vae(dev, B=4096)              # 256 x 64 rows: four chunks
    G, T = 256, 2.0
    x_seed = torch.zeros(G, D, device=dev)
    w = torch.as_tensor(np.eye(4, dtype=np.float32)[np.arange(G) % 4], device=dev)
    _check_exactness(lambda roll, P: eng.generate_smc(x_seed, w, TR.T4, roll, P, seed=43, temperature=T),
                     TR.xhat_of('cl_vae', p, T), G=G)


def test_tempered_filter_graph_equals_eager_and_chunking_changes_nothing(dev):
    rng = np.random.default_rng(7)
    ev, _ = TS._vrnn(dev)
    N, S, nsteps, P, seed = 6, 2, 6, 8, 31
    x_seed, w = TS._inputs(dev, N, S, 10, 8)
    roll = TS._roll(rng, N, nsteps, frac=0.2)
    kw = dict(resample_threshold=0.6, n_out=3, seed=seed, temperature=0.7, z_temperature=1.3)
    a = ev.generate_smc(x_seed, w, nsteps, roll, P, **kw)
    b = ev.generate_smc(x_seed, w, nsteps, roll, P, use_graph=False, **kw)
    c = ev.generate_smc(x_seed, w, nsteps, roll, P, chunk=4, **kw)
    d = ev.generate_smc(x_seed, w, nsteps, roll, P, chunk=1, **kw)
    torch.cuda.synchronize()
    assert _same(a, b) and _same(a, c) and _same(a, d)
    va, _ = TS._vae(dev, B=48)
    vb, _ = TS._vae(dev, B=16)
    x1, w1 = TS._inputs(dev, N, None, 4, 9)
    roll = TS._roll(rng, N, nsteps, frac=0.2)
    a = va.generate_smc(x1, w1, nsteps, roll, P, **kw)
    b = va.generate_smc(x1, w1, nsteps, roll, P, use_graph=False, **kw)
    c = vb.generate_smc(x1, w1, nsteps, roll, P, **kw)
    torch.cuda.synchronize()
    assert _same(a, b) and _same(a, c)


# ------------------------------------------------------------------ 9. refusals
def test_refusals(dev):
    import ctypes as C
    from clvae_amd import _lib, ops
    from clvae_amd.cl_vae import model as MV
    from clvae_amd.cl_vrnn import model as MR
    from clvae_amd.harmonize import harmonize
    N, nsteps = 2, 4
    vr, _ = MR.get_model(4, 88, 88, 2, 8, 3, True, 'adam', seed=1)
    va, _ = MV.get_model(4, 88, (88, 2), (88, 3), 'adam', use_x_prev=True, seed=1)
    seeds_r, seeds_a, w = np.zeros((N, 2, 88)), np.zeros((N, 88)), np.eye(3)[[0, 1]]
    roll = np.full((N, nsteps, 88), FREE, np.uint8)
    src = np.zeros((N, nsteps, 88))
    src[:, :, 40] = 1
    bad = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float('nan')), dict(temperature=float('inf')),
           dict(temperature=1e-39), dict(temperature=1e46), dict(temperature=True), dict(z_temperature=-0.1),
           dict(z_temperature=float('nan')), dict(z_temperature=float('inf')), dict(z_temperature=False)]
    for kw in bad:
        for model, seeds in ((vr, seeds_r), (va, seeds_a)):
            gen = MR.generate_samples_device if model is vr else MV.generate_samples_device
            with pytest.raises(ValueError):
                gen(model, seeds, nsteps, w, **kw)
            with pytest.raises(ValueError):
                gen(model, seeds, nsteps, w, clamp=roll, particles=4, **kw)
            with pytest.raises(ValueError):
                harmonize(model, seeds, src, w, **kw)
            xs = torch.as_tensor(seeds, dtype=torch.float32, device=dev)
            wt = torch.as_tensor(w, dtype=torch.float32, device=dev)
            with pytest.raises(ValueError):
                model.engine.generate(xs, wt, nsteps, **kw)
            with pytest.raises(ValueError):
                model.engine.generate(xs, wt, nsteps, persistent=False, **kw)
            with pytest.raises(ValueError):
                model.engine.generate_smc(xs, wt, nsteps, roll, 4, **kw)
    # the C ABI: CLV_EINVAL (-1) for a zero, negative or non-finite inv_temperature and a negative or non-finite z_temperature
    lib, EINVAL = _lib.lib(), -1
    buf = torch.zeros(64, device=dev)
    stream = ops._stream()
    nan, inf = float('nan'), float('inf')
    for v in (0.0, -1.0, nan, inf, -inf):
        assert lib.clv_sigmoid_temper(64, ops._ptr(buf), C.c_float(v), stream) == EINVAL
    for v in (-1.0, nan, inf, -inf):
        assert lib.clv_scale_temper(64, ops._ptr(buf), C.c_float(v), stream) == EINVAL
    assert lib.clv_sigmoid_temper(64, ops._ptr(buf), C.c_float(2.0), stream) == 0
    assert lib.clv_scale_temper(64, ops._ptr(buf), C.c_float(0.0), stream) == 0
    torch.cuda.synchronize()
    assert bool((buf == 0).all())                   # sigmoid(0) = 0.5, then scaled by 0
    eng = TC._vrnn(dev, 2)
    x_seed, wv = TC._inputs(dev, N, 2, 10, 1)
    Xs = torch.zeros(N, nsteps, D, device=dev)
    cfg, P, off = eng.cfg, eng.P, eng.off
    rows = lambda name, r: P.rows(P.params, name, r)

    def vrnn_call(inv_T, Tz):
        try:
            ops.vrnn_generate(N, 2, nsteps, D, 88, 2, 10, eng.gate_act, False, 1, x_seed, wv, P.p('encoder_h/kernel'),
                              rows('encoder_h/kernel', D), P.p('encoder_h/bias'), P.p('encoder_h/recurrent_kernel'),
                              P.p('Zargs/kernel'), P.p('Zargs/bias'), P.p('decoder_h/kernel'), rows('decoder_h/kernel', off),
                              rows('decoder_h/kernel', off + 2), P.p('decoder_h/bias'), P.p('decoder_h/recurrent_kernel'),
                              P.p('X_decoded_mean/kernel'), P.p('X_decoded_mean/bias'), Xs, None, temper=(inv_T, Tz))
        except _lib.ClvError as e:
            return str(e)
        return None
    ev = TC._vae(dev)
    xs1, w1 = TC._inputs(dev, N, None, 4, 2)
    Pv = ev.P

    def vae_call(inv_T, Tz):
        try:
            ops.vae_generate(N, nsteps, D, 88, 3, 4, True, False, 1, xs1, w1, Pv.p('h/kernel'), Pv.p('h/bias'),
                             Pv.p('zargs/kernel'), Pv.p('zargs/bias'), Pv.p('decoder_h/kernel'), Pv.p('decoder_h/bias'),
                             Pv.p('x_decoded_mean/kernel'), Pv.p('x_decoded_mean/bias'), Xs, None, temper=(inv_T, Tz))
        except _lib.ClvError as e:
            return str(e)
        return None
    for call in (vrnn_call, vae_call):
        assert call(1.25, 0.5) is None and call(1.0, 0.0) is None
        for inv_T, Tz in ((0.0, 1.0), (-1.0, 1.0), (nan, 1.0), (inf, 1.0), (1.0, -1.0), (1.0, nan), (1.0, inf)):
            msg = call(inv_T, Tz)
            assert msg is not None and '(-1)' in msg, (inv_T, Tz, msg)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 10. both sample tools at a temperature
@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_sample_tools_at_a_temperature(dev, tmp_path, monkeypatch, capsys, which):
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, HARMONIZE_FLAGS, TEMPERATURE_FLAGS, parser_for
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    TRN = importlib.import_module('clvae_amd.%s.train' % which)
    data = make_synthetic_pickle(str(tmp_path / "syn.pickle"), n_songs=(10, 4, 4), seed=1)
    mdir, sdir, hdir = str(tmp_path / "models"), str(tmp_path / "samples"), str(tmp_path / "harmonized")
    for d_ in (mdir, sdir, hdir):
        os.makedirs(d_)
    extra = ['--latent_dim', '4', '--batch_size', '50'] if which == 'cl_vae' else ['--seq_length', '8', '--batch_size', '20']
    np.random.seed(0)
    TRN.train(TRN.build_parser().parse_args(['m', '--use_x_prev', '--num_epochs', '2', '--patience', '0', '--train_file', data,
                                             '--model_dir', mdir] + extra))
    parser = parser_for('%s.sample' % which, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS + TEMPERATURE_FLAGS)
    common = ['h', '-n', '3', '-t', '8', '--seed', '4', '-i', os.path.join(mdir, 'm.h5'), '--train_file', data]
    temper = ['--temperature', '0.7', '--z_temperature', '0.5']
    with pytest.raises(SystemExit) as e:
        parser.parse_args(common + ['--sample_dir', sdir, '--host_loop', '--temperature', '0.7'])
    assert e.value.code != 0
    # alone: the device loop is implied; the tempered call is the one made
    seen = []
    real_gen = S.M.generate_samples_device

    def spy_gen(*a, **kw):
        seen.append(kw)
        return real_gen(*a, **kw)
    monkeypatch.setattr(S.M, 'generate_samples_device', spy_gen)
    np.random.seed(3)
    rolls = S.sample(parser.parse_args(common + ['--sample_dir', sdir] + temper))
    assert len(rolls) == 3 and all(set(np.unique(r)) <= {0.0, 1.0} for r in rolls)
    assert len(seen) == 1 and seen[0]['temperature'] == 0.7 and seen[0]['z_temperature'] == 0.5
    files = os.listdir(sdir)
    for j in range(3):
        assert 'h_%d.mid' % j in files and open(os.path.join(sdir, 'h_%d.mid' % j), 'rb').read()[:4] == b'MThd'
    # with --harmonize top --particles 8: the kept voice is intact
    sources = []
    real = S.harmonize

    def spy(model, seeds, src, w_vals, **kw):
        sources.append((np.asarray(src), kw))
        return real(model, seeds, src, w_vals, **kw)
    monkeypatch.setattr(S, 'harmonize', spy)
    np.random.seed(3)
    capsys.readouterr()
    rolls = S.sample(parser.parse_args(common + ['--sample_dir', hdir, '--harmonize', 'top', '--particles', '8'] + temper))
    printed = capsys.readouterr().out
    assert len(rolls) == 3 and len(sources) == 1
    kw = sources[0][1]
    assert kw['particles'] == 8 and kw['temperature'] == 0.7 and kw['z_temperature'] == 0.5
    assert sum('log p(voice) per frame' in line for line in printed.splitlines()) == 3
    TC._top_voice_kept(rolls, sources[0][0])
    files = os.listdir(hdir)
    for j in range(3):
        for name in ('h_%d.mid' % j, 'h_%d_source.mid' % j):
            assert name in files and open(os.path.join(hdir, name), 'rb').read()[:4] == b'MThd'
