"""-m gpu: the particle filter with a label w per particle: the three kernels against the fp64 reference
(tests/smc_key_reference.py), the identities of the definition on both engines, exactness of the key posterior on models
whose histories can be enumerated, and the sample CLIs with --infer_key."""
import itertools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import smc_key_reference as KR
import smc_reference as SR
import test_gpu_smc as TG                     # its engines, inputs and fp64 frame oracles (imported, not collected here)
from helpers import make_synthetic_pickle
from oracle import clvae_oracle as O

pytestmark = pytest.mark.gpu

FREE = 255
D = 88
ULP = 2.0 ** -23                              # of 1.0 in float32


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _probs(rng, G, C):
    """skewed rows with zeros; row 0 one-hot (where G allows: in the middle), row 1 all mass in the last class"""
    p = rng.dirichlet(np.full(C, 0.3), G)
    p[rng.random((G, C)) < 0.3] = 0.0
    p[:, 0] += (p.sum(axis=1) == 0)
    p /= p.sum(axis=1, keepdims=True)
    p[0] = np.eye(C)[C // 2]
    if G > 1:
        p[1] = np.eye(C)[C - 1]
    if G > 2:
        p[2] = np.eye(C)[0] * 0.5 + np.eye(C)[C - 1] * 0.5
    return p


# ------------------------------------------------------------------ 1. the kernels against the reference
@pytest.mark.parametrize("C", [2, 10, 25])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 1024])
def test_smc_init_w_categorical_kernel(dev, P, C):
    from clvae_amd import ops
    rng = np.random.default_rng(100 * C + P)
    G, seed, m0 = 7, 1234567890123, 11
    probs = _probs(rng, G, C)
    wr = torch.full((G * P, C), float('nan'), device=dev)
    ops.smc_init_w(G, P, C, ops.SMC_W_CATEGORICAL, seed, m0, torch.as_tensor(probs, device=dev), None, None, wr)
    torch.cuda.synchronize()
    want, keys = KR.init_categorical(probs, P, seed, m0)
    got = wr.cpu().numpy()
    assert np.array_equal(got, want)
    assert np.all(keys[0] == C // 2) and np.all(keys[1] == C - 1)
    counts = np.stack([np.bincount(k, minlength=C) for k in keys])
    assert np.all(counts[probs == 0] == 0) and np.all(np.abs(counts - P * probs) < 1 + 1e-9)


@pytest.mark.parametrize("P,C", [(1, 2), (63, 10), (64, 25), (65, 10), (1024, 10), (200, 32)])
def test_smc_init_w_logistic_normal_kernel(dev, P, C):
    """Bound: 16 ulp of 1.0.  The kernel's eps is the float32 Box-Muller draw; its angle 2 pi u is rounded to float32
    (|error| <= pi 2^-23 ~ 3.7e-7), which moves eps by up to radius * that (radius <= 5.8: 2.2e-6), and s = mean + sd * eps
    (|s| < 8, sd <= 1 here) adds two roundings of half an ulp of 8 (4.8e-7 each): |ds| <= 3.2e-6 in the worst case.  A
    softmax output moves by at most w (1 - w) |ds| <= |ds| / 4 = 0.8e-6, and expf, the sum and the division add about 4
    ulp of relative error to w <= 1 (0.5e-6): 1.3e-6 < 16 ulp = 1.9e-6.  Measured maximum on the MI355X over these cases:
    2.11e-7 (1.77 ulp, at P = 1024, C = 10)."""
    from clvae_amd import ops
    rng = np.random.default_rng(P + C)
    G, seed, m0 = 5, 99, 3
    mean = rng.uniform(-1, 1, (G, C - 1)).astype(np.float32)
    lv = rng.uniform(-3, 0, (G, C - 1)).astype(np.float32)
    mean[0], lv[0] = 0.0, 0.0                       # the model's own prior at w_log_var_prior = 0
    wr = torch.full((G * P, C), float('nan'), device=dev)
    ops.smc_init_w(G, P, C, ops.SMC_W_LOGISTIC_NORMAL, seed, m0, None, torch.as_tensor(mean, device=dev),
                   torch.as_tensor(lv, device=dev), wr)
    torch.cuda.synchronize()
    want = KR.init_logistic_normal(mean, lv, P, seed, m0)
    got = wr.cpu().numpy().astype(np.float64)
    err = np.abs(got - want).max()
    print("logistic-normal rows P=%d C=%d: max |w - fp64| = %.3e (%.2f ulp of 1.0)" % (P, C, err, err / ULP))
    assert err <= 16 * ULP
    assert np.abs(got.sum(axis=1) - 1).max() <= 4 * ULP * np.sqrt(C)


@pytest.mark.parametrize("P,C", [(1, 2), (5, 10), (64, 25), (100, 10), (1024, 10), (1000, 32)])
def test_smc_w_posterior_kernel(dev, P, C):
    from clvae_amd import ops
    rng = np.random.default_rng(7 * P + C)
    G, nsteps, S = 4, 5, 2
    lw = rng.standard_normal((G, P)) * 3
    lw -= np.log(np.exp(lw).sum(axis=1, keepdims=True))
    wr = rng.dirichlet(np.ones(C), G * P).astype(np.float32)
    wr[:P] = np.eye(C, dtype=np.float32)[rng.integers(0, C, P)]          # melody 0: one-hot rows
    t = lambda a: torch.as_tensor(a, device=dev)
    lw_d, wr_d = t(lw), t(wr)
    out = torch.full((G, nsteps, C), -7.0, dtype=torch.float64, device=dev)
    want = np.full((G, nsteps, C), -7.0)
    for c in (0, S - 1, S + nsteps):                  # a seed step, the bridge, past the end: the output is untouched
        ops.smc_w_posterior(G, P, C, nsteps, S, lw_d, wr_d, TG._counter(dev, c), out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    for k in (0, 3, nsteps - 1):
        ops.smc_w_posterior(G, P, C, nsteps, S, lw_d, wr_d, TG._counter(dev, S + k), out)
        want[:, k] = KR.w_posterior(lw, wr)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    untouched = np.ones(nsteps, bool)
    untouched[[0, 3, nsteps - 1]] = False
    assert np.all(got[:, untouched] == -7.0)
    np.testing.assert_allclose(got[:, ~untouched], want[:, ~untouched], rtol=1e-12, atol=0)
    np.testing.assert_allclose(got[:, 0].sum(axis=1), 1.0, rtol=0, atol=1e-6)      # float32 rows sum to 1 within rounding


@pytest.mark.parametrize("P,C,n_out", [(1, 2, 1), (5, 10, 3), (64, 25, 64), (1024, 10, 9)])
def test_smc_take_w_kernel(dev, P, C, n_out):
    from clvae_amd import ops
    rng = np.random.default_rng(P + n_out)
    G = 6
    wr = rng.standard_normal((G * P, C)).astype(np.float32)
    picks = rng.integers(0, P, (G, n_out)).astype(np.int32)
    picks[0, 0], picks[-1, -1] = 0, P - 1
    w_out = torch.full((G, n_out, C), float('nan'), device=dev)
    ops.smc_take_w(G, P, C, n_out, torch.as_tensor(picks, device=dev), torch.as_tensor(wr, device=dev), w_out)
    torch.cuda.synchronize()
    assert np.array_equal(w_out.cpu().numpy(), KR.take_w(wr, picks, P))


# ------------------------------------------------------------------ 2. the identities of the definition
def _prior_cases(N, C, rng):
    from clvae_amd.engine_generate import WPrior
    return {'categorical': WPrior.categorical(_probs(rng, N, C)),
            'logistic_normal': WPrior.logistic_normal(rng.uniform(-1, 1, (N, C - 1)), rng.uniform(-2, 0, (N, C - 1)))}


@pytest.mark.parametrize("S", [0, 3])
def test_one_hot_prior_is_the_fixed_label_filter_vrnn(dev, S):
    from clvae_amd.engine_generate import SmcKeyResult, SmcResult, WPrior
    eng, _ = TG._vrnn(dev)
    N, nsteps, P, seed = 5, 6, 8, 21 + S
    x_seed, w = TG._inputs(dev, N, S, 10, 1)
    roll = TG._roll(np.random.default_rng(2), N, nsteps, frac=0.2)
    kw = dict(resample_threshold=0.6, n_out=3, seed=seed)
    a = eng.generate_smc(x_seed, w, nsteps, roll, P, **kw)
    b = eng.generate_smc(x_seed, None, nsteps, roll, P, w_prior=WPrior.categorical(w.cpu().numpy()), **kw)
    torch.cuda.synchronize()
    assert type(a) is SmcResult and type(b) is SmcKeyResult
    assert int(a.resamples.sum()) > 0
    assert TG._same(a, b[:4])
    w_np = w.cpu().numpy().astype(np.float64)
    post = b.w_posterior.cpu().numpy()
    assert post.shape == (N, nsteps, 10) and np.all(post[w_np[:, None].repeat(nsteps, 1) == 0] == 0.0)
    np.testing.assert_allclose(post, w_np[:, None].repeat(nsteps, 1), rtol=0, atol=1e-12)
    assert torch.equal(b.w_out, w[:, None].repeat(1, 3, 1))


def test_one_hot_prior_is_the_fixed_label_filter_vae(dev):
    from clvae_amd.engine_generate import WPrior
    eng, _ = TG._vae(dev, B=16)                       # 6 melodies x 8 particles: chunks of two melodies
    N, nsteps, P, seed = 6, 7, 8, 13
    x_seed, w = TG._inputs(dev, N, None, 4, 3)
    roll = TG._roll(np.random.default_rng(4), N, nsteps, frac=0.2)
    kw = dict(resample_threshold=0.6, n_out=2, seed=seed)
    a = eng.generate_smc(x_seed, w, nsteps, roll, P, **kw)
    b = eng.generate_smc(x_seed, None, nsteps, roll, P, w_prior=WPrior.categorical(w.cpu().numpy()), **kw)
    torch.cuda.synchronize()
    assert int(a.resamples.sum()) > 0
    assert TG._same(a, b[:4])
    np.testing.assert_allclose(b.w_posterior.cpu().numpy(), w.cpu().numpy()[:, None].repeat(nsteps, 1), rtol=0, atol=1e-12)
    assert torch.equal(b.w_out, w[:, None].repeat(1, 2, 1))


def _rows_of(prior, P, seed, dev):
    """the particles' label rows [N * P, C] as the engine draws them (one chunk from melody 0)"""
    wr = torch.zeros(prior.N * P, prior.C, device=dev)
    prior.to(dev).init_rows(0, prior.N, P, seed, wr)
    return wr


def _check_tau_zero(r, ell_sum, wr, N, P):
    """identity 2: without resampling the posterior is the softmax-weighted mean of the rows by the accumulated
    increments.  ell_sum comes from the fp64 frame oracle, the filter's from float32 x_hat: they agree to rtol = atol =
    1e-4 (the margin of tests/test_gpu_smc.py for these sums).  Weights W_p = softmax(ell_sum) move by sum_p |dW_p| <=
    2 max |d ell_sum| and the rows lie in [0, 1], so each posterior entry moves by at most twice that."""
    assert int(r.resamples.sum()) == 0
    tol = 2 * (1e-4 + 1e-4 * np.abs(ell_sum).max())
    want = KR.posterior_from_increments(ell_sum.reshape(N, P), wr)
    got = r.w_posterior.cpu().numpy()[:, -1]
    print("tau = 0: max |w_posterior - softmax mean| = %.3e (bound %.3e)" % (np.abs(got - want).max(), tol))
    assert np.abs(got - want).max() <= tol
    np.testing.assert_allclose(r.log_evidence.cpu().numpy(),
                               np.log(np.exp(ell_sum.reshape(N, P)).mean(axis=1)), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("kind", ['categorical', 'logistic_normal'])
def test_tau_zero_posterior_is_the_softmax_of_the_increments_vrnn(dev, kind):
    eng, p = TG._vrnn(dev)
    N, S, nsteps, P, seed, L = 4, 2, 5, 8, 17, 2
    x_seed, _ = TG._inputs(dev, N, S, 10, 5)
    roll = TG._roll(np.random.default_rng(6), N, nsteps, frac=0.2)
    prior = _prior_cases(N, 10, np.random.default_rng(7))[kind]
    r = eng.generate_smc(x_seed, None, nsteps, roll, P, resample_threshold=0.0, seed=seed, w_prior=prior)
    wr = _rows_of(prior, P, seed, dev)
    # no resampling: the particles are independent rows, so plain clamped generation of the R rows walks the same paths
    xs_rep, roll_rep = x_seed.repeat_interleave(P, 0), np.repeat(roll, P, axis=0)
    paths = eng.generate(xs_rep, wr, nsteps, seed=seed, persistent=False, clamp=roll_rep)
    torch.cuda.synchronize()
    xs_np, w_np = xs_rep.cpu().numpy().astype(np.float64), wr.cpu().numpy().astype(np.float64)
    Xs = paths.cpu().numpy().astype(np.float64)
    xh_bridge = TG._vrnn_xhat_along(p, xs_np, w_np, seed, L)[:, S - 1]
    u = TG.OP.uniform(N * P * D, seed, step=S - 1, stream_id=1).reshape(N * P, D)
    bridge = (u <= xh_bridge.astype(np.float32)).astype(np.float64)[:, None]
    xh = TG._vrnn_xhat_along(p, np.concatenate([xs_np, bridge, Xs[:, :-1]], 1), w_np, seed, L)[:, S:]
    ell_sum = sum(SR.increment(xh[:, j], roll_rep[:, j]) for j in range(nsteps))
    _check_tau_zero(r, ell_sum, w_np, N, P)


@pytest.mark.parametrize("kind", ['categorical', 'logistic_normal'])
def test_tau_zero_posterior_is_the_softmax_of_the_increments_vae(dev, kind):
    eng, p = TG._vae(dev, B=32)
    N, nsteps, P, seed, L = 4, 6, 8, 19, 3
    x_seed, _ = TG._inputs(dev, N, None, 4, 7)
    roll = TG._roll(np.random.default_rng(8), N, nsteps, frac=0.2)
    prior = _prior_cases(N, 4, np.random.default_rng(9))[kind]
    r = eng.generate_smc(x_seed, None, nsteps, roll, P, resample_threshold=0.0, seed=seed, w_prior=prior)
    wr = _rows_of(prior, P, seed, dev)
    xs_rep, roll_rep = x_seed.repeat_interleave(P, 0), np.repeat(roll, P, axis=0)
    paths = eng.generate(xs_rep, wr, nsteps, seed=seed, persistent=False, clamp=roll_rep)
    torch.cuda.synchronize()
    w_np = wr.cpu().numpy().astype(np.float64)
    xh = TG._vae_xhat_along(p, xs_rep.cpu().numpy().astype(np.float64), paths.cpu().numpy().astype(np.float64), w_np, seed, L)
    ell_sum = sum(SR.increment(xh[:, t], roll_rep[:, t]) for t in range(nsteps))
    _check_tau_zero(r, ell_sum, w_np, N, P)


@pytest.mark.parametrize("kind", ['categorical', 'logistic_normal'])
def test_key_filter_graph_equals_eager_and_chunking_changes_nothing(dev, kind):
    rng = np.random.default_rng(7)
    ev, _ = TG._vrnn(dev)
    N, S, nsteps, P, seed = 6, 2, 6, 8, 31          # 48 rows: one GEMM tiling for every chunk
    x_seed, _ = TG._inputs(dev, N, S, 10, 8)
    roll = TG._roll(rng, N, nsteps, frac=0.2)
    prior = _prior_cases(N, 10, rng)[kind]
    kw = dict(resample_threshold=0.6, n_out=3, seed=seed, w_prior=prior)
    a = ev.generate_smc(x_seed, None, nsteps, roll, P, **kw)
    b = ev.generate_smc(x_seed, None, nsteps, roll, P, use_graph=False, **kw)
    c = ev.generate_smc(x_seed, None, nsteps, roll, P, chunk=4, **kw)
    d = ev.generate_smc(x_seed, None, nsteps, roll, P, chunk=1, **kw)
    torch.cuda.synchronize()
    assert int(a.resamples.sum()) > 0 and len(a) == 6
    assert TG._same(a, b) and TG._same(a, c) and TG._same(a, d)
    np.testing.assert_allclose(a.w_posterior.cpu().numpy().sum(axis=2), 1.0, rtol=0, atol=1e-5)
    # cl_vae: the engine's batch size forces the chunks
    va, _ = TG._vae(dev, B=48)
    vb, _ = TG._vae(dev, B=16)
    x1, _ = TG._inputs(dev, N, None, 4, 9)
    roll = TG._roll(rng, N, nsteps, frac=0.2)
    kw['w_prior'] = _prior_cases(N, 4, rng)[kind]
    a = va.generate_smc(x1, None, nsteps, roll, P, **kw)
    b = va.generate_smc(x1, None, nsteps, roll, P, use_graph=False, **kw)
    c = vb.generate_smc(x1, None, nsteps, roll, P, **kw)
    torch.cuda.synchronize()
    assert int(a.resamples.sum()) > 0
    assert TG._same(a, b) and TG._same(a, c)


def test_key_filter_value_errors(dev):
    from clvae_amd.engine_generate import WPrior
    eng, _ = TG._vrnn(dev)
    N, nsteps = 3, 4
    x_seed, w = TG._inputs(dev, N, 2, 10, 1)
    roll = np.full((N, nsteps, D), FREE, np.uint8)
    for kw in (dict(w=None), dict(w=w, w_prior=WPrior.uniform(N, 10)), dict(w=None, w_prior=WPrior.uniform(N + 1, 10)),
               dict(w=None, w_prior=WPrior.uniform(N, 9)), dict(w=None, w_prior=np.full((N, 10), 0.1))):
        with pytest.raises(ValueError):
            eng.generate_smc(x_seed, kw.pop('w'), nsteps, roll, 4, **kw)


# ------------------------------------------------------------------ 3. exactness on an enumerable model
T4 = TG.T4
ROLL01 = TG.ROLL01
KEYS_VRNN = (1, 4, 7)            # the classes whose decoder rows are set; the prior is uniform over them
KEYS_VAE = (0, 2, 3)


def enumerable_vrnn_params():
    """TG._enumerable_vrnn with decoder rows of w for three classes: the candidate of unit 0 is tanh(3 x0_prev + a_c) and
    that of unit 1 tanh(x1_prev + b_c), so p(note 1) = sigmoid(10 tanh(tanh(3 x0_prev + a_c)) - 4) depends on the key"""
    cfg = O.vrnn_config(latent_dim=2, seq_length=8, n_classes=10, use_x_prev=True, gate_act='hard_sigmoid')
    p = {k: np.asarray(v, np.float32) for k, v in O.vrnn_init_params(cfg, seed=3).items()}
    H, L = 88, 2
    K = np.zeros_like(p['decoder_h/kernel'])              # rows [x_prev (88), z (2), w (10)]
    K[0, 2 * H + 0] = 3.0
    K[1, 2 * H + 1] = 1.0
    for c, a, b_ in zip(KEYS_VRNN, (0.0, 0.1, -0.1), (0.0, -1.0, 1.0)):
        K[D + L + c, 2 * H + 0] = a
        K[D + L + c, 2 * H + 1] = b_
    b = np.zeros(4 * H, np.float32)
    b[:H], b[H:2 * H], b[3 * H:] = 5.0, -5.0, 5.0           # i = 1, f = 0, o = 1: no memory beyond the last frame
    p['decoder_h/kernel'], p['decoder_h/bias'] = K, b
    p['decoder_h/recurrent_kernel'] = np.zeros_like(p['decoder_h/recurrent_kernel'])
    Wo = np.zeros_like(p['X_decoded_mean/kernel'])
    Wo[0, 1], Wo[1, 0] = 10.0, 0.3 / np.tanh(np.tanh(1.0))
    bo = np.full(D, -40.0, np.float32)
    bo[0], bo[1] = 0.0, -4.0
    p['X_decoded_mean/kernel'], p['X_decoded_mean/bias'] = Wo.astype(np.float32), bo
    return cfg, p


def enumerable_vae_params():
    """TG._enumerable_vae with decoder rows of w for three classes: p(note 1 at t) = sigmoid(2 relu(4 x0(t-2) + a_c) - 4)"""
    cfg = O.vae_config(latent_dim=3, n_classes=4, use_x_prev=True)
    p = {k: np.asarray(v, np.float32) for k, v in O.vae_init_params(cfg, seed=4).items()}
    K = np.zeros_like(p['decoder_h/kernel'])              # rows [w (4), history (88), z (3)]
    K[4 + 0, 0] = 4.0
    K[4 + 1, 1] = 1.0
    for c, a, b_ in zip(KEYS_VAE, (0.0, 0.5, -0.5), (0.0, 2.0, 0.5)):
        K[c, 0] = a
        K[c, 1] = b_
    p['decoder_h/kernel'], p['decoder_h/bias'] = K, np.zeros_like(p['decoder_h/bias'])
    Wo = np.zeros_like(p['x_decoded_mean/kernel'])
    Wo[0, 1], Wo[1, 0] = 2.0, 0.4
    bo = np.full(D, -40.0, np.float32)
    bo[0], bo[1] = 0.0, -4.0
    p['x_decoded_mean/kernel'], p['x_decoded_mean/bias'] = Wo, bo
    return cfg, p


def vrnn_xhat_of(p):
    def xhat_of(frames, key):
        n = frames.shape[0]
        inputs = np.concatenate([np.zeros((n, 1, D)), frames[:, :-1]], 1)
        return TG._vrnn_xhat_along(p, inputs, np.eye(10)[np.full(n, key)], 0, 2)
    return xhat_of


def vae_xhat_of(p):
    def xhat_of(frames, key):
        n = frames.shape[0]
        return TG._vae_xhat_along(p, np.zeros((n, D)), frames, np.eye(4)[np.full(n, key)], 0, 3)
    return xhat_of


def exact_joint(xhat_of, keys):
    """p(constraints, key = c) for the uniform prior over `keys`, by enumerating 3 keys x 4^T4 histories of notes 0 / 1
    with the fp64 forward xhat_of(frames, key)"""
    hs = np.array(list(itertools.product((0.0, 1.0), repeat=2 * T4))).reshape(-1, T4, 2)
    frames = np.zeros((len(hs), T4, D))
    frames[:, :, :2] = hs
    clamped = ROLL01 <= 1
    consistent = np.all(~clamped[None] | (hs == ROLL01[None]), axis=(1, 2))
    joint = []
    for c in keys:
        xh = xhat_of(frames, c)[:, :, :2]
        bern = np.where(hs == 1, xh, 1 - xh)
        joint.append((np.prod(bern, axis=(1, 2)) * consistent).sum() / len(keys))
    return np.array(joint)


def key_prior(keys, G, C):
    probs = np.zeros((G, C))
    probs[:, list(keys)] = 1.0 / len(keys)
    return probs


def check_key_exactness(joint, keys, C, logZ, post_last, w_out, Xs):
    """the two comparisons of tests/test_smc_key_reference.py at 4 standard errors, the power assertion,
    and that every returned path carries one of the keys and satisfies the roll"""
    keys = list(keys)
    G = len(logZ)
    Z = joint.sum()
    post = joint / Z
    assert np.abs(post - 1.0 / len(keys)).max() >= 0.2, post     # a filter that ignored the weights would report the prior
    others = [c for c in range(C) if c not in keys]
    assert np.all(post_last[:, others] == 0.0)
    est, se, ratio, se_r = KR.pooled_estimates(logZ, post_last[:, keys], logZ_scale=np.log(Z))
    print("joint / Z: estimate %s exact %s se %s" % (est, post, se))
    print("pooled posterior: estimate %s exact %s se %s" % (ratio, post, se_r))
    assert np.all(np.abs(est - post) < 4 * se + 1e-12), (est, post, se)
    assert np.all(np.abs(ratio - post) < 4 * se_r + 1e-12), (ratio, post, se_r)
    r = np.exp(logZ - np.log(Z))
    assert abs(r.mean() - 1) < 4 * r.std() / np.sqrt(G) + 1e-9, (r.mean(), r.std())
    assert np.all(np.sort(w_out, axis=-1)[..., :-1] == 0.0) and np.all(w_out.max(axis=-1) == 1.0)       # one-hot rows
    assert set(np.unique(np.argmax(w_out, axis=-1))) <= set(keys)
    free = ROLL01 > 1
    assert np.all(Xs[:, :, 2:] == 0) and np.all(Xs[:, :, :2][:, ~free] == ROLL01[~free])


def _run_exactness(gen, xhat_of, keys, C, G=256, P=64):
    roll = np.full((G, T4, D), FREE, np.uint8)
    roll[:, :, :2] = ROLL01
    r = gen(roll, P, key_prior(keys, G, C))
    torch.cuda.synchronize()
    check_key_exactness(exact_joint(xhat_of, keys), keys, C, r.log_evidence.cpu().numpy(),
                        r.w_posterior.cpu().numpy()[:, -1], r.w_out[:, 0].cpu().numpy(), r.Xs[:, 0].cpu().numpy())


def test_exact_key_posterior_on_enumerable_vrnn(dev):
    from clvae_amd.engine import VrnnEngine
    from clvae_amd.engine_generate import WPrior
    cfg, p = enumerable_vrnn_params()
    eng = VrnnEngine(cfg, 4, dev)
    eng.P.set_weights(p)
    G = 256
    x_seed = torch.zeros(G, 0, D, device=dev)
    gen = lambda roll, P, probs: eng.generate_smc(x_seed, None, T4, roll, P, seed=41, w_prior=WPrior.categorical(probs))
    _run_exactness(gen, vrnn_xhat_of(p), KEYS_VRNN, 10, G=G)


def test_exact_key_posterior_on_enumerable_vae(dev):
    from clvae_amd.engine import VaeEngine
    from clvae_amd.engine_generate import WPrior
    cfg, p = enumerable_vae_params()
    eng = VaeEngine(cfg, 4096, dev)                       # 256 x 64 rows: four chunks
    eng.P.set_weights(p)
    G = 256
    x_seed = torch.zeros(G, D, device=dev)
    gen = lambda roll, P, probs: eng.generate_smc(x_seed, None, T4, roll, P, seed=43, w_prior=WPrior.categorical(probs))
    _run_exactness(gen, vae_xhat_of(p), KEYS_VAE, 4, G=G)


# ------------------------------------------------------------------ 4. the sample CLIs with --infer_key
@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_infer_key_cli_end_to_end(dev, tmp_path, capsys, monkeypatch, which):
    import importlib
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, HARMONIZE_FLAGS, parser_for
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    TR = importlib.import_module('clvae_amd.%s.train' % which)
    data = make_synthetic_pickle(str(tmp_path / "syn.pickle"), n_songs=(10, 4, 4), seed=1)
    mdir, sdir = str(tmp_path / "models"), str(tmp_path / "samples")
    os.makedirs(mdir); os.makedirs(sdir)
    extra = ['--latent_dim', '4', '--batch_size', '50'] if which == 'cl_vae' else ['--seq_length', '8', '--batch_size', '20']
    np.random.seed(0)
    TR.train(TR.build_parser().parse_args(['m', '--use_x_prev', '--num_epochs', '2', '--patience', '0', '--train_file', data,
                                           '--model_dir', mdir] + extra))
    parser = parser_for('%s.sample' % which, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS)
    common = ['h', '-n', '3', '-t', '8', '--seed', '4', '-i', os.path.join(mdir, 'm.h5'), '--train_file', data,
              '--sample_dir', sdir]
    with pytest.raises(SystemExit):
        parser.parse_args(common + ['--harmonize', 'top', '--infer_key', 'discrete'])
    for mode in ('discrete', 'continuous'):
        args = parser.parse_args(common + ['--harmonize', 'top', '--particles', '8', '--infer_key', mode])
        seen = []
        real = S.print_key_posterior

        def spy(names, w_posterior, key_map):
            seen.append((np.asarray(w_posterior), dict(key_map)))
            return real(names, w_posterior, key_map)
        monkeypatch.setattr(S, 'print_key_posterior', spy)
        np.random.seed(3)
        capsys.readouterr()
        rolls = S.sample(args)
        printed = capsys.readouterr().out.splitlines()
        monkeypatch.setattr(S, 'print_key_posterior', real)
        assert len(rolls) == 3 and all(set(np.unique(r)) <= {0.0, 1.0} for r in rolls)
        assert sum('log p(voice) per frame' in line for line in printed) == 3
        lines = [line for line in printed if ': key posterior ' in line]
        assert len(lines) == 3 and len(seen) == 1
        post, key_map = seen[0]
        assert post.shape == (3, 8, len(key_map)) and post.dtype == np.float64 and np.all(post >= 0)
        tol = 1e-9 if mode == 'discrete' else 1e-5           # float32 softmax rows sum to 1 within their rounding only
        assert np.abs(post.sum(axis=2) - 1).max() < tol
        for line, q in zip(lines, post[:, -1]):             # every key named, most probable first
            pairs = [kv.split('=') for kv in line.split(': key posterior ')[1].split()]
            assert sorted(k for k, _ in pairs) == sorted(key_map)
            vals = [float(v) for _, v in pairs]
            assert vals == sorted(vals, reverse=True) and abs(vals[0] - q.max()) < 1e-4
