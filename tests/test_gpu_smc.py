"""-m gpu: particle-filter sampling under a constraint roll: the four kernels of csrc/smc.hip against the
fp64 reference (tests/smc_reference.py), the frame chains of both engines around them, and exactness on a model whose
histories can be enumerated."""
import itertools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import smc_reference as SR
from helpers import make_synthetic_pickle
from oracle import clvae_oracle as O
from oracle import philox as OP

pytestmark = pytest.mark.gpu

FREE = 255
D = 88


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _counter(dev, c):
    return torch.full((1,), c, dtype=torch.int32, device=dev)


def _roll(rng, N, nsteps, frac=0.3, on=0.3):
    r = rng.random((N, nsteps, D))
    return np.where(r < frac, (r < frac * on).astype(np.uint8), np.uint8(FREE)).astype(np.uint8)


# ------------------------------------------------------------------ 1. the kernels against the reference
def test_smc_sample_kernel(dev):
    from clvae_amd import ops
    rng = np.random.default_rng(0)
    G, P, nsteps, S = 6, 7, 3, 2
    R = G * P
    xhat = rng.random((R, D)).astype(np.float32)
    special = np.array([0.0, 1.0, 1e-7, np.float32(1) - np.float32(1e-7), 1e-9, 1 - 1e-9, 5e-8, 0.5], np.float32)
    xhat[:, :len(special)] = special
    u = rng.random((R, D)).astype(np.float32)
    roll = _roll(rng, G, nsteps, frac=0.5)
    roll[0] = FREE                                    # melody 0 all free
    roll[1] = (rng.random((nsteps, D)) < 0.5)         # melody 1 fully clamped
    roll[2, :, :len(special)] = 1
    roll[3, :, :len(special)] = 0
    t = lambda a: torch.as_tensor(a, device=dev)
    p_d, u_d, c_d = t(xhat), t(u), t(roll)
    for k in (1, -1, nsteps):                         # a returned step, the bridge, past the end
        x = torch.full((R, D), float('nan'), device=dev)
        ell = torch.full((R,), float('nan'), dtype=torch.float64, device=dev)
        hist = torch.full((nsteps, R, D), 7, dtype=torch.uint8, device=dev)
        ops.smc_sample(R, D, P, nsteps, S, p_d, u_d, c_d, _counter(dev, S + k), x, ell, hist)
        torch.cuda.synchronize()
        if 0 <= k < nsteps:
            rows = np.repeat(roll[:, k], P, axis=0)
            want = SR.sample_frame(xhat, u, rows)
            assert np.array_equal(x.cpu().numpy(), want)
            np.testing.assert_allclose(ell.cpu().numpy(), SR.increment(xhat, rows), rtol=1e-12, atol=0)
            assert np.all(ell.cpu().numpy()[:P] == 0.0)
            h = hist.cpu().numpy()
            assert np.array_equal(h[k], want.astype(np.uint8))
            assert np.all(np.delete(h, k, axis=0) == 7)
        else:                                         # no constraint, no weight, no history
            assert np.array_equal(x.cpu().numpy(), (u <= xhat).astype(np.float32))
            assert torch.isnan(ell).all() and bool((hist == 7).all())


@pytest.mark.parametrize("G,P,tau", [(5, 1, 0.5), (4, 5, 0.5), (3, 64, 0.7), (3, 100, 1.0), (2, 33, 0.0), (1, 1024, 0.5)])
def test_smc_resample_kernel(dev, G, P, tau):
    from clvae_amd import ops
    rng = np.random.default_rng(P)
    nsteps, S, seed, m0 = 12, 3, 77, 5
    R = G * P
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    ell, logW = torch.zeros(R, **f64), torch.full((R,), float('nan'), **f64)
    logZ, ess = torch.full((G,), float('nan'), **f64), torch.zeros(G, nsteps, **f64)
    nres, flag, anc = torch.full((G,), -5, **i32), torch.zeros(G, **i32), torch.full((nsteps, R), -1, **i32)
    ref = SR.Filter(G, P, nsteps, tau, seed, m0)
    for k in range(nsteps):
        scale = [0.0, 0.3, 3.0][k % 3]
        e = -np.abs(rng.standard_normal(R)) * scale - rng.random(R) * 2 * (k % 2)
        ell.copy_(torch.as_tensor(e, device=dev))
        ops.smc_resample(G, P, nsteps, S, seed, m0, tau, ell, logW, logZ, ess, nres, flag, anc, _counter(dev, S + k))
        ref.step(e, S + k, k)
        torch.cuda.synchronize()
        np.testing.assert_allclose(logZ.cpu().numpy(), ref.logZ, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(logW.cpu().numpy(), ref.logW.reshape(-1), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(ess[:, k].cpu().numpy(), ref.ess[:, k], rtol=1e-12)
        assert np.array_equal(flag.cpu().numpy().astype(bool), ref.resampled[k])
        a = anc[k].cpu().numpy()
        assert not ref.near[k].any()                      # no draw of this test sits within 1e-9 P of a grid point
        assert np.array_equal(a, ref.anc[k]), (k, np.argwhere(a != ref.anc[k])[:4])
    assert np.array_equal(nres.cpu().numpy(), ref.nres)
    if tau == 0.0:
        assert ref.nres.sum() == 0
    elif P > 1:
        assert ref.nres.sum() > 0
    # steps outside [S, S + nsteps) change nothing
    before = [t.clone() for t in (logW, logZ, ess, nres, anc)]
    for c in (S - 1, S + nsteps):
        ops.smc_resample(G, P, nsteps, S, seed, m0, tau, ell, logW, logZ, ess, nres, flag, anc, _counter(dev, c))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (logW, logZ, ess, nres, anc)))


def test_smc_gather_kernel(dev):
    from clvae_amd import ops
    rng = np.random.default_rng(3)
    G, P, nsteps, S, k = 5, 6, 4, 1, 2
    R = G * P
    widths = [88, 352, 7]
    bufs = [torch.as_tensor(rng.standard_normal((R, w)).astype(np.float32), device=dev) for w in widths]
    orig = [b.cpu().numpy() for b in bufs]
    anc_np = np.tile(np.arange(R, dtype=np.int32), (nsteps, 1))
    anc_np[k] = (np.arange(R) // P * P + rng.integers(0, P, R)).astype(np.int32)
    flag_np = np.array([1, 0, 1, 1, 0], np.int32)
    anc, flag = torch.as_tensor(anc_np, device=dev), torch.as_tensor(flag_np, device=dev)
    gather = ops.SmcGather(R, P, nsteps, S, bufs)
    gather(anc, flag, _counter(dev, S + k))
    torch.cuda.synchronize()
    moved = np.repeat(flag_np, P).astype(bool)
    for b, o in zip(bufs, orig):
        want = np.where(moved[:, None], o[anc_np[k]], o)
        assert np.array_equal(b.cpu().numpy(), want)
    # a step outside the returned range moves nothing
    snap = [b.clone() for b in bufs]
    gather(anc, flag, _counter(dev, S - 1))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(snap, bufs))


@pytest.mark.parametrize("P,n_out", [(1, 1), (5, 3), (64, 64), (200, 9)])
def test_smc_backtrack_kernel(dev, P, n_out):
    from clvae_amd import ops
    rng = np.random.default_rng(P + n_out)
    G, nsteps, seed, m0 = 4, 6, 123, 9
    R = G * P
    lw = rng.standard_normal((G, P)) * 1.5
    lw -= np.log(np.exp(lw).sum(axis=1, keepdims=True))
    anc = (np.arange(R)[None] // P * P + rng.integers(0, P, (nsteps, R))).astype(np.int32)
    hist = (rng.random((nsteps, R, D)) < 0.3).astype(np.uint8)
    Xs = torch.full((G, n_out, nsteps, D), float('nan'), device=dev)
    picks = torch.full((G, n_out), -1, dtype=torch.int32, device=dev)
    t = lambda a: torch.as_tensor(a, device=dev)
    ops.smc_backtrack(G, P, nsteps, D, n_out, seed, m0, 50, t(lw), t(anc), t(hist), Xs, picks)
    torch.cuda.synchronize()
    want, wp = SR.backtrack(lw, anc, hist, n_out, seed, 50, m0)
    assert np.array_equal(picks.cpu().numpy(), wp)
    assert np.array_equal(Xs.cpu().numpy(), want)


# ------------------------------------------------------------------ engines and fp64 frame oracles
def _vrnn(dev, L=2, B=4, seed=5):
    from clvae_amd.engine import VrnnEngine
    cfg = O.vrnn_config(latent_dim=L, seq_length=8, n_classes=10, use_x_prev=True, gate_act='hard_sigmoid')
    rng = np.random.default_rng(L)
    p = {k: np.asarray(v, np.float32) for k, v in O.vrnn_init_params(cfg, seed=seed).items()}
    for k in p:
        if not k.startswith('hW'):
            p[k] = (p[k] + 0.15 * rng.standard_normal(p[k].shape)).astype(np.float32)
    eng = VrnnEngine(cfg, B, dev)
    eng.P.set_weights(p)
    return eng, p


def _vae(dev, L=3, C=4, B=8):
    from clvae_amd.engine import VaeEngine
    cfg = O.vae_config(latent_dim=L, n_classes=C, use_x_prev=True)
    rng = np.random.default_rng(L + C)
    p = {k: np.asarray(v, np.float32) for k, v in O.vae_init_params(cfg, seed=6).items()}
    for k in p:
        p[k] = (p[k] + 0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    p['x_decoded_mean/bias'] = (p['x_decoded_mean/bias'] - 2.0).astype(np.float32)
    eng = VaeEngine(cfg, B, dev)
    eng.P.set_weights(p)
    return eng, p


def _inputs(dev, N, S, C, seed):
    rng = np.random.default_rng(seed)
    shape = (N, S, D) if S is not None else (N, D)
    x_seed = torch.as_tensor((rng.random(shape) < 0.06).astype(np.float32), device=dev)
    w = torch.as_tensor(np.eye(C, dtype=np.float32)[rng.integers(0, C, N)], device=dev)
    return x_seed, w


def _cell(x, h, c, k, r, b, H=88):
    zz = x @ k + b + h @ r
    i, f_, g, o = O.hard_sigmoid(zz[:, :H]), O.hard_sigmoid(zz[:, H:2 * H]), np.tanh(zz[:, 2 * H:3 * H]), \
        O.hard_sigmoid(zz[:, 3 * H:])
    c = f_ * c + i * g
    return o * np.tanh(c), c


def _vrnn_xhat_along(p, inputs, w, seed, L):
    """fp64 x_hat of every step of cl_vrnn given the input frame of each step, inputs [N,T,D] (the seed frames, then each
    step's sample); z from the Philox eps of step t at row n"""
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    N = inputs.shape[0]
    H = 88
    he, ce, hd, cd = (np.zeros((N, H)) for _ in range(4))
    out = []
    for t in range(inputs.shape[1]):
        x_prev = inputs[:, t]
        he, ce = _cell(np.concatenate([x_prev, w], 1), he, ce, p['encoder_h/kernel'], p['encoder_h/recurrent_kernel'],
                       p['encoder_h/bias'])
        zm = he @ p['Z_mean/kernel'] + p['Z_mean/bias']
        zlv = he @ p['Z_log_var/kernel'] + p['Z_log_var/bias']
        eps = OP.normal(N * L, seed, step=t, stream_id=0).reshape(N, L).astype(np.float64)
        z = zm + np.exp(zlv / 2) * eps
        hd, cd = _cell(np.concatenate([x_prev, z, w], 1), hd, cd, p['decoder_h/kernel'], p['decoder_h/recurrent_kernel'],
                       p['decoder_h/bias'])
        out.append(O.sigmoid(hd @ p['X_decoded_mean/kernel'] + p['X_decoded_mean/bias']))
    return np.stack(out, axis=1)


def _vae_xhat_along(p, seeds, frames, w, seed, L):
    """fp64 x_hat of every frame of cl_vae fed its own frames [N,T,D]: encoder on frame t-1, decoder history frame t-2"""
    p = {k: np.asarray(v, np.float64) for k, v in p.items()}
    N, T = frames.shape[:2]
    x_in, hist, out = seeds, seeds, []
    for t in range(T):
        h = O.relu(np.concatenate([x_in, w], 1) @ p['h/kernel'] + p['h/bias'])
        zm, zlv = h @ p['z_mean/kernel'] + p['z_mean/bias'], h @ p['z_log_var/kernel'] + p['z_log_var/bias']
        eps = OP.normal(N * L, seed, step=t, stream_id=0).reshape(N, L).astype(np.float64)
        z = zm + np.exp(zlv / 2) * eps
        hd = O.relu(np.concatenate([w, hist, z], 1) @ p['decoder_h/kernel'] + p['decoder_h/bias'])
        out.append(O.sigmoid(hd @ p['x_decoded_mean/kernel'] + p['x_decoded_mean/bias']))
        hist, x_in = x_in, frames[:, t]
    return np.stack(out, axis=1)


# ------------------------------------------------------------------ 2. P = 1 is clamped frame-chain generation
def test_one_particle_equals_clamped_generation_vrnn(dev):
    eng, p = _vrnn(dev)
    N, S, nsteps, seed, L = 5, 3, 7, 21, 2
    x_seed, w = _inputs(dev, N, S, 10, 1)
    roll = _roll(np.random.default_rng(2), N, nsteps)
    ref = eng.generate(x_seed, w, nsteps, seed=seed, persistent=False, clamp=roll)
    r = eng.generate_smc(x_seed, w, nsteps, roll, 1, seed=seed)
    torch.cuda.synchronize()
    assert torch.equal(r.Xs[:, 0], ref)
    assert int(r.resamples.sum()) == 0 and bool((r.ess == 1.0).all())
    # log Z = sum of l along the returned path; the unreturned bridge sample is redrawn from its uniform
    xs_np, w_np = x_seed.cpu().numpy().astype(np.float64), w.cpu().numpy().astype(np.float64)
    Xs = r.Xs[:, 0].cpu().numpy().astype(np.float64)
    xh_bridge = _vrnn_xhat_along(p, xs_np, w_np, seed, L)[:, S - 1]
    u = OP.uniform(N * D, seed, step=S - 1, stream_id=1).reshape(N, D)
    bridge = (u <= xh_bridge.astype(np.float32)).astype(np.float64)[:, None]
    xh = _vrnn_xhat_along(p, np.concatenate([xs_np, bridge, Xs[:, :-1]], 1), w_np, seed, L)[:, S:]
    want = sum(SR.increment(xh[:, j], roll[:, j]) for j in range(nsteps))
    np.testing.assert_allclose(r.log_evidence.cpu().numpy(), want, rtol=1e-4, atol=1e-4)


def test_one_particle_equals_clamped_generation_vae(dev):
    eng, p = _vae(dev)
    N, nsteps, seed, L = 6, 8, 13, 3
    x_seed, w = _inputs(dev, N, None, 4, 3)
    roll = _roll(np.random.default_rng(4), N, nsteps)
    ref = eng.generate(x_seed, w, nsteps, seed=seed, persistent=False, clamp=roll)
    r = eng.generate_smc(x_seed, w, nsteps, roll, 1, seed=seed)
    torch.cuda.synchronize()
    assert torch.equal(r.Xs[:, 0], ref)
    Xs = r.Xs[:, 0].cpu().numpy().astype(np.float64)
    xh = _vae_xhat_along(p, x_seed.cpu().numpy().astype(np.float64), Xs, w.cpu().numpy().astype(np.float64), seed, L)
    want = sum(SR.increment(xh[:, t], roll[:, t]) for t in range(nsteps))
    np.testing.assert_allclose(r.log_evidence.cpu().numpy(), want, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------ 3. all-free rolls, graph against eager, chunking
def test_all_free_particles_are_plain_generation_vrnn(dev):
    eng, _ = _vrnn(dev)
    N, S, nsteps, seed, P = 4, 2, 6, 8, 8
    x_seed, w = _inputs(dev, N, S, 10, 5)
    free = np.full((N, nsteps, D), FREE, np.uint8)
    plain = eng.generate(x_seed.repeat_interleave(P, 0), w.repeat_interleave(P, 0), nsteps, seed=seed, persistent=False)
    r = eng.generate_smc(x_seed, w, nsteps, free, P, resample_threshold=1.0, n_out=P, seed=seed)
    torch.cuda.synchronize()
    assert torch.equal(r.Xs.reshape(N * P, nsteps, D), plain)
    assert bool((r.log_evidence == 0).all()) and int(r.resamples.sum()) == 0 and bool((r.ess == P).all())


def test_all_free_particles_are_plain_generation_vae(dev):
    eng, _ = _vae(dev, B=32)
    N, nsteps, seed, P = 4, 7, 9, 8
    x_seed, w = _inputs(dev, N, None, 4, 6)
    free = np.full((N, nsteps, D), FREE, np.uint8)
    plain = eng.generate(x_seed.repeat_interleave(P, 0), w.repeat_interleave(P, 0), nsteps, seed=seed, persistent=False)
    r = eng.generate_smc(x_seed, w, nsteps, free, P, resample_threshold=1.0, n_out=P, seed=seed, chunk=1)
    torch.cuda.synchronize()
    assert torch.equal(r.Xs.reshape(N * P, nsteps, D), plain)
    assert bool((r.log_evidence == 0).all()) and int(r.resamples.sum()) == 0


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_graph_equals_eager_and_chunking_changes_nothing(dev):
    rng = np.random.default_rng(7)
    ev, _ = _vrnn(dev)
    N, S, nsteps, P, seed = 6, 2, 6, 8, 31          # 48 rows: one GEMM tiling for every chunk
    x_seed, w = _inputs(dev, N, S, 10, 8)
    roll = _roll(rng, N, nsteps, frac=0.2)
    kw = dict(resample_threshold=0.6, n_out=3, seed=seed)
    a = ev.generate_smc(x_seed, w, nsteps, roll, P, **kw)
    b = ev.generate_smc(x_seed, w, nsteps, roll, P, use_graph=False, **kw)
    c = ev.generate_smc(x_seed, w, nsteps, roll, P, chunk=4, **kw)
    d = ev.generate_smc(x_seed, w, nsteps, roll, P, chunk=1, **kw)
    torch.cuda.synchronize()
    assert int(a.resamples.sum()) > 0
    assert _same(a, b) and _same(a, c) and _same(a, d)
    # cl_vae: the engine's batch size forces the chunks
    va, _ = _vae(dev, B=48)
    vb, _ = _vae(dev, B=16)
    x1, w1 = _inputs(dev, N, None, 4, 9)
    roll = _roll(rng, N, nsteps, frac=0.2)
    a = va.generate_smc(x1, w1, nsteps, roll, P, **kw)
    b = va.generate_smc(x1, w1, nsteps, roll, P, use_graph=False, **kw)
    c = vb.generate_smc(x1, w1, nsteps, roll, P, **kw)
    torch.cuda.synchronize()
    assert int(a.resamples.sum()) > 0
    assert _same(a, b) and _same(a, c)


# ------------------------------------------------------------------ 4. exactness on an enumerable model
T4 = 4
# notes 0 / 1 per frame: note 1 is steered by note 0 of an earlier frame; forcing it later pulls note 0 earlier up
ROLL01 = np.array([[FREE, FREE], [FREE, 1], [0, 1], [FREE, 1]], np.uint8)


def _enumerable_vrnn(dev, B):
    """cl_vrnn whose z rows are zero and whose notes 2..87 never sound: x_hat depends on the previous frame only,
    p(note 1) = sigmoid(10 tanh(tanh(3 x0_prev)) - 4), p(note 0) = sigmoid(0.3 x1_prev)"""
    from clvae_amd.engine import VrnnEngine
    cfg = O.vrnn_config(latent_dim=2, seq_length=8, n_classes=10, use_x_prev=True, gate_act='hard_sigmoid')
    p = {k: np.asarray(v, np.float32) for k, v in O.vrnn_init_params(cfg, seed=3).items()}
    H = 88
    K = np.zeros_like(p['decoder_h/kernel'])
    K[0, 2 * H + 0] = 3.0
    K[1, 2 * H + 1] = 1.0
    b = np.zeros(4 * H, np.float32)
    b[:H], b[H:2 * H], b[3 * H:] = 5.0, -5.0, 5.0           # i = 1, f = 0, o = 1: no memory beyond the last frame
    p['decoder_h/kernel'], p['decoder_h/bias'] = K, b
    p['decoder_h/recurrent_kernel'] = np.zeros_like(p['decoder_h/recurrent_kernel'])
    Wo = np.zeros_like(p['X_decoded_mean/kernel'])
    Wo[0, 1], Wo[1, 0] = 10.0, 0.3 / np.tanh(np.tanh(1.0))
    bo = np.full(D, -40.0, np.float32)
    bo[0], bo[1] = 0.0, -4.0
    p['X_decoded_mean/kernel'], p['X_decoded_mean/bias'] = Wo.astype(np.float32), bo
    eng = VrnnEngine(cfg, B, dev)
    eng.P.set_weights(p)
    return eng, p


def _enumerable_vae(dev, B):
    """cl_vae whose z rows are zero and whose notes 2..87 never sound: p(note 1 at t) = sigmoid(8 x0(t-2) - 4)"""
    from clvae_amd.engine import VaeEngine
    cfg = O.vae_config(latent_dim=3, n_classes=4, use_x_prev=True)
    p = {k: np.asarray(v, np.float32) for k, v in O.vae_init_params(cfg, seed=4).items()}
    K = np.zeros_like(p['decoder_h/kernel'])              # rows [w (4), history (88), z (3)]
    K[4 + 0, 0] = 4.0
    K[4 + 1, 1] = 1.0
    p['decoder_h/kernel'], p['decoder_h/bias'] = K, np.zeros_like(p['decoder_h/bias'])
    Wo = np.zeros_like(p['x_decoded_mean/kernel'])
    Wo[0, 1], Wo[1, 0] = 2.0, 0.4
    bo = np.full(D, -40.0, np.float32)
    bo[0], bo[1] = 0.0, -4.0
    p['x_decoded_mean/kernel'], p['x_decoded_mean/bias'] = Wo, bo
    eng = VaeEngine(cfg, B, dev)
    eng.P.set_weights(p)
    return eng, p


def _exact(xhat_of):
    """enumerate the 4^T4 histories of notes 0 / 1: p(constraints), exact posterior and clamped-ancestral marginals [T4,2]"""
    hs = np.array(list(itertools.product((0.0, 1.0), repeat=2 * T4))).reshape(-1, T4, 2)
    frames = np.zeros((len(hs), T4, D))
    frames[:, :, :2] = hs
    xh = xhat_of(frames)[:, :, :2]                        # [n, T4, 2]: x_hat of frame t given frames < t
    bern = np.where(hs == 1, xh, 1 - xh)
    clamped = ROLL01 <= 1
    consistent = np.all(~clamped[None] | (hs == ROLL01[None]), axis=(1, 2))
    joint = np.prod(bern, axis=(1, 2)) * consistent
    anc = np.prod(np.where(clamped[None], 1.0, bern), axis=(1, 2)) * consistent
    Z = joint.sum()
    post = (joint[:, None, None] * hs).sum(0) / Z
    ancm = (anc[:, None, None] * hs).sum(0) / anc.sum()
    return Z, post, ancm


def _check_exactness(gen, xhat_of, G=256, P=64):
    Z, post, ancm = _exact(xhat_of)
    free = ROLL01 > 1
    assert np.abs(post - ancm)[free].max() >= 0.2
    roll = np.full((G, T4, D), FREE, np.uint8)
    roll[:, :, :2] = ROLL01
    r = gen(roll, P)
    Xs, logZ = r.Xs[:, 0].cpu().numpy(), r.log_evidence.cpu().numpy()
    assert np.all(Xs[:, :, 2:] == 0) and np.all(Xs[:, :, :2][:, ~free] == ROLL01[~free])
    ratio = np.exp(logZ - np.log(Z))
    assert abs(ratio.mean() - 1) < 4 * ratio.std() / np.sqrt(G) + 1e-9, (ratio.mean(), ratio.std())
    sig = np.sqrt(np.maximum(post * (1 - post), 0.01) / G)
    m = Xs[:, :, :2].mean(0)
    assert np.all(np.abs(m - post)[free] < 4 * sig[free]), (m, post)
    r1 = gen(roll, 1)                                     # the power check: ancestral sampling is far off
    m1 = r1.Xs[:, 0, :, :2].cpu().numpy().mean(0)
    assert np.abs(m1 - post)[free].max() > 8 * sig[free][np.argmax(np.abs(m1 - post)[free])]
    assert np.all(np.isfinite(r1.log_evidence.cpu().numpy()))


def test_exact_posterior_on_enumerable_vrnn(dev):
    eng, p = _enumerable_vrnn(dev, B=4)
    G = 256
    x_seed = torch.zeros(G, 0, D, device=dev)
    w = torch.as_tensor(np.eye(10, dtype=np.float32)[np.arange(G) % 10], device=dev)

    def xhat_of(frames):
        n = frames.shape[0]
        inputs = np.concatenate([np.zeros((n, 1, D)), frames[:, :-1]], 1)
        return _vrnn_xhat_along(p, inputs, np.eye(10)[np.zeros(n, int)], 0, 2)

    _check_exactness(lambda roll, P: eng.generate_smc(x_seed, w, T4, roll, P, seed=41), xhat_of, G=G)


def test_exact_posterior_on_enumerable_vae(dev):
    eng, p = _enumerable_vae(dev, B=4096)                 # 256 x 64 rows: four chunks
    G = 256
    x_seed = torch.zeros(G, D, device=dev)
    w = torch.as_tensor(np.eye(4, dtype=np.float32)[np.arange(G) % 4], device=dev)

    def xhat_of(frames):
        n = frames.shape[0]
        return _vae_xhat_along(p, np.zeros((n, D)), frames, np.eye(4)[np.zeros(n, int)], 0, 3)

    _check_exactness(lambda roll, P: eng.generate_smc(x_seed, w, T4, roll, P, seed=43), xhat_of, G=G)


# ------------------------------------------------------------------ 5. the sample CLIs with --particles
@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_particles_cli_end_to_end(dev, tmp_path, capsys, monkeypatch, which):
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
        parser.parse_args(common + ['--particles', '8'])
    args = parser.parse_args(common + ['--harmonize', 'top', '--particles', '8'])
    assert args.particles == 8
    seen = []
    real = S.harmonize

    def spy(model, seeds, sources, w_vals, **kw):
        seen.append((np.asarray(sources), kw))
        return real(model, seeds, sources, w_vals, **kw)
    monkeypatch.setattr(S, 'harmonize', spy)
    np.random.seed(3)
    capsys.readouterr()
    rolls = S.sample(args)
    printed = capsys.readouterr().out
    assert len(rolls) == 3 and len(seen) == 1 and seen[0][1]['particles'] == 8 and seen[0][1]['voice'] == 'top'
    assert all(set(np.unique(r)) <= {0.0, 1.0} for r in rolls)
    assert sum('log p(voice) per frame' in line for line in printed.splitlines()) == 3
    for roll, src in zip(rolls, seen[0][0]):          # the top voice of the source frames is kept
        assert roll.shape == src.shape
        for t in range(src.shape[0]):
            sn = np.nonzero(src[t])[0]
            if len(sn):
                g = np.nonzero(roll[t])[0]
                assert len(g) and g.max() == sn.max(), t
    files = os.listdir(sdir)
    for j in range(3):
        for name in ('h_%d.mid' % j, 'h_%d_source.mid' % j):
            assert name in files and open(os.path.join(sdir, name), 'rb').read()[:4] == b'MThd'


# ------------------------------------------------------------------ 6. ValueError cases
def test_smc_value_errors(dev):
    from clvae_amd.cl_vae import model as MV
    from clvae_amd.cl_vrnn import model as MR
    from clvae_amd.harmonize import harmonize
    N, nsteps = 2, 4
    vr, _ = MR.get_model(4, 88, 88, 2, 8, 3, True, 'adam', seed=1)
    va, _ = MV.get_model(4, 88, (88, 2), (88, 3), 'adam', use_x_prev=True, seed=1)
    seeds_r, seeds_a, w = np.zeros((N, 2, 88)), np.zeros((N, 88)), np.eye(3)[[0, 1]]
    roll = np.full((N, nsteps, 88), FREE, np.uint8)
    for gen, seeds in ((MR.generate_samples_device, seeds_r), (MV.generate_samples_device, seeds_a)):
        for kw in (dict(particles=0, clamp=roll), dict(particles=-3, clamp=roll), dict(particles=2.5, clamp=roll),
                   dict(particles=4), dict(particles=4, clamp=roll, resample_threshold=-0.1),
                   dict(particles=4, clamp=roll, resample_threshold=1.5), dict(clamp=roll, return_evidence=True)):
            with pytest.raises(ValueError):
                gen(vr if seeds is seeds_r else va, seeds, nsteps, w, **kw)
    with pytest.raises(ValueError):
        vr.engine.generate_smc(torch.zeros(N, 2, 88, device=dev), torch.as_tensor(w, dtype=torch.float32, device=dev),
                               nsteps, roll, 4, n_out=0)
    with pytest.raises(ValueError):
        harmonize(vr, seeds_r, np.zeros((N, nsteps, 88)), w, particles=0)
    out, le = MR.generate_samples_device(vr, seeds_r, nsteps, w, clamp=roll, particles=3, return_evidence=True)
    assert out.shape == (N, nsteps, 88) and le.shape == (N,) and np.all(le == 0)
