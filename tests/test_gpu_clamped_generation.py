"""-m gpu: generation under a constraint roll (clamped ancestral sampling) on both engines and both routes: the persistent
kernels (csrc/generate.hip, csrc/vae_generate.hip, CL instances) and the per-frame chains (clv_bernoulli_sample_clamped)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import make_synthetic_pickle
from oracle import clvae_oracle as O
from oracle import philox as OP

pytestmark = pytest.mark.gpu

FREE = 255


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _vrnn(dev, L, use_x_prev=True, gate='hard_sigmoid', Cn=10, B=4, seed=5):
    from clvae_amd.engine import VrnnEngine
    cfg = O.vrnn_config(latent_dim=L, seq_length=8, n_classes=Cn, use_x_prev=use_x_prev, gate_act=gate)
    rng = np.random.default_rng(L)
    p = {k: np.asarray(v, np.float32) for k, v in O.vrnn_init_params(cfg, seed=seed).items()}
    for k in p:                                    # livelier weights than the initialisers give
        if not k.startswith('hW'):
            p[k] = (p[k] + 0.15 * rng.standard_normal(p[k].shape)).astype(np.float32)
    eng = VrnnEngine(cfg, B, dev)
    eng.P.set_weights(p)
    return eng


def _vae(dev, L=3, C=4, use_x_prev=True, B=8):
    from clvae_amd.engine import VaeEngine
    cfg = O.vae_config(latent_dim=L, n_classes=C, use_x_prev=use_x_prev)
    rng = np.random.default_rng(L + C)
    p = {k: np.asarray(v, np.float32) for k, v in O.vae_init_params(cfg, seed=6).items()}
    for k in p:
        p[k] = (p[k] + 0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    p['x_decoded_mean/bias'] = (p['x_decoded_mean/bias'] - 2.0).astype(np.float32)
    eng = VaeEngine(cfg, B, dev)
    eng.P.set_weights(p)
    return eng


def _inputs(dev, N, S, C, seed):
    rng = np.random.default_rng(seed)
    shape = (N, S, 88) if S is not None else (N, 88)
    x_seed = torch.as_tensor((rng.random(shape) < 0.06).astype(np.float32), device=dev)
    w = torch.as_tensor(np.eye(C, dtype=np.float32)[rng.integers(0, C, N)], device=dev)
    return x_seed, w


def _roll(N, nsteps, frac=0.3, on=0.3, seed=0):
    """about `frac` of the notes clamped, a fraction `on` of those forced on"""
    rng = np.random.default_rng(seed)
    r = rng.random((N, nsteps, 88))
    return np.where(r < frac, (r < frac * on).astype(np.uint8), np.uint8(FREE)).astype(np.uint8)


def _uniform(dev, N, seed, step):
    from clvae_amd import ops
    u = torch.zeros(N, 88, dtype=torch.float32, device=dev)
    ops.philox_uniform(u, N * 88, seed, step, 1, 0)
    return u


def _check_clamped(Xs, clamp):
    c = torch.as_tensor(clamp, device=Xs.device)
    fixed = c <= 1
    assert torch.equal(Xs[fixed], c[fixed].float())
    return fixed


# ------------------------------------------------------------------ 1. an all-FREE roll changes nothing
@pytest.mark.parametrize("persistent", [True, False])
def test_all_free_roll_is_bit_identical_vrnn(dev, persistent):
    eng = _vrnn(dev, 2)
    N, S, nsteps, seed = 3, 4, 7, 11
    x_seed, w = _inputs(dev, N, S, 10, 1)
    free = np.full((N, nsteps, 88), FREE, np.uint8)
    kw = dict(seed=seed, persistent=persistent)
    if persistent:
        xh0, xh1 = (torch.zeros(N, S + nsteps, 88, device=dev) for _ in range(2))
        a = eng.generate(x_seed, w, nsteps, xhat_out=xh0, **kw)
        b = eng.generate(x_seed, w, nsteps, xhat_out=xh1, clamp=free, **kw)
        assert torch.equal(xh0, xh1)
    else:
        a = eng.generate(x_seed, w, nsteps, **kw)
        b = eng.generate(x_seed, w, nsteps, clamp=free, **kw)
    assert torch.equal(a, b) and 0 < float(a.mean()) < 1


@pytest.mark.parametrize("persistent", [True, False])
def test_all_free_roll_is_bit_identical_vae(dev, persistent):
    eng = _vae(dev)
    N, nsteps, seed = 5, 9, 99
    x_seed, w = _inputs(dev, N, None, 4, 2)
    free = torch.full((N, nsteps, 88), FREE, dtype=torch.uint8, device=dev)
    kw = dict(seed=seed, persistent=persistent)
    if persistent:
        xh0, xh1 = (torch.zeros(N, nsteps, 88, device=dev) for _ in range(2))
        a = eng.generate(x_seed, w, nsteps, xhat_out=xh0, **kw)
        b = eng.generate(x_seed, w, nsteps, xhat_out=xh1, clamp=free, **kw)
        assert torch.equal(xh0, xh1)
    else:
        a = eng.generate(x_seed, w, nsteps, **kw)
        b = eng.generate(x_seed, w, nsteps, clamp=free, **kw)
    assert torch.equal(a, b) and 0 < float(a.mean()) < 1


# ------------------------------------------------------------------ 2. persistent cl_vrnn under ~30 % clamped notes
@pytest.mark.parametrize("N,L,use_x_prev,gate,z_prior", [(3, 2, True, 'hard_sigmoid', False), (2, 5, False, 'sigmoid', False),
                                                         (1, 16, True, 'hard_sigmoid', True), (2, 32, True, 'hard_sigmoid', False),
                                                         (2, 19, False, 'sigmoid', False), (2, 32, True, 'sigmoid', False)])
def test_persistent_clamped_generation(dev, N, L, use_x_prev, gate, z_prior):
    from clvae_amd import ops
    Cn, S, nsteps, seed = 10, 5, 9, 4242
    eng = _vrnn(dev, L, use_x_prev, gate, Cn)
    f = dict(dtype=torch.float32, device=dev)
    x_seed, w = _inputs(dev, N, S, Cn, L)
    clamp = _roll(N, nsteps, seed=L)
    xhat = torch.zeros(N, S + nsteps, 88, **f)
    Xs = eng.generate(x_seed, w, nsteps, seed=seed, z_prior=z_prior, xhat_out=xhat, clamp=clamp)
    torch.cuda.synchronize()
    fixed = _check_clamped(Xs, clamp)
    assert 0.2 < float(fixed.float().mean()) < 0.4
    # every free note is [u <= x_hat] with the documented uniform (step S+j, stream 1, index n*88+k)
    for j in range(nsteps):
        drawn = (_uniform(dev, N, seed, S + j) <= xhat[:, S + j]).float()
        free = ~fixed[:, j]
        assert torch.equal(Xs[:, j][free], drawn[free])
    # teacher-forcing the bridge sample (unconstrained) and the returned frames reproduces x_hat bit for bit
    x_bridge = (_uniform(dev, N, seed, S - 1) <= xhat[:, S - 1]).float().unsqueeze(1)
    forced = torch.cat([x_seed, x_bridge, Xs[:, :-1]], dim=1).contiguous()
    xhat2 = torch.zeros(N, S + nsteps, 88, **f)
    eng.generate(forced, w, 0, seed=seed, z_prior=z_prior, xhat_out=xhat2)
    torch.cuda.synchronize()
    assert torch.equal(xhat2, xhat)
    # the host-driven single-step path
    st = eng.new_state(N)
    eps, z = torch.zeros(N, L, **f), torch.zeros(N, L, **f)
    for t in range(S + nsteps):
        x = forced[:, t].contiguous()
        eng.enc_step(x, w, st)
        ops.philox_normal(eps, N * L, seed, t, 0, 0)
        if z_prior:
            st['zargs'].zero_()
        ops.gauss_fwd(N, L, st['zargs'], eps, z, L, None)
        eng.dec_step(z, x if use_x_prev else None, w, st)
        torch.cuda.synchronize()
        np.testing.assert_allclose(xhat[:, t].cpu().numpy(), st['xhat'].cpu().numpy(), rtol=0, atol=2e-5)


# ------------------------------------------------------------------ 3. fp64 oracle frame loops with clamps
def _apply(x_t, c):
    return np.where(c <= 1, c.astype(np.float64), x_t)


def test_vrnn_clamped_generation_matches_oracle(dev):
    from clvae_amd.cl_vrnn.model import generate_samples_device, get_model
    T, L, C, N, S, nsteps, seed = 8, 2, 10, 5, 3, 6, 31
    model, _ = get_model(4, 88, 88, L, T, C, True, 'adam', seed=9)
    p = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in model.engine.P.get_weights().items()}
    rng = np.random.default_rng(4)
    seeds = (rng.random((N, S, 88)) < 0.06).astype(np.float64)
    w = np.eye(C)[rng.integers(0, C, N)]
    clamp = _roll(N, nsteps, seed=3)
    out = generate_samples_device(model, seeds, nsteps, w, seed=seed, clamp=clamp)
    assert out.shape == (N, nsteps, 88)
    H = 88
    he, ce, hd, cd = (np.zeros((N, H)) for _ in range(4))

    def cell(x, h, c, k, r, b):
        zz = x @ k + b + h @ r
        i, f_, g, o = O.hard_sigmoid(zz[:, :H]), O.hard_sigmoid(zz[:, H:2 * H]), np.tanh(zz[:, 2 * H:3 * H]), O.hard_sigmoid(zz[:, 3 * H:])
        c = f_ * c + i * g
        return o * np.tanh(c), c
    flips = 0
    for t in range(S + nsteps):
        if t < S:
            x_prev = seeds[:, t]
        he, ce = cell(np.concatenate([x_prev, w], 1), he, ce, p['encoder_h/kernel'], p['encoder_h/recurrent_kernel'], p['encoder_h/bias'])
        zm = he @ p['Z_mean/kernel'] + p['Z_mean/bias']; zlv = he @ p['Z_log_var/kernel'] + p['Z_log_var/bias']
        eps = OP.normal(N * L, seed, step=t, stream_id=0).reshape(N, L).astype(np.float64)
        z = zm + np.exp(zlv / 2) * eps
        hd, cd = cell(np.concatenate([x_prev, z, w], 1), hd, cd, p['decoder_h/kernel'], p['decoder_h/recurrent_kernel'], p['decoder_h/bias'])
        xhat = O.sigmoid(hd @ p['X_decoded_mean/kernel'] + p['X_decoded_mean/bias'])
        uu = OP.uniform(N * 88, seed, step=t, stream_id=1).reshape(N, 88).astype(np.float64)
        x_t = (uu <= xhat).astype(np.float64)
        if t >= S:
            c = clamp[:, t - S]
            x_t = _apply(x_t, c)
            got = out[:, t - S]
            assert np.array_equal(got[c <= 1], c[c <= 1].astype(np.float64))
            close = np.abs(uu - xhat) < 1e-5           # a free draw within fp32 noise of its probability may flip
            assert np.all((got == x_t) | close), (t, np.argwhere((got != x_t) & ~close)[:3])
            flips += int((got != x_t).sum())
            x_t = got
        x_prev = x_t
    assert flips <= 2


def test_vae_clamped_generation_matches_oracle(dev):
    from clvae_amd.cl_vae.model import generate_samples_device, get_model
    L, C, N, nsteps, seed = 3, 4, 6, 7, 17
    model, _ = get_model(8, 88, (88, L), (88, C), 'adam', use_x_prev=True, seed=2)
    p = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in model.engine.P.get_weights().items()}
    rng = np.random.default_rng(8)
    seeds = (rng.random((N, 88)) < 0.06).astype(np.float64)
    w = np.eye(C)[rng.integers(0, C, N)]
    clamp = _roll(N, nsteps, seed=5)
    out = generate_samples_device(model, seeds, nsteps, w, seed=seed, clamp=clamp)
    x_in, hist, flips = seeds, seeds, 0
    for t in range(nsteps):
        h = O.relu(np.concatenate([x_in, w], 1) @ p['h/kernel'] + p['h/bias'])
        zm, zlv = h @ p['z_mean/kernel'] + p['z_mean/bias'], h @ p['z_log_var/kernel'] + p['z_log_var/bias']
        eps = OP.normal(N * L, seed, step=t, stream_id=0).reshape(N, L).astype(np.float64)
        z = zm + np.exp(zlv / 2) * eps
        hd = O.relu(np.concatenate([w, hist, z], 1) @ p['decoder_h/kernel'] + p['decoder_h/bias'])
        xhat = O.sigmoid(hd @ p['x_decoded_mean/kernel'] + p['x_decoded_mean/bias'])
        uu = OP.uniform(N * 88, seed, step=t, stream_id=1).reshape(N, 88).astype(np.float64)
        c = clamp[:, t]
        x_t, got = _apply((uu <= xhat).astype(np.float64), c), out[:, t]
        assert np.array_equal(got[c <= 1], c[c <= 1].astype(np.float64))
        close = np.abs(uu - xhat) < 1e-5
        assert np.all((got == x_t) | close), (t, np.argwhere((got != x_t) & ~close)[:3])
        flips += int((got != x_t).sum())
        hist, x_in = x_in, got
    assert flips <= 2


# ------------------------------------------------------------------ 4. persistent kernel against the frame chain
def _agree_until_a_near_flip(dev, Xp, Xf, xhat, seed, step0, clamp):
    """the two routes give the same frames; they may part only where a free draw lies within rounding of its probability"""
    _check_clamped(Xp, clamp)
    _check_clamped(Xf, clamp)
    N = Xp.shape[0]
    for j in range(Xp.shape[1]):
        diff = Xp[:, j] != Xf[:, j]
        if diff.any():
            u = _uniform(dev, N, seed, step0 + j)
            assert float((u - xhat[:, step0 + j]).abs()[diff].max()) < 1e-5
            return j
    return None


@pytest.mark.parametrize("L", [2, 19])
def test_vrnn_persistent_matches_frame_chain_under_constraints(dev, L):
    N, S, nsteps, seed = 4, 3, 8, 7
    eng = _vrnn(dev, L)
    x_seed, w = _inputs(dev, N, S, 10, 3)
    clamp = _roll(N, nsteps, seed=9)
    xhat = torch.zeros(N, S + nsteps, 88, device=dev)
    Xp = eng.generate(x_seed, w, nsteps, seed=seed, xhat_out=xhat, clamp=clamp)
    Xf = eng.generate(x_seed, w, nsteps, seed=seed, persistent=False, clamp=clamp)
    torch.cuda.synchronize()
    _agree_until_a_near_flip(dev, Xp, Xf, xhat, seed, S, clamp)
    # S = 0: no bridge, row 0 constrains the first sample
    x0 = torch.zeros(N, 0, 88, device=dev)
    xhat0 = torch.zeros(N, nsteps, 88, device=dev)
    Xp0 = eng.generate(x0, w, nsteps, seed=seed, xhat_out=xhat0, clamp=clamp)
    Xf0 = eng.generate(x0, w, nsteps, seed=seed, persistent=False, clamp=clamp)
    _agree_until_a_near_flip(dev, Xp0, Xf0, xhat0, seed, 0, clamp)


def test_vae_persistent_matches_frame_chain_under_constraints(dev):
    N, nsteps, seed = 6, 9, 5
    eng = _vae(dev)
    x_seed, w = _inputs(dev, N, None, 4, 4)
    clamp = _roll(N, nsteps, seed=11)
    xhat = torch.zeros(N, nsteps, 88, device=dev)
    Xp = eng.generate(x_seed, w, nsteps, seed=seed, xhat_out=xhat, clamp=clamp)
    Xf = eng.generate(x_seed, w, nsteps, seed=seed, persistent=False, clamp=clamp)
    torch.cuda.synchronize()
    _agree_until_a_near_flip(dev, Xp, Xf, xhat, seed, 0, clamp)


# ------------------------------------------------------------------ 5. many sequences on NaN-poisoned outputs
def test_large_batch_on_poisoned_memory(dev):
    from clvae_amd import ops
    N, S, nsteps, seed, pad = 1024, 2, 64, 3, 4096
    clamp = torch.as_tensor(_roll(N, nsteps, seed=1), device=dev)
    nan = float('nan')
    # cl_vrnn, wide latent
    eng = _vrnn(dev, 32)
    cfg, P, off = eng.cfg, eng.P, eng.off
    x_seed, w = _inputs(dev, N, S, 10, 5)
    L, D = cfg['L'], 88
    buf = torch.full((N * nsteps * D + pad,), nan, device=dev)
    xbuf = torch.full((N * (S + nsteps) * D + pad,), nan, device=dev)
    Xs, xhat = buf[:N * nsteps * D].view(N, nsteps, D), xbuf[:N * (S + nsteps) * D].view(N, S + nsteps, D)
    rows = lambda name, r: P.rows(P.params, name, r)
    ops.vrnn_generate(N, S, nsteps, D, 88, L, 10, eng.gate_act, False, seed, x_seed, w, P.p('encoder_h/kernel'),
                      rows('encoder_h/kernel', D), P.p('encoder_h/bias'), P.p('encoder_h/recurrent_kernel'), P.p('Zargs/kernel'),
                      P.p('Zargs/bias'), P.p('decoder_h/kernel'), rows('decoder_h/kernel', off), rows('decoder_h/kernel', off + L),
                      P.p('decoder_h/bias'), P.p('decoder_h/recurrent_kernel'), P.p('X_decoded_mean/kernel'),
                      P.p('X_decoded_mean/bias'), Xs, xhat, clamp=clamp)
    torch.cuda.synchronize()
    assert not torch.isnan(Xs).any() and not torch.isnan(xhat).any()
    assert torch.isnan(buf[N * nsteps * D:]).all() and torch.isnan(xbuf[N * (S + nsteps) * D:]).all()
    assert set(torch.unique(Xs).tolist()) <= {0.0, 1.0}
    _check_clamped(Xs, clamp)
    # cl_vae
    ev = _vae(dev, L=8, C=4)
    xs1, w1 = _inputs(dev, N, None, 4, 6)
    buf.fill_(nan)
    xb = torch.full((N * nsteps * D + pad,), nan, device=dev)
    Xs, xhat = buf[:N * nsteps * D].view(N, nsteps, D), xb[:N * nsteps * D].view(N, nsteps, D)
    Pv = ev.P
    ops.vae_generate(N, nsteps, D, 88, 8, 4, True, False, seed, xs1, w1, Pv.p('h/kernel'), Pv.p('h/bias'), Pv.p('zargs/kernel'),
                     Pv.p('zargs/bias'), Pv.p('decoder_h/kernel'), Pv.p('decoder_h/bias'), Pv.p('x_decoded_mean/kernel'),
                     Pv.p('x_decoded_mean/bias'), Xs, xhat, clamp=clamp)
    torch.cuda.synchronize()
    assert not torch.isnan(Xs).any() and not torch.isnan(xhat).any()
    assert torch.isnan(buf[N * nsteps * D:]).all() and torch.isnan(xb[N * nsteps * D:]).all()
    _check_clamped(Xs, clamp)


# ------------------------------------------------------------------ 6. a roll that fixes every note
@pytest.mark.parametrize("persistent", [True, False])
def test_fully_fixed_roll_returns_the_constraint(dev, persistent):
    N, S, nsteps = 3, 2, 6
    roll = (np.random.default_rng(0).random((N, nsteps, 88)) < 0.1).astype(np.uint8)
    eng = _vrnn(dev, 2)
    x_seed, w = _inputs(dev, N, S, 10, 7)
    out = eng.generate(x_seed, w, nsteps, seed=1, persistent=persistent, clamp=roll)
    assert np.array_equal(out.cpu().numpy(), roll.astype(np.float32))
    ev = _vae(dev)
    xs1, w1 = _inputs(dev, N, None, 4, 8)
    out = ev.generate(xs1, w1, nsteps, seed=1, persistent=persistent, clamp=roll)
    assert np.array_equal(out.cpu().numpy(), roll.astype(np.float32))


# ------------------------------------------------------------------ 7. wrong shape or dtype
def test_wrong_clamp_raises_value_error(dev):
    from clvae_amd.cl_vae import model as MV
    from clvae_amd.cl_vrnn import model as MR
    N, nsteps = 2, 4
    vr, _ = MR.get_model(4, 88, 88, 2, 8, 3, True, 'adam', seed=1)
    va, _ = MV.get_model(4, 88, (88, 2), (88, 3), 'adam', use_x_prev=True, seed=1)
    seeds_r, seeds_a, w = np.zeros((N, 2, 88)), np.zeros((N, 88)), np.eye(3)[[0, 1]]
    for bad in (np.zeros((N, nsteps, 88), np.float32), np.zeros((N, nsteps + 1, 88), np.uint8),
                np.zeros((N, nsteps, 87), np.uint8), torch.zeros(N, nsteps, 88, dtype=torch.int32)):
        with pytest.raises(ValueError):
            MR.generate_samples_device(vr, seeds_r, nsteps, w, clamp=bad)
        with pytest.raises(ValueError):
            MV.generate_samples_device(va, seeds_a, nsteps, w, clamp=bad)


# ------------------------------------------------------------------ 8. both CLIs with --harmonize top
def _top_voice_kept(rolls, sources):
    for roll, src in zip(rolls, sources):
        assert roll.shape == src.shape
        for t in range(src.shape[0]):
            s = np.nonzero(src[t])[0]
            if len(s):
                g = np.nonzero(roll[t])[0]
                assert len(g) and g.max() == s.max(), t


@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_harmonize_cli_end_to_end(dev, tmp_path, monkeypatch, which):
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
    seen = []
    real = S.harmonize

    def spy(model, seeds, sources, w_vals, **kw):
        seen.append(np.asarray(sources))
        assert kw['voice'] == 'top'
        return real(model, seeds, sources, w_vals, **kw)
    monkeypatch.setattr(S, 'harmonize', spy)
    args = parser_for('%s.sample' % which, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS).parse_args(
        ['h', '-n', '3', '-t', '8', '--harmonize', 'top', '--seed', '4', '-i', os.path.join(mdir, 'm.h5'),
         '--train_file', data, '--sample_dir', sdir])
    np.random.seed(3)
    rolls = S.sample(args)
    assert len(rolls) == 3 and len(seen) == 1 and seen[0].shape == (3, 8, 88)
    assert all(set(np.unique(r)) <= {0.0, 1.0} for r in rolls)
    assert any(seen[0][j].any() for j in range(3))
    _top_voice_kept(rolls, seen[0])
    files = os.listdir(sdir)
    for j in range(3):
        for name in ('h_%d.mid' % j, 'h_%d_source.mid' % j):
            assert name in files and open(os.path.join(sdir, name), 'rb').read()[:4] == b'MThd'
    if which == 'cl_vrnn':
        assert sum(f.startswith('h%d_seed_' % j) for f in files for j in range(3)) == 3
