"""-m gpu: particle Gibbs: the four kernels against the fp64 reference (tests/gibbs_reference.py), the
identities that tie generate_gibbs to generate_smc bit for bit on both engines, the constraints on every retained path,
exactness on the enumerable models of tests/test_gpu_smc.py with the CPU test's M, P and K, and the sample CLIs."""
import importlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gibbs_reference as GR
import test_gibbs_reference as TG
import test_gpu_smc as TS
from helpers import make_synthetic_pickle

pytestmark = pytest.mark.gpu

FREE = 255
D = 88


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


# ------------------------------------------------------------------ 1. the kernels against the reference
@pytest.mark.parametrize("P", [1, 5])
@pytest.mark.parametrize("S", [0, 2])
def test_pin_kernels(dev, P, S):
    from clvae_amd import ops
    rng = np.random.default_rng(10 * P + S)
    G, nsteps, L = 3, 4, 3
    R, T = G * P, S + nsteps
    t = lambda a: torch.as_tensor(a, device=dev)
    z_ref = rng.standard_normal((G, T, L)).astype(np.float32)
    x_ref = (rng.random((G, nsteps, D)) < 0.4).astype(np.uint8)
    bridge = (rng.random((G, D)) < 0.4).astype(np.float32)
    z0 = rng.standard_normal((R, L)).astype(np.float32)
    x0 = (rng.random((R, D)) < 0.4).astype(np.float32)
    h0 = np.full((nsteps, R, D), 7, np.uint8)
    for step in range(-1, T + 2):
        z, x, hist = t(z0), t(x0), t(h0)
        ops.smc_pin_z(G, P, L, T, t(z_ref), TS._counter(dev, step), z)
        ops.smc_pin_frame(G, P, D, nsteps, S, t(x_ref), t(bridge) if S else None, TS._counter(dev, step), x, hist)
        torch.cuda.synchronize()
        assert np.array_equal(z.cpu().numpy(), GR.pin_z(z0, z_ref, step, P)), step
        wx, wh = GR.pin_frame(x0, h0, x_ref, bridge if S else None, step, S, P)
        assert np.array_equal(x.cpu().numpy(), wx) and np.array_equal(hist.cpu().numpy(), wh), step
        if not 0 <= step < T:
            assert np.array_equal(z.cpu().numpy(), z0)
        if not S - 1 <= step < T or (S == 0 and step < 0):
            assert np.array_equal(x.cpu().numpy(), x0) and np.array_equal(hist.cpu().numpy(), h0)
    # without a bridge pointer the bridge step pins nothing
    if S:
        x, hist = t(x0), t(h0)
        ops.smc_pin_frame(G, P, D, nsteps, S, t(x_ref), None, TS._counter(dev, S - 1), x, hist)
        torch.cuda.synchronize()
        assert np.array_equal(x.cpu().numpy(), x0) and np.array_equal(hist.cpu().numpy(), h0)


@pytest.mark.parametrize("P", [2, 63, 64, 65, 1024])
@pytest.mark.parametrize("tau", [0.5, 1.0])
def test_resample_conditional_kernel(dev, P, tau):
    from clvae_amd import ops
    rng = np.random.default_rng(P)
    G = 3 if P < 1024 else 2
    nsteps, S, seed, m0 = 6, 3, GR.sweep_seed(77, 2), 5
    R = G * P
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    ell, logW = torch.zeros(R, **f64), torch.full((R,), float('nan'), **f64)
    logZ, ess = torch.full((G,), float('nan'), **f64), torch.zeros(G, nsteps, **f64)
    nres, flag, anc = torch.full((G,), -5, **i32), torch.zeros(G, **i32), torch.full((nsteps, R), -1, **i32)
    ref = GR.ConditionalFilter(G, P, nsteps, tau, seed, m0)
    for k in range(nsteps):
        scale = [0.0, 0.3, 3.0][k % 3]
        e = -np.abs(rng.standard_normal(R)) * scale - rng.random(R) * 2 * (k % 2)
        ell.copy_(torch.as_tensor(e, device=dev))
        ops.smc_resample_conditional(G, P, nsteps, S, seed, m0, tau, ell, logW, logZ, ess, nres, flag, anc,
                                     TS._counter(dev, S + k))
        ref.step(e, S + k, k)
        torch.cuda.synchronize()
        np.testing.assert_allclose(logZ.cpu().numpy(), ref.logZ, rtol=1e-12, atol=0)
        np.testing.assert_allclose(logW.cpu().numpy(), ref.logW.reshape(-1), rtol=1e-12, atol=0)
        np.testing.assert_allclose(ess[:, k].cpu().numpy(), ref.ess[:, k], rtol=1e-12, atol=0)
        assert np.array_equal(flag.cpu().numpy().astype(bool), ref.resampled[k])
        a = anc[k].cpu().numpy()
        assert not ref.near[k].any()                      # no draw of this test sits within 1e-9 of a cumulative weight
        assert np.array_equal(a, ref.anc[k]), (k, np.argwhere(a != ref.anc[k])[:4])
        assert np.array_equal(a[::P], np.arange(G) * P)   # the pinned particle keeps itself
    assert np.array_equal(nres.cpu().numpy(), ref.nres)
    if tau * P <= 1:                                      # an ESS is at least 1: two particles at tau = 0.5 never resample
        assert ref.nres.sum() == 0
    else:
        assert ref.nres.sum() > 0
    # steps outside [S, S + nsteps) change nothing
    before = [t.clone() for t in (logW, logZ, ess, nres, anc)]
    for c in (S - 1, S + nsteps):
        ops.smc_resample_conditional(G, P, nsteps, S, seed, m0, tau, ell, logW, logZ, ess, nres, flag, anc,
                                     TS._counter(dev, c))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (logW, logZ, ess, nres, anc)))


@pytest.mark.parametrize("P,S", [(1, 0), (5, 2), (70, 1), (5, 0)])
def test_backtrack_path_kernel(dev, P, S):
    from clvae_amd import ops
    rng = np.random.default_rng(P + S)
    G, nsteps, L = 6, 5, 3
    R, T = G * P, S + nsteps
    anc = (np.arange(R)[None] // P * P + rng.integers(0, P, (nsteps, R))).astype(np.int32)
    anc[:, 0] = 0                                         # melody 0's pinned row keeps itself, and is picked below
    hist = (rng.random((nsteps, R, D)) < 0.3).astype(np.uint8)
    zhist = rng.standard_normal((T, R, L)).astype(np.float32)
    brows = (rng.random((R, D)) < 0.3).astype(np.float32)
    picks = rng.integers(0, P, G).astype(np.int32)
    picks[0] = 0
    t = lambda a: torch.as_tensor(a, device=dev)
    x_ref = torch.full((G, nsteps, D), 9, dtype=torch.uint8, device=dev)
    z_ref = torch.full((G, T, L), float('nan'), device=dev)
    b_ref = torch.full((G, D), float('nan'), device=dev) if S else None
    renewed = torch.full((G, nsteps), 9, dtype=torch.uint8, device=dev)
    ops.smc_backtrack_path(G, P, nsteps, S, D, L, t(picks), t(anc), t(hist), t(zhist), t(brows) if S else None, x_ref, z_ref,
                           b_ref, renewed)
    torch.cuda.synchronize()
    wx, wz, wb, wr = GR.backtrack_path(picks, anc, hist, zhist, brows if S else None, P, S)
    assert np.array_equal(x_ref.cpu().numpy(), wx) and np.array_equal(z_ref.cpu().numpy(), wz)
    assert np.array_equal(renewed.cpu().numpy(), wr.astype(np.uint8))
    if S:
        assert np.array_equal(b_ref.cpu().numpy(), wb)
    assert not wr[0].any()
    assert wr.any() == (P > 1)


# ------------------------------------------------------------------ 2. identities, bit for bit
def _cases(dev):
    """(name, engine, x_seed, w, C) for cl_vrnn with S = 0 and S = 2 and cl_vae, 6 melodies, random weights"""
    ev, _ = TS._vrnn(dev)
    va, _ = TS._vae(dev, B=48)
    out = []
    for name, eng, S, C in (('vrnn_S0', ev, 0, 10), ('vrnn_S2', ev, 2, 10), ('vae', va, None, 4)):
        x_seed, w = TS._inputs(dev, 6, S, C, 8)
        out.append((name, eng, x_seed, w))
    return out


@pytest.fixture(scope="module")
def cases(dev):
    return _cases(dev)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_one_sweep_is_the_filter(dev, cases):
    rng = np.random.default_rng(7)
    nsteps, P, seed = 6, 8, 31
    for name, eng, x_seed, w in cases:
        roll = TS._roll(rng, 6, nsteps, frac=0.2)
        a = eng.generate_smc(x_seed, w, nsteps, roll, P, resample_threshold=0.6, n_out=1, seed=seed)
        g = eng.generate_gibbs(x_seed, w, nsteps, roll, P, 1, resample_threshold=0.6, seed=seed)
        torch.cuda.synchronize()
        assert int(a.resamples.sum()) > 0, name
        assert torch.equal(g.Xs[:, 0], a.Xs[:, 0]) and torch.equal(g.log_evidence[:, 0], a.log_evidence), name
        assert bool(g.renewed.all()) and g.renewed.shape == (6, 1, nsteps), name
        S = x_seed.shape[1] if x_seed.dim() == 3 else 0
        assert g.z.shape == (6, S + nsteps, eng.cfg['L']) and bool(torch.isfinite(g.z).all()), name
        # more sweeps leave sweep 0 alone
        g3 = eng.generate_gibbs(x_seed, w, nsteps, roll, P, 3, resample_threshold=0.6, seed=seed)
        assert torch.equal(g3.Xs[:, 0], a.Xs[:, 0]) and torch.equal(g3.log_evidence[:, 0], a.log_evidence), name
        assert bool(g3.renewed[:, 0].all()) and bool(g3.renewed[:, 1:].any()) and not bool(g3.renewed[:, 1:].all()), name


def test_one_particle_keeps_its_path(dev, cases):
    """P = 1: the only particle is the pinned one, so every sweep must return sweep 0's path and, the weights not being
    zero, its log evidence bit for bit -- although each sweep draws under another key.  That holds only if the latents,
    the bridge and the frames of the retained path all reach the decoder."""
    rng = np.random.default_rng(9)
    nsteps, seed = 6, 5
    for name, eng, x_seed, w in cases:
        roll = TS._roll(rng, 6, nsteps, frac=0.3)
        g = eng.generate_gibbs(x_seed, w, nsteps, roll, 1, 3, seed=seed)
        other = eng.generate_smc(x_seed, w, nsteps, roll, 1, seed=GR.sweep_seed(seed, 1))
        torch.cuda.synchronize()
        assert bool((g.log_evidence[:, 0] < -1e-3).all()), name
        assert not torch.equal(other.Xs[:, 0], g.Xs[:, 0]), name        # unpinned, sweep 1's key gives another path
        for s in (1, 2):
            assert torch.equal(g.Xs[:, s], g.Xs[:, 0]), (name, s)
            assert torch.equal(g.log_evidence[:, s], g.log_evidence[:, 0]), (name, s)
        assert not bool(g.renewed[:, 1:].any()) and bool(g.renewed[:, 0].all()), name


def test_graph_equals_eager_and_chunking_changes_nothing(dev, cases):
    rng = np.random.default_rng(11)
    nsteps, P, seed = 6, 8, 31                            # 48 rows, 8 per chunk of one melody: as tests/test_gpu_smc.py
    vb, _ = TS._vae(dev, B=16)
    for name, eng, x_seed, w in cases:
        roll = TS._roll(rng, 6, nsteps, frac=0.2)
        kw = dict(resample_threshold=0.6, seed=seed)
        a = eng.generate_gibbs(x_seed, w, nsteps, roll, P, 3, **kw)
        b = eng.generate_gibbs(x_seed, w, nsteps, roll, P, 3, use_graph=False, **kw)
        c = eng.generate_gibbs(x_seed, w, nsteps, roll, P, 3, chunk=1, **kw)
        torch.cuda.synchronize()
        assert _same(a, b), name
        assert _same(a, c), name
        if name == 'vae':                                 # the engine's batch size forces the chunks
            d = vb.generate_gibbs(x_seed, w, nsteps, roll, P, 3, **kw)
            assert _same(a, d), name


# ------------------------------------------------------------------ 3. every retained path obeys the constraints
def test_retained_paths_obey_roll_and_counts(dev, cases):
    from clvae_amd.engine_generate import Constraints
    rng = np.random.default_rng(13)
    nsteps, P, K = 6, 8, 4
    for name, eng, x_seed, w in cases:
        roll = TS._roll(rng, 6, nsteps, frac=0.1, on=0.2)
        roll[(roll == 1).cumsum(-1) > 3] = FREE           # at most 3 notes forced on: feasible under (3, 4)
        g = eng.generate_gibbs(x_seed, w, nsteps, roll, P, K, resample_threshold=0.6, seed=3)
        c = eng.generate_gibbs(x_seed, w, nsteps, Constraints.between(3, 4, roll=roll), P, K, resample_threshold=0.6, seed=3)
        torch.cuda.synchronize()
        for r in (g, c):
            Xs = r.Xs.cpu().numpy()
            assert set(np.unique(Xs)) <= {0.0, 1.0}, name
            forced = roll <= 1
            for s in range(K):
                assert np.all(Xs[:, s][forced] == roll[forced]), (name, s)
        n = c.Xs.sum(-1)
        assert bool(((n >= 3) & (n <= 4)).all()), name
        assert bool(torch.isfinite(c.log_evidence).all()) and bool(c.renewed[:, 1:].any()), name


# ------------------------------------------------------------------ 4. exactness on the enumerable models
def _check_gibbs_exactness(gen, xhat_of):
    """tests/test_gibbs_reference.py's check with its M, P = 2, tau and K: after K sweeps the marginals of every free note
    lie within 4 binomial standard errors of the enumerated posterior (the variance floored at 0.01 as in
    tests/test_gpu_smc.py: a marginal at 0 or 1 has no binomial error to measure in), and the sweep-0 paths of the same run,
    the plain filter at P = 2, miss one by more than 8.  Observed on an MI355X: cl_vrnn 1.12 after 64 sweeps against 126 for
    sweep 0, cl_vae 1.35 against 119."""
    M, P, K = TG.M, TG.P, TG.K
    Z, post, ancm = TS._exact(xhat_of)
    free = TS.ROLL01 > 1
    roll = np.full((M, TS.T4, D), FREE, np.uint8)
    roll[:, :, :2] = TS.ROLL01
    r = gen(roll, M, P, K)
    Xs = r.Xs.cpu().numpy()
    assert np.all(Xs[:, :, :, 2:] == 0) and np.all(Xs[:, :, :, :2][:, :, ~free] == TS.ROLL01[~free])
    sig = np.sqrt(np.maximum(post * (1 - post), 0.01) / M)
    err = lambda s: (np.abs(Xs[:, s, :, :2].mean(0) - post) / sig)[free]
    print("gibbs exactness: max error in standard errors, sweep 0: %.2f, sweep %d: %.2f; renewed per sweep %.3f"
          % (err(0).max(), K, err(K - 1).max(), float(r.renewed[:, 1:].float().mean())))
    assert err(K - 1).max() < 4, err(K - 1)
    assert err(0).max() > 8, err(0)
    ratio = np.exp(r.log_evidence[:, 0].cpu().numpy() - np.log(Z))      # sweep 0's evidence is the unbiased one
    assert abs(ratio.mean() - 1) < 4 * ratio.std() / np.sqrt(M) + 1e-9, (ratio.mean(), ratio.std())


def test_exact_posterior_on_enumerable_vrnn(dev):
    eng, p = TS._enumerable_vrnn(dev, B=4)

    def xhat_of(frames):
        n = frames.shape[0]
        inputs = np.concatenate([np.zeros((n, 1, D)), frames[:, :-1]], 1)
        return TS._vrnn_xhat_along(p, inputs, np.eye(10)[np.zeros(n, int)], 0, 2)

    def gen(roll, M, P, K):
        x_seed = torch.zeros(M, 0, D, device=dev)
        w = torch.as_tensor(np.eye(10, dtype=np.float32)[np.arange(M) % 10], device=dev)
        return eng.generate_gibbs(x_seed, w, TS.T4, roll, P, K, resample_threshold=TG.TAU, seed=41)

    _check_gibbs_exactness(gen, xhat_of)


def test_exact_posterior_on_enumerable_vae(dev):
    eng, p = TS._enumerable_vae(dev, B=TG.M * TG.P)

    def xhat_of(frames):
        n = frames.shape[0]
        return TS._vae_xhat_along(p, np.zeros((n, D)), frames, np.eye(4)[np.zeros(n, int)], 0, 3)

    def gen(roll, M, P, K):
        x_seed = torch.zeros(M, D, device=dev)
        w = torch.as_tensor(np.eye(4, dtype=np.float32)[np.arange(M) % 4], device=dev)
        return eng.generate_gibbs(x_seed, w, TS.T4, roll, P, K, resample_threshold=TG.TAU, seed=43)

    _check_gibbs_exactness(gen, xhat_of)


# ------------------------------------------------------------------ 5. the sample CLIs with --sweeps
@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_sweeps_cli_end_to_end(dev, tmp_path, capsys, monkeypatch, which):
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, GIBBS_FLAGS, HARMONIZE_FLAGS, parser_for
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    TR = importlib.import_module('clvae_amd.%s.train' % which)
    data = make_synthetic_pickle(str(tmp_path / "syn.pickle"), n_songs=(10, 4, 4), seed=1)
    mdir, sdir = str(tmp_path / "models"), str(tmp_path / "samples")
    os.makedirs(mdir); os.makedirs(sdir)
    extra = ['--latent_dim', '4', '--batch_size', '50'] if which == 'cl_vae' else ['--seq_length', '8', '--batch_size', '20']
    np.random.seed(0)
    TR.train(TR.build_parser().parse_args(['m', '--use_x_prev', '--num_epochs', '2', '--patience', '0', '--train_file', data,
                                           '--model_dir', mdir] + extra))
    parser = parser_for('%s.sample' % which, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS + GIBBS_FLAGS)
    args = parser.parse_args(['h', '-n', '3', '-t', '8', '--seed', '4', '-i', os.path.join(mdir, 'm.h5'), '--train_file', data,
                              '--sample_dir', sdir, '--harmonize', 'top', '--particles', '4', '--sweeps', '2'])
    seen = []
    real = S.harmonize

    def spy(model, seeds, sources, w_vals, **kw):
        seen.append((np.asarray(sources), kw))
        return real(model, seeds, sources, w_vals, **kw)
    monkeypatch.setattr(S, 'harmonize', spy)
    np.random.seed(3)
    capsys.readouterr()
    rolls = S.sample(args)
    printed = capsys.readouterr().out.splitlines()
    assert len(rolls) == 3 and len(seen) == 1
    assert seen[0][1]['particles'] == 4 and seen[0][1]['sweeps'] == 2 and seen[0][1]['return_renewed'] is True
    assert all(set(np.unique(r)) <= {0.0, 1.0} for r in rolls)
    assert sum('log p(voice) per frame' in line for line in printed) == 3
    lines = [line for line in printed if 'renewed per sweep' in line]
    assert len(lines) == 3
    for line in lines:                                   # sweep 0 renews everything; then one share per sweep
        shares = [float(v) for v in line.split('renewed per sweep')[1].split()]
        assert len(shares) == 2 and shares[0] == 1.0 and 0.0 <= shares[1] <= 1.0
    for roll, src in zip(rolls, seen[0][0]):              # the top voice of the source frames is kept
        for t in range(src.shape[0]):
            sn = np.nonzero(src[t])[0]
            if len(sn):
                g = np.nonzero(roll[t])[0]
                assert len(g) and g.max() == sn.max(), t
    files = os.listdir(sdir)
    for j in range(3):
        assert 'h_%d.mid' % j in files and open(os.path.join(sdir, 'h_%d.mid' % j), 'rb').read()[:4] == b'MThd'
