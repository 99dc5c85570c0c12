"""-m gpu: voice-count constraints: the two kernels of csrc/voices.hip against the fp64 reference
(tests/voices_reference.py), the frame chains and the particle filter of both engines around them, and exactness on the
enumerable models of tests/test_gpu_smc.py."""
import itertools
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_smc as TS
import voices_reference as VR
from helpers import make_synthetic_pickle
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


def _C():
    from clvae_amd.engine_generate import Constraints
    return Constraints


def _counts_ok(Xs, voices, roll=None):
    """every frame of Xs [N, T, D] has its count in its pair's range (free pairs aside) and honours the roll"""
    Xs = Xs.cpu().numpy() if isinstance(Xs, torch.Tensor) else np.asarray(Xs)
    n = Xs.sum(-1)
    lo, hi = voices[..., 0].astype(int), voices[..., 1].astype(int)
    free = (lo == 0) & (hi == 255)
    ok = bool(np.all(free | ((n >= lo) & (n <= hi)))) and set(np.unique(Xs)) <= {0.0, 1.0}
    if roll is not None:
        ok = ok and bool(np.all((roll > 1) | (Xs == roll)))
    return ok


def _pairs(N, T, lo, hi):
    return np.broadcast_to(np.array([lo, hi], np.uint8), (N, T, 2)).copy()


def _mixed_voices(rng, N, T):
    """pairs of several kinds, free frames mixed in"""
    kinds = [(4, 4), (3, 4), (1, 1), (0, 15), (0, 255), (2, 6)]
    return np.array([[kinds[i] for i in rng.integers(0, len(kinds), T)] for _ in range(N)], np.uint8)


def _thin_roll(rng, N, T, voices):
    """a roll that forces at most two notes on per frame (feasible with every pair of _mixed_voices but (1, 1): one there)"""
    roll = np.full((N, T, D), FREE, np.uint8)
    for n in range(N):
        for t in range(T):
            hi = int(voices[n, t, 1])
            idx = rng.permutation(D)
            k = int(rng.integers(0, min(hi, 2) + 1))
            roll[n, t, idx[:k]] = 1
            roll[n, t, idx[k:k + 12]] = 0
    return roll


# ------------------------------------------------------------------ 1. both kernels against the reference, direct inputs
@pytest.mark.parametrize("R,P", [(1, 1), (5, 1), (5, 5), (67, 1), (66, 11)])
@pytest.mark.parametrize("with_roll", [False, True])
def test_voices_kernels_against_reference(dev, R, P, with_roll):
    from clvae_amd import ops
    nsteps, S = 5, 2
    xhat, u, roll, voices = VR.kernel_case(R, P, nsteps, with_roll, seed=R + P)
    t = lambda a: None if a is None else torch.as_tensor(a, device=dev)
    p_d, u_d, c_d, v_d = t(xhat), t(u), t(roll), t(voices)
    f64 = dict(dtype=torch.float64, device=dev)
    for k in (0, 3, nsteps - 1, -1, -S, nsteps):          # returned steps; the bridge, a seed step, past the end
        rows = None if roll is None else np.repeat(roll[:, max(0, min(k, nsteps - 1))], P, axis=0)
        pairs = np.repeat(voices[:, max(0, min(k, nsteps - 1))], P, axis=0)
        x = torch.full((R, D), float('nan'), device=dev)
        ell, logb = torch.full((R,), float('nan'), **f64), torch.full((R,), float('nan'), **f64)
        hist = torch.full((nsteps, R, D), 7, dtype=torch.uint8, device=dev)
        ops.smc_sample_voices(R, D, P, nsteps, S, p_d, u_d, c_d, v_d, TS._counter(dev, S + k), x, ell, hist, logb)
        if P == 1:
            x1, logb1 = torch.full((R, D), float('nan'), device=dev), torch.full((R,), float('nan'), **f64)
            ops.bernoulli_sample_voices(R * D, D, nsteps, S, p_d, u_d, c_d, v_d, TS._counter(dev, S + k), x1, logb1)
        torch.cuda.synchronize()
        if P == 1:                                        # the chain's twin: the same frame, the same log B[0][0]
            assert torch.equal(x1, x) and torch.equal(logb1, logb)
        if 0 <= k < nsteps:
            want, want_ell, want_logb, margin = VR.sample_frame(xhat, u, rows, pairs)
            assert margin >= 1e-9                         # the reference alone: no note close enough to flip
            assert np.array_equal(x.cpu().numpy(), want)
            assert _counts_ok(x[:, None], pairs[:, None], None if rows is None else rows[:, None])
            np.testing.assert_allclose(logb.cpu().numpy(), want_logb, rtol=1e-12, atol=0)
            np.testing.assert_allclose(ell.cpu().numpy(), want_ell, rtol=1e-12, atol=0)
            h = hist.cpu().numpy()
            assert np.array_equal(h[k], want.astype(np.uint8)) and np.all(np.delete(h, k, axis=0) == 7)
        else:                                             # no constraint, no weight, no history
            assert np.array_equal(x.cpu().numpy(), (u <= xhat).astype(np.float32))
            assert torch.isnan(ell).all() and bool((hist == 7).all()) and bool((logb == 0).all())


def test_free_pairs_are_the_twins_bit_for_bit(dev):
    """an all-free voices array: x, ell and the history of clv_smc_sample, x of clv_bernoulli_sample_clamped"""
    from clvae_amd import ops
    rng = np.random.default_rng(11)
    G, P, nsteps, S, k = 6, 7, 3, 2, 1
    R = G * P
    xhat = rng.random((R, D)).astype(np.float32)
    xhat[:, :len(VR.SPECIAL)] = VR.SPECIAL
    u = rng.random((R, D)).astype(np.float32)
    roll = TS._roll(rng, G, nsteps, frac=0.5)
    t = lambda a: torch.as_tensor(a, device=dev)
    p_d, u_d, c_d, v_d = t(xhat), t(u), t(roll), t(_pairs(G, nsteps, 0, 255))
    out = []
    for voiced in (False, True):
        x = torch.full((R, D), float('nan'), device=dev)
        ell = torch.full((R,), float('nan'), dtype=torch.float64, device=dev)
        hist = torch.full((nsteps, R, D), 7, dtype=torch.uint8, device=dev)
        if voiced:
            ops.smc_sample_voices(R, D, P, nsteps, S, p_d, u_d, c_d, v_d, TS._counter(dev, S + k), x, ell, hist)
        else:
            ops.smc_sample(R, D, P, nsteps, S, p_d, u_d, c_d, TS._counter(dev, S + k), x, ell, hist)
        out.append((x, ell, hist))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*out))
    c_rows, v_rows = t(np.repeat(roll, P, axis=0)), t(_pairs(R, nsteps, 0, 255))
    xa, xb = torch.zeros(R, D, device=dev), torch.zeros(R, D, device=dev)
    ops.bernoulli_sample_clamped(R * D, D, nsteps, S, p_d, u_d, c_rows, TS._counter(dev, S + k), xa)
    ops.bernoulli_sample_voices(R * D, D, nsteps, S, p_d, u_d, c_rows, v_rows, TS._counter(dev, S + k), xb)
    torch.cuda.synchronize()
    assert torch.equal(xa, xb) and torch.equal(xa, out[0][0])


# ------------------------------------------------------------------ 2. bit-for-bit equivalences on the engines
def _engines(dev):
    (ev, pv), (ea, pa) = TS._vrnn(dev), TS._vae(dev, B=64)
    return [('cl_vrnn', ev, pv, 2, 10, 2), ('cl_vae', ea, pa, None, 4, 3)]        # name, engine, params, S, C, L


@pytest.mark.parametrize("use_graph", [True, False])
def test_voiceless_and_all_free_are_todays_calls(dev, use_graph):
    C = _C()
    for name, eng, _, S, Cn, _ in _engines(dev):
        N, nsteps, P, seed = 4, 5, 6, 17
        x_seed, w = TS._inputs(dev, N, S, Cn, 3)
        roll = TS._roll(np.random.default_rng(5), N, nsteps, frac=0.2)
        free = _pairs(N, nsteps, 0, 255)
        xh = [torch.zeros(N, nsteps, D, device=dev) for _ in range(3)]
        src = torch.as_tensor((np.random.default_rng(6).random((N, nsteps, D)) < 0.06).astype(np.float32), device=dev)
        kw = dict(seed=seed, use_graph=use_graph, persistent=False)
        a = eng.vary(src, w, clamp=roll, xhat_out=xh[0], **kw)
        b = eng.vary(src, w, clamp=C(roll), xhat_out=xh[1], **kw)
        c = eng.vary(src, w, clamp=C(roll, free), xhat_out=xh[2], **kw)
        assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(xh[0], xh[1]) and torch.equal(xh[0], xh[2]), name
        a = eng.generate(x_seed, w, nsteps, clamp=roll, **kw)
        assert torch.equal(a, eng.generate(x_seed, w, nsteps, clamp=C(roll), **kw)), name
        assert torch.equal(a, eng.generate(x_seed, w, nsteps, clamp=C(roll, free), **kw)), name
        assert torch.equal(eng.generate(x_seed, w, nsteps, **kw), eng.generate(x_seed, w, nsteps, clamp=C(None, free), **kw))
        skw = dict(resample_threshold=0.6, n_out=2, seed=seed, use_graph=use_graph)
        a = eng.generate_smc(x_seed, w, nsteps, roll, P, **skw)
        for other in (C(roll), C(roll, free)):
            b = eng.generate_smc(x_seed, w, nsteps, other, P, **skw)
            assert TS._same(a, b), name                  # Xs, log_evidence, ess, resamples
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 3. constraints are honoured; 4. teacher forcing
def test_every_route_honours_counts_and_roll(dev):
    C = _C()
    rng = np.random.default_rng(21)
    for name, eng, _, S, Cn, L in _engines(dev):
        N, nsteps, seed = 5, 6, 29
        voices = _mixed_voices(rng, N, nsteps)
        roll = _thin_roll(rng, N, nsteps, voices)
        for con, r in ((C(roll, voices), roll), (C(None, voices), None), (C.between(3, 4), None), (C.exactly(4, roll=None), None)):
            vv = voices if isinstance(con.voices, np.ndarray) else _pairs(N, nsteps, *con.voices)
            for S_ in ({0, S} if S is not None else {None}):
                x_seed, w = TS._inputs(dev, N, S_, Cn, 7)
                a = eng.generate(x_seed, w, nsteps, seed=seed, clamp=con, persistent=True)
                b = eng.generate(x_seed, w, nsteps, seed=seed, clamp=con, persistent=False)
                assert torch.equal(a, b) and _counts_ok(a, vv, r), (name, S_)
                g = eng.generate_smc(x_seed, w, nsteps, con, 8, n_out=2, seed=seed)
                assert _counts_ok(g.Xs[:, 0], vv, r) and _counts_ok(g.Xs[:, 1], vv, r), (name, S_)
                assert np.all(np.isfinite(g.log_evidence.cpu().numpy()))
            src = torch.as_tensor((rng.random((N, nsteps, D)) < 0.06).astype(np.float32), device=dev)
            zout = torch.zeros(3, N, nsteps, L, device=dev)
            a = eng.vary(src, w, seed=seed, clamp=con, zout=zout)
            assert torch.equal(a, eng.vary(src, w, seed=seed, clamp=con, persistent=False)) and _counts_ok(a, vv, r), name
            d = eng.decode_latents(zout[2].contiguous(), w, seed=seed, clamp=con)
            assert torch.equal(a, d), name                   # the path of a re-decoding decodes to its frames


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_stream_chunks_carry_the_counts(dev, which):
    """generate_chunked slices the counts with the roll: the frames of the one call, every chunk boundary included"""
    import importlib
    from clvae_amd.stream import generate_chunked
    C = _C()
    M = importlib.import_module('clvae_amd.%s.model' % which)
    rng = np.random.default_rng(2)
    N, nsteps = 3, 7
    if which == 'cl_vrnn':
        model, _ = M.get_model(4, 88, 88, 2, 8, 3, True, 'adam', seed=1)
        seeds = (rng.random((N, 2, 88)) < 0.06).astype(np.float64)
    else:
        model, _ = M.get_model(4, 88, (88, 2), (88, 3), 'adam', use_x_prev=True, seed=1)
        seeds = (rng.random((N, 88)) < 0.06).astype(np.float64)
    w = np.eye(3)[[0, 1, 2]]
    voices = _mixed_voices(rng, N, nsteps)
    roll = _thin_roll(rng, N, nsteps, voices)
    con = C(roll, voices)
    one = M.generate_samples_device(model, seeds, nsteps, w, seed=5, clamp=con)
    parts = generate_chunked(model, seeds, nsteps, w, chunk=3, seed=5, clamp=con)
    assert np.array_equal(one, parts) and _counts_ok(one, voices, roll)


def test_morph_rows_carry_their_pairs_counts(dev):
    """morph(clamp=Constraints over the pairs): every row of a pair is decoded under the pair's roll and counts"""
    from clvae_amd.cl_vrnn import model as M
    from clvae_amd.morph import morph
    C = _C()
    rng = np.random.default_rng(3)
    model, _ = M.get_model(4, 88, 88, 2, 8, 3, True, 'adam', seed=1)
    pairs, T, K = 2, 5, 3
    a, b = ((rng.random((pairs, T, D)) < 0.06).astype(np.float64) for _ in range(2))
    voices = _mixed_voices(rng, pairs, T)
    roll = _thin_roll(rng, pairs, T, voices)
    w = np.eye(3)[[0, 1]]
    out = morph(model, a, b, steps=K, w_a=w, w_b=w[::-1], seed=7, clamp=C(roll, voices))
    assert out.shape == (pairs, K + 1, T, D)
    for k in range(K + 1):
        assert _counts_ok(out[:, k], voices, roll), k
    assert np.all(morph(model, a, b, steps=K, w_a=w, w_b=w, seed=7, clamp=C.exactly(3)).sum(-1) == 3)


def test_teacher_forcing_reproduces_every_frame(dev):
    """the frames of a constrained re-decoding are the reference's draw from the returned x_hat and the uniforms of Philox
    stream 1 at (step = frame, index = row * D + note); teacher-forcing the frames on their path gives the same x_hat"""
    C = _C()
    rng = np.random.default_rng(31)
    for name, eng, _, _, Cn, L in _engines(dev):
        N, T, seed = 6, 5, 37
        voices = _mixed_voices(rng, N, T)
        roll = _thin_roll(rng, N, T, voices)
        con = C(roll, voices)
        _, w = TS._inputs(dev, N, None, Cn, 9)
        src = torch.as_tensor((rng.random((N, T, D)) < 0.06).astype(np.float32), device=dev)
        xh, xh2 = torch.zeros(N, T, D, device=dev), torch.zeros(N, T, D, device=dev)
        zout = torch.zeros(3, N, T, L, device=dev)
        Xs = eng.vary(src, w, seed=seed, clamp=con, xhat_out=xh, zout=zout)
        again = eng.decode_latents(zout[2].contiguous(), w, history=Xs, seed=seed, clamp=con, xhat_out=xh2)
        torch.cuda.synchronize()
        assert torch.equal(again, Xs) and torch.equal(xh, xh2), name
        u = np.stack([OP.uniform(N * D, seed, step=t, stream_id=1).reshape(N, D) for t in range(T)], axis=1)
        want, _, margin = VR.frames(xh.cpu().numpy(), u, roll, voices)
        assert margin >= 1e-9, (name, margin)
        assert np.array_equal(Xs.cpu().numpy(), want), name


# ------------------------------------------------------------------ 5 / 6. exactness on the enumerable models
T4 = TS.T4
# exactly one voice per frame and a note forced on in frame 2 that the model's own run makes unlikely there (cl_vrnn
# alternates note 0, note 1, note 0: note 1 is forced; cl_vae plays note 0 twice, then note 1: note 0 is forced), so the
# filter must move the earlier frames, which constrained ancestral sampling leaves where they were
ROLLV = {'cl_vrnn': np.array([[FREE, FREE], [FREE, FREE], [FREE, 1], [FREE, FREE]], np.uint8),
         'cl_vae': np.array([[FREE, FREE], [FREE, FREE], [1, FREE], [FREE, FREE]], np.uint8)}
OTHERS = 86e-7          # the enumeration treats notes 2..87 as off: each has q = 1e-7 (the clip), so a frame's single voice
                        # is one of them with probability below 86e-7 / P(count = 1) -- about 88e-7 per frame


def _exact_one_voice(xhat_of, roll01):
    """enumerate the histories of notes 0 / 1 with exactly one of them per frame: p(roll and counts), the exact posterior
    marginals and those of constrained ancestral sampling [T4, 2]"""
    hs = np.array(list(itertools.product((0.0, 1.0), repeat=2 * T4))).reshape(-1, T4, 2)
    frames = np.zeros((len(hs), T4, D))
    frames[:, :, :2] = hs
    xh = xhat_of(frames)[:, :, :2]
    bern = np.where(hs == 1, xh, 1 - xh)
    clamped = roll01 <= 1
    ok = np.all(~clamped[None] | (hs == roll01[None]), axis=(1, 2)) & np.all(hs.sum(-1) == 1, axis=1)
    joint = np.prod(bern, axis=(1, 2)) * ok
    # ancestral: each frame drawn from p(frame | its roll row, count = 1) given the past
    allowed = [[h for h in ((1.0, 0.0), (0.0, 1.0)) if all(c > 1 or h[i] == c for i, c in enumerate(roll01[t]))]
               for t in range(T4)]
    anc = np.zeros(len(hs))
    for i in np.nonzero(ok)[0]:
        pr = 1.0
        for t in range(T4):
            num = np.prod(bern[i, t])
            den = sum(np.prod(np.where(np.array(h) == 1, xh[i, t], 1 - xh[i, t])) for h in allowed[t])
            pr *= num / den
        anc[i] = pr
    Z = joint.sum()
    return Z, (joint[:, None, None] * hs).sum(0) / Z, (anc[:, None, None] * hs).sum(0) / anc.sum()


def _xhat_of(which, p):
    if which == 'cl_vrnn':
        def f(frames):
            n = frames.shape[0]
            inputs = np.concatenate([np.zeros((n, 1, D)), frames[:, :-1]], 1)
            return TS._vrnn_xhat_along(p, inputs, np.eye(10)[np.zeros(n, int)], 0, 2)
    else:
        def f(frames):
            n = frames.shape[0]
            return TS._vae_xhat_along(p, np.zeros((n, D)), frames, np.eye(4)[np.zeros(n, int)], 0, 3)
    return f


def _enumerable(dev, which, B):
    if which == 'cl_vrnn':
        eng, p = TS._enumerable_vrnn(dev, B=4)
        seed_of = lambda n: torch.zeros(n, 0, D, device=dev)
        w_of = lambda n: torch.as_tensor(np.eye(10, dtype=np.float32)[np.arange(n) % 10], device=dev)
    else:
        eng, p = TS._enumerable_vae(dev, B=B)
        seed_of = lambda n: torch.zeros(n, D, device=dev)
        w_of = lambda n: torch.as_tensor(np.eye(4, dtype=np.float32)[np.arange(n) % 4], device=dev)
    return eng, p, seed_of, w_of


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_exact_count_frequencies(dev, which):
    """65536 sequences of 4 frames under exactly(1): the frequencies of notes 0 and 1 per frame against the enumerated
    conditional chain, within 4 standard errors (plus OTHERS, far below them)"""
    C = _C()
    n, chunk = 65536, 4096
    eng, p, seed_of, w_of = _enumerable(dev, which, chunk)
    free01 = np.full((T4, 2), FREE, np.uint8)
    _, _, want = _exact_one_voice(_xhat_of(which, p), free01)
    tot = np.zeros((T4, 2))
    for i in range(n // chunk):                        # the Philox keys follow the row: another seed, other draws
        Xs = eng.generate(seed_of(chunk), w_of(chunk), T4, seed=100 + i, clamp=C.exactly(1), persistent=False)
        assert bool((Xs.sum(-1) == 1).all())
        tot += Xs[:, :, :2].sum(0).cpu().numpy()
    freq = tot / n
    se = np.sqrt(np.maximum(want * (1 - want), 1e-4) / n)
    print(which, 'frequencies', freq.round(4).tolist(), 'enumerated', want.round(4).tolist(), 'se', se.max(), 'others', OTHERS)
    assert np.all(np.abs(freq - want) < 4 * se + OTHERS), (freq, want)


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_filter_evidence_and_posterior_under_counts(dev, which):
    """256 melodies x 64 particles under exactly(1) and a late forced note: the enumerated evidence and posterior marginals
    within 4 standard errors; one particle (constrained ancestral sampling) is far off"""
    C = _C()
    G, P = 256, 64
    eng, p, seed_of, w_of = _enumerable(dev, which, 4096)
    rollv = ROLLV[which]
    Z, post, ancm = _exact_one_voice(_xhat_of(which, p), rollv)
    free = rollv > 1
    assert np.abs(post - ancm)[free].max() >= 0.1
    roll = np.full((G, T4, D), FREE, np.uint8)
    roll[:, :, :2] = rollv
    con = C.exactly(1, roll=roll)
    r = eng.generate_smc(seed_of(G), w_of(G), T4, con, P, seed=47)
    Xs, logZ = r.Xs[:, 0].cpu().numpy(), r.log_evidence.cpu().numpy()
    assert np.all(Xs.sum(-1) == 1) and np.all(Xs[:, :, :2][:, ~free] == rollv[~free])
    ratio = np.exp(logZ - np.log(Z))
    assert abs(ratio.mean() - 1) < 4 * ratio.std() / np.sqrt(G) + T4 * OTHERS, (ratio.mean(), ratio.std())
    sig = np.sqrt(np.maximum(post * (1 - post), 0.01) / G)
    m = Xs[:, :, :2].mean(0)
    assert np.all(np.abs(m - post)[free] < 4 * sig[free] + OTHERS), (m, post)
    m1 = eng.generate_smc(seed_of(G), w_of(G), T4, con, 1, seed=47).Xs[:, 0, :, :2].cpu().numpy().mean(0)
    assert np.abs(m1 - post)[free].max() > 4 * sig[free][np.argmax(np.abs(m1 - post)[free])]


def test_one_particle_is_constrained_generation_and_evidence_is_the_sum_of_ell(dev):
    C = _C()
    rng = np.random.default_rng(41)
    for name, eng, _, S, Cn, L in _engines(dev):
        N, nsteps, seed = 5, 6, 53
        voices = _mixed_voices(rng, N, nsteps)
        roll = _thin_roll(rng, N, nsteps, voices)
        con = C(roll, voices)
        x_seed, w = TS._inputs(dev, N, S, Cn, 11)
        ref = eng.generate(x_seed, w, nsteps, seed=seed, clamp=con)
        r = eng.generate_smc(x_seed, w, nsteps, con, 1, seed=seed)
        assert torch.equal(r.Xs[:, 0], ref), name
        assert int(r.resamples.sum()) == 0 and bool((r.ess == 1.0).all())
        # the path's x_hat: teacher-force it (cl_vae: vary's decoder history is the frame before, generate's the one
        # before that, so the chain is rebuilt from generate itself with the path as its roll)
        full = ref.to(torch.uint8).contiguous()
        xh = _path_xhat(eng, name, x_seed, w, nsteps, seed, full, dev)
        _, ell, margin = VR.frames(xh, _uniforms(N, nsteps, seed, S or 0), roll, voices)
        np.testing.assert_allclose(r.log_evidence.cpu().numpy(), ell.sum(1), rtol=1e-12, atol=0)


def _uniforms(N, nsteps, seed, S):
    return np.stack([OP.uniform(N * D, seed, step=S + t, stream_id=1).reshape(N, D) for t in range(nsteps)], axis=1)


def _path_xhat(eng, name, x_seed, w, nsteps, seed, full, dev):
    """the float32 x_hat of every returned frame along the path `full` (uint8 [N, nsteps, D], used as a roll that forces
    every note): the chain's own probabilities, read frame by frame"""
    from clvae_amd import engine_generate as EG
    N = full.shape[0]
    out = torch.zeros(N, nsteps, D, device=dev)
    if name == 'cl_vrnn':
        S = int(x_seed.shape[1])
        chain = EG._Chain(EG._VrnnRows(eng, N), w, w, nsteps, seed, None, 'shared', seed_frames=x_seed, clamp=full, S=S)
        chain.run(S + nsteps, False, lambda t: out[:, t - S].copy_(chain.rows.xhat[:N]) if t >= S else None)
    else:
        chain = EG._Chain(EG._VaeRows(eng, N), w, w, nsteps, seed, None, 'enc_input', x_enc=x_seed.clone(),
                          x_dec=x_seed.clone(), clamp=full)
        chain.run(nsteps, False, lambda t: out[:, t].copy_(chain.rows.xhat[:N]))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_filter_chunking_and_graph_change_nothing(dev):
    C = _C()
    rng = np.random.default_rng(43)
    for name, eng, _, S, Cn, _ in _engines(dev):
        N, nsteps, P, seed = 6, 5, 8, 59
        voices = _mixed_voices(rng, N, nsteps)
        con = C(_thin_roll(rng, N, nsteps, voices), voices)
        x_seed, w = TS._inputs(dev, N, S, Cn, 13)
        kw = dict(resample_threshold=0.9, n_out=3, seed=seed)
        a = eng.generate_smc(x_seed, w, nsteps, con, P, **kw)
        b = eng.generate_smc(x_seed, w, nsteps, con, P, use_graph=False, **kw)
        c = eng.generate_smc(x_seed, w, nsteps, con, P, chunk=1, **kw)
        torch.cuda.synchronize()
        assert TS._same(a, b) and TS._same(a, c), name
        assert int(a.resamples.sum()) > 0, name


# ------------------------------------------------------------------ 7. refusals
def test_refusals(dev):
    from clvae_amd import _lib, ops
    C = _C()
    eng, _ = TS._vrnn(dev)
    N, S, nsteps = 2, 1, 3
    x_seed, w = TS._inputs(dev, N, S, 10, 1)
    roll = np.full((N, nsteps, D), FREE, np.uint8)
    roll[1, 2, :5] = 1
    bad = [C(roll, _pairs(N, nsteps, 0, 4)),               # five forced on, hi = 4
           C(None, _pairs(N, nsteps, 5, 3)), C(None, _pairs(N, nsteps, 0, 16)), C(None, _pairs(N + 1, nsteps, 1, 1)),
           C(None, _pairs(N, nsteps, 1, 1).astype(np.int32))]
    allbut = np.zeros((N, nsteps, D), np.uint8)
    allbut[:, :, :2] = FREE
    bad.append(C(allbut, _pairs(N, nsteps, 3, 4)))         # two free notes, lo = 3
    for con in bad:
        for call in (lambda: eng.generate(x_seed, w, nsteps, clamp=con),
                     lambda: eng.generate_smc(x_seed, w, nsteps, con, 4)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        eng.generate_smc(x_seed, w, nsteps, C(), 4)
    p = torch.zeros(4, D, device=dev)
    v = torch.zeros(4, 2, 2, dtype=torch.uint8, device=dev)
    c = TS._counter(dev, 0)
    with pytest.raises(_lib.ClvError):
        ops.bernoulli_sample_voices(4 * D, D, 2, 0, p, p, None, None, c, p)
    with pytest.raises(_lib.ClvError):
        ops.bernoulli_sample_voices(4 * 129, 129, 2, 0, p, p, None, v, c, p)
    with pytest.raises(_lib.ClvError):
        ops.smc_sample_voices(4, D, 3, 2, 0, p, p, None, v, c, p, torch.zeros(4, dtype=torch.float64, device=dev),
                              torch.zeros(2, 4, D, dtype=torch.uint8, device=dev))


# ------------------------------------------------------------------ 8. the sample CLIs with --voices
@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_voices_cli_end_to_end(dev, tmp_path, capsys, which):
    import importlib
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, HARMONIZE_FLAGS, VOICES_FLAGS, parser_for
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    TR = importlib.import_module('clvae_amd.%s.train' % which)
    data = make_synthetic_pickle(str(tmp_path / "syn.pickle"), n_songs=(10, 4, 4), seed=1)
    mdir, sdir = str(tmp_path / "models"), str(tmp_path / "samples")
    os.makedirs(mdir); os.makedirs(sdir)
    extra = ['--latent_dim', '4', '--batch_size', '50'] if which == 'cl_vae' else ['--seq_length', '8', '--batch_size', '20']
    np.random.seed(0)
    TR.train(TR.build_parser().parse_args(['m', '--use_x_prev', '--num_epochs', '2', '--patience', '0', '--train_file', data,
                                           '--model_dir', mdir] + extra))
    parser = parser_for('%s.sample' % which, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS + VOICES_FLAGS)
    common = ['h', '-n', '3', '-t', '8', '--seed', '4', '-i', os.path.join(mdir, 'm.h5'), '--train_file', data,
              '--sample_dir', sdir]
    for more in ([], ['--particles', '8']):
        np.random.seed(3)
        rolls = S.sample(parser.parse_args(common + ['--harmonize', 'top', '--voices', '4'] + more))
        assert len(rolls) == 3
        for r in rolls:
            assert set(np.unique(r)) <= {0.0, 1.0} and np.all(r.sum(-1) == 4)
    capsys.readouterr()
