"""-m gpu: latent paths in and out on both routes: the ZO and ZG instances of the persistent kernels
(csrc/generate.hip, csrc/vae_generate.hip), the frame chains, clv_lerp_rows, morph(), the public calls and the sample tools'
--morph.  The reference is tests/latent_reference.py; the conditions on this file's inputs that need no device (flip cap,
float32 deviation of the latents, seeds of the keyed enumeration) are asserted in tests/test_latent_reference.py."""
import importlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import latent_reference as LR
import test_gpu_clamped_generation as TC
import vary_reference as VR
from helpers import write_jsb_pickle
from test_gpu_vary import _engine, _near_flip, _t, _vary

pytestmark = pytest.mark.gpu

FREE, D = 255, 88
ROUTES = ['persistent', 'chain']


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _vary_z(eng, dev, route, src, w_enc, w_dec=None, x0=None, **kw):
    """engine.vary with its latents: (Xs, x_hat, zout [3, N, T, L]) as device tensors, zout NaN-poisoned before the run"""
    N, Tn = np.shape(src)[:2]
    zout = torch.full((3, N, Tn, eng.cfg['L']), float('nan'), device=dev)
    Xs, xh = _vary(eng, dev, route, src, w_enc, w_dec, x0, zout=zout, **kw)
    assert not torch.isnan(zout).any()
    return Xs, xh, zout


def _decode(eng, dev, route, z, w_dec, x0=None, history='own', xhat=True, **kw):
    """engine.decode_latents by `route`: (Xs, x_hat) as device tensors; z, history numpy or device tensors"""
    z = z if isinstance(z, torch.Tensor) else _t(dev, z)
    hist = history if isinstance(history, (str, torch.Tensor)) else _t(dev, history)
    xh = torch.full((z.shape[0], z.shape[1], D), float('nan'), device=dev) if xhat else None
    use_graph = kw.pop('use_graph', True)
    Xs = eng.decode_latents(z, _t(dev, w_dec), x0=_t(dev, x0), history=hist, persistent=route == 'persistent', use_graph=use_graph,
                    xhat_out=xh, **kw)
    torch.cuda.synchronize()
    assert set(torch.unique(Xs).tolist()) <= {0.0, 1.0} and (xh is None or not torch.isnan(xh).any())
    return Xs, xh


def _case(which, L, gate, use_x_prev, dev):
    eng, p = _engine(dev, which, L, use_x_prev, gate)
    C = VR.classes_of(which)
    return (eng, p) + VR.case_inputs(LR.LATENT_N, LR.LATENT_T, C)


# ------------------------------------------------------------------ 1. latents out
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which,L,gate,use_x_prev", LR.LATENT_CASES)
def test_latents_out_match_the_fp64_reference(dev, which, L, gate, use_x_prev, route):
    """z_mean, z_log_var and z of every frame against the float64 reference, within LATENT_TOL = 2e-4: the bound
    tests/test_gpu_vary.py holds logits to (the same LSTM chain followed by an 88-long product).  The float32 numpy
    reference on the CPU uses under a tenth of it (tests/test_latent_reference.py), so the bound stands as it is.
    Measured on MI355X: 1.4e-7 .. 1.0e-6 over the twelve cases.  And storing the latents does not change Xs or
    x_hat by a bit."""
    eng, p, src, x0, w_enc, w_dec = _case(which, L, gate, use_x_prev, dev)
    kw = dict(history='own', seed=LR.LATENT_SEED, temperature=0.9, z_temperature=0.7)
    Xs, xh, zout = _vary_z(eng, dev, route, src, w_enc, w_dec, x0, **kw)
    z, zm, zlv = LR.encode(which, p, src, w_enc, seed=LR.LATENT_SEED, L=L, Tz=0.7, gate=gate)
    got = zout.cpu().numpy().astype(np.float64)
    errs = [float(np.abs(g - w).max()) for g, w in zip(got, (zm, zlv, z))]
    print("%s L=%d %s x_prev=%s %s: max |z_mean, z_log_var, z - fp64| = %.3e %.3e %.3e (bound %.0e)"
          % ((which, L, gate, use_x_prev, route) + tuple(errs) + (LR.LATENT_TOL,)))
    assert max(errs) < LR.LATENT_TOL
    X0, xh0 = _vary(eng, dev, route, src, w_enc, w_dec, x0, **kw)
    assert torch.equal(X0, Xs) and torch.equal(xh0, xh)


# ------------------------------------------------------------------ 2. the round trip
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("T,Tz", VR.FREE_RUN_TEMPS)
@pytest.mark.parametrize("which,L,gate,use_x_prev", LR.LATENT_CASES)
def test_decoding_the_latents_of_a_redecoding_gives_its_frames(dev, which, L, gate, use_x_prev, T, Tz, route):
    """decode(z of vary, w_dec, the same seed, x0, roll and temperature) equals that vary bit for bit, in Xs and x_hat, on
    each route against its own vary, under a 30 % roll and another decoder label"""
    eng, p, src, x0, w_enc, w_dec = _case(which, L, gate, use_x_prev, dev)
    clamp = VR.roll(LR.LATENT_N, LR.LATENT_T, seed=3)
    Xs, xh, zout = _vary_z(eng, dev, route, src, w_enc, w_dec, x0, history='own', seed=41, clamp=clamp, temperature=T,
                           z_temperature=Tz)
    Xd, xhd = _decode(eng, dev, route, zout[2].contiguous(), w_dec, x0, seed=41, clamp=clamp, temperature=T)
    assert torch.equal(Xd, Xs) and torch.equal(xhd, xh)
    TC._check_clamped(Xd, clamp)
    # and the path matters: another one gives other probabilities
    _, xo = _decode(eng, dev, route, (zout[2] + 0.5).contiguous(), w_dec, x0, seed=41, clamp=clamp, temperature=T)
    assert not torch.equal(xo, xh)


# ------------------------------------------------------------------ 3. the training identity
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which,L,gate,use_x_prev", LR.LATENT_CASES)
def test_teacher_forced_decode_of_the_encoders_z_is_the_training_forward_pass(dev, which, L, gate, use_x_prev, route):
    """history = sources, the encoder's own z, w_dec = w_enc: logits within LOGIT_TOL = 2e-4 of the float64 reference
    (measured on MI355X: 4.2e-7 .. 8.5e-7), compared on the logit side"""
    eng, p, src, x0, w_enc, _ = _case(which, L, gate, use_x_prev, dev)
    _, _, want = VR.vary(which, p, src, w_enc, None, x0=x0, history='source', seed=LR.LATENT_SEED, L=L, gate=gate)
    _, _, zout = _vary_z(eng, dev, route, src, w_enc, None, x0, history='source', seed=LR.LATENT_SEED)
    _, xh = _decode(eng, dev, route, zout[2].contiguous(), w_enc, x0, history=src, seed=LR.LATENT_SEED)
    err = np.abs(VR.logit_of(xh.cpu().numpy()) - want).max()
    print("%s L=%d %s x_prev=%s %s: max |logit - fp64| = %.3e (bound %.0e)" % (which, L, gate, use_x_prev, route, err, LR.LOGIT_TOL))
    assert err < LR.LOGIT_TOL
    if use_x_prev:                          # the history is read: the free-running decode sees other frames
        _, xo = _decode(eng, dev, route, zout[2].contiguous(), w_enc, x0, history='own', seed=LR.LATENT_SEED)
        assert torch.equal(xo[:, 0], xh[:, 0]) and not torch.equal(xo, xh)


# ------------------------------------------------------------------ 4. the free run on a path of one's own
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("T", [t for t, _ in VR.FREE_RUN_TEMPS])
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_free_run_on_a_random_path_matches_reference(dev, which, T, route):
    """a random path (not an encoder's) under a roll with about 30 % of the notes clamped: clamped notes exact; a free note
    differs from the fp64 reference only within window(T) of its probability; at most FLIP_CAP such flips (a condition on
    the inputs: tests/test_latent_reference.py)"""
    p, z, x0, w_dec, clamp, L, seed = LR.free_path_case(which)
    eng, p2 = _engine(dev, which, L)
    assert all(np.array_equal(p[k], p2[k]) for k in p)
    Xs, _ = _decode(eng, dev, route, z, w_dec, x0, seed=seed, clamp=clamp, temperature=T)
    fol = LR.Follow(Xs.cpu().numpy(), LR.window(T))
    LR.decode(which, p, z, w_dec, x0=x0, seed=seed, L=L, clamp=clamp, T=T, follow=fol)
    print("%s %s T=%g: %d flips, %d outside the window of %.1e, %d clamped notes wrong"
          % (which, route, T, fol.flips, fol.far, fol.win, fol.clamp_wrong))
    assert fol.clamp_wrong == 0
    assert fol.far == 0
    assert fol.flips <= LR.FLIP_CAP


# ------------------------------------------------------------------ 5. the routes
@pytest.mark.parametrize("with_hist", [False, True])
@pytest.mark.parametrize("Tn", [1, 2, 9])
@pytest.mark.parametrize("N", [1, 4, 300])
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_routes_agree(dev, which, N, Tn, with_hist):
    """the chain captured as a graph equals the chain run eagerly, bit for bit; the persistent kernel and the chain agree
    until a near flip.  N = 300 on the NaN-poisoned memory of the suite: more workgroups than one wave of launches"""
    L, C, seed = (2 if which == 'cl_vrnn' else 3), VR.classes_of(which), 11 + N + Tn
    eng, _ = _engine(dev, which, L, B=304)
    src, x0, _, w_dec = VR.case_inputs(N, Tn, C, data_seed=N + Tn)
    z = np.random.default_rng(N * 16 + Tn).standard_normal((N, Tn, L))
    clamp = VR.roll(N, Tn, seed=Tn)
    kw = dict(history=src if with_hist else 'own', seed=seed, clamp=clamp, temperature=0.8)
    x0[:, 40] = 1.0                         # a sounding note in every row
    Xp, xhp = _decode(eng, dev, 'persistent', z, w_dec, x0, **kw)
    Xg, xhg = _decode(eng, dev, 'chain', z, w_dec, x0, **kw)
    Xe, xhe = _decode(eng, dev, 'chain', z, w_dec, x0, use_graph=False, **kw)
    assert torch.equal(Xg, Xe) and torch.equal(xhg, xhe)
    if with_hist:                           # teacher forcing: no flip can part the routes, every frame's x_hat is comparable
        TC._check_clamped(Xp, clamp)
        assert float((xhp - xhg).abs().max()) < 2e-5 * 1.25
    else:
        _near_flip(dev, Xp, Xg, xhp, seed, clamp, VR.window(0.8))
        assert float((xhp[:, 0] - xhg[:, 0]).abs().max()) < 2e-5 * 1.25   # frame 0 has no history of samples: the same x_hat
    X0, xh0 = _decode(eng, dev, 'persistent', z, w_dec, None, **kw)        # x0 is read: the decoder's first history
    assert not torch.equal(xh0[:, 0], xhp[:, 0])


# ------------------------------------------------------------------ 6. noise_rows
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which,L", [('cl_vrnn', 2), ('cl_vrnn', 19), ('cl_vae', 3)])
def test_noise_rows(dev, which, L, route):
    N, Tn, C, seed = 6, 7, VR.classes_of(which), 29
    eng, _ = _engine(dev, which, L, gate='sigmoid' if L == 19 else 'hard_sigmoid')
    _, x0, _, w_dec = VR.case_inputs(N, Tn, C, data_seed=3)
    z = np.random.default_rng(5).standard_normal((N, Tn, L))
    clamp = VR.roll(N, Tn, seed=6)
    run = lambda i, nr: _decode(eng, dev, route, z[i], w_dec[i], x0[i], seed=seed, clamp=clamp[i], temperature=1.1, noise_rows=nr)
    ident = np.arange(N)
    base = run(ident, None)
    same = run(ident, ident)                                              # None is arange(N)
    assert torch.equal(base[0], same[0]) and torch.equal(base[1], same[1])
    i = np.array([3, 3, 1, 3, 0, 5])                                      # duplicated rows give duplicated frames ...
    dup = run(i, i)
    assert torch.equal(dup[0][0], dup[0][1]) and torch.equal(dup[0][0], dup[0][3])
    assert torch.equal(dup[1][0], dup[1][1]) and torch.equal(dup[1][0], dup[1][3])
    ix = torch.as_tensor(i, device=dev)
    assert torch.equal(dup[0], base[0][ix]) and torch.equal(dup[1], base[1][ix])          # ... those of the row they name
    perm = np.array([4, 2, 5, 0, 3, 1])                                   # a permuted batch with the permuted noise_rows
    got = run(perm, perm)
    px = torch.as_tensor(perm, device=dev)
    assert torch.equal(got[0], base[0][px]) and torch.equal(got[1], base[1][px])
    moved = run(perm, None)                                               # without them the uniforms are the position's
    assert not torch.equal(moved[0], base[0][px])
    far = run(ident, ident + 1000)                                        # a row number beyond the batch is a row like any
    assert not torch.equal(far[0], base[0]) and torch.equal(far[1][:, 0], base[1][:, 0])


# ------------------------------------------------------------------ 7. clv_lerp_rows
@pytest.mark.parametrize("n", [10, 18, 171])
@pytest.mark.parametrize("R", [1, 300])
def test_lerp_rows(dev, R, n):
    from clvae_amd.engine_generate import lerp_rows
    rng = np.random.default_rng(R + n)
    a = (rng.standard_normal((7, n)) * 3).astype(np.float32)
    b = (rng.standard_normal((5, n)) * 3).astype(np.float32)
    ia, ib = rng.integers(0, 7, R), rng.integers(0, 5, R)
    run = lambda al: lerp_rows(_t(dev, a), ia, _t(dev, b), ib, al).cpu().numpy()
    assert np.array_equal(run(np.zeros(R)), a[ia])                        # the end points are exact ...
    assert np.array_equal(run(np.ones(R)), b[ib])
    al = rng.random(R).astype(np.float32)
    al[:: 3] = (np.arange(len(al[:: 3])) % 9) / 8.0                        # ... among them the alphas of an 8-step morph
    got = run(al).astype(np.float64)
    want = LR.lerp_rows(a, ia, b, ib, al)
    bound = LR.lerp_bound(a, ia, b, ib)
    ratio = float((np.abs(got - want) / np.maximum(bound, 1e-300)).max())
    print("R=%d n=%d: max |got - fp64| / (2^-23 (|a| + |b|)) = %.3f" % (R, n, ratio))
    assert np.all(np.abs(got - want) <= bound)
    assert not np.array_equal(run(al), run(al[::-1].copy())) or R == 1     # alpha is per row


# ------------------------------------------------------------------ 8. morph
def _model(which, C=4, seed=1):
    M = importlib.import_module('clvae_amd.%s.model' % which)
    if which == 'cl_vrnn':
        model, _ = M.get_model(4, D, 88, 2, 8, C, True, 'adam', seed=seed)
    else:
        model, _ = M.get_model(4, D, (88, 2), (88, C), 'adam', use_x_prev=True, seed=seed)
    return M, model


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_morph_ends_are_redecodings_and_common_noise_is_shared(dev, which):
    from clvae_amd.morph import morph
    M, model = _model(which)
    K, pairs, Tn, C = 3, 2, 9, 4
    a, _, w_a, w_b = VR.case_inputs(pairs, Tn, C, data_seed=7)
    b = VR.case_inputs(pairs, Tn, C, data_seed=8)[0]
    kw = dict(seed=13, temperature=0.9, z_temperature=0.6)
    out = morph(model, a, b, steps=K, w_a=w_a, w_b=w_b, common_noise=False, **kw)
    assert out.shape == (pairs, K + 1, Tn, D) and out.dtype == np.float64 and set(np.unique(out)) <= {0.0, 1.0}
    R = pairs * (K + 1)
    for j in range(pairs):
        # row 0 of pair j is vary of a batch whose row j (K + 1) holds a, row `steps` one whose row j (K + 1) + K holds b
        for k, piece, w in ((0, a[j], w_a[j]), (K, b[j], w_b[j])):
            ref = M.vary_samples_device(model, np.repeat(piece[None], R, 0), np.repeat(w[None], R, 0), **kw)
            assert np.array_equal(out[j, k], ref[j * (K + 1) + k]), (j, k)
    assert not np.array_equal(out[0, 0], out[0, K])
    # identical pieces and labels under common noise: every row of a pair is the same
    same = morph(model, a, a, steps=K, w_a=w_a, w_b=w_a, common_noise=True, seed=13, temperature=0.9)
    assert all(np.array_equal(same[j, k], same[j, 0]) for j in range(pairs) for k in range(K + 1))
    assert not np.array_equal(same[0, 0], same[1, 0])
    indep = morph(model, a, a, steps=K, w_a=w_a, w_b=w_a, common_noise=False, seed=13, temperature=0.9)
    assert np.array_equal(indep[:, 0], same[:, 0]) and not np.array_equal(indep[0, 1], indep[0, 0])
    one = morph(model, a[0], b[0], steps=1, w_a=w_a[0], w_b=w_b[0])      # one pair given as [T, 88]
    assert one.shape == (1, 2, Tn, D)


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_morph_on_keyed_models_ends_in_w_b(dev, which):
    """the keyed enumerable models (z rows zero: only the label reaches the output), 4096 pairs of one source, one step: the
    frequencies of the 4^4 histories of the alpha = 1 rows follow w_b's enumeration within 4 binomial standard errors (the
    seeds are inputs: tests/test_latent_reference.py holds the reference's own sample to the same criterion)"""
    from clvae_amd.engine import VaeEngine, VrnnEngine
    from clvae_amd.morph import morph
    L, C = (2, 10) if which == 'cl_vrnn' else (3, 4)
    cfg, p, keys = VR.keyed_params(which)
    n = VR.KEYED_ROWS
    eng = (VrnnEngine if which == 'cl_vrnn' else VaeEngine)(cfg, 4, dev)
    eng.P.set_weights(p)

    class Model:
        engine = eng
    src = np.repeat(VR.keyed_source()[None], n, 0)
    label = lambda c: np.eye(C)[np.full(n, c)]
    for c in keys:
        want, _, _ = VR.enumerate_redecoding(which, p, L, C, keys[0], c)
        out = morph(Model(), src, src, steps=1, w_a=label(keys[0]), w_b=label(c), common_noise=False,
                    seed=LR.KEYED_MORPH_SEED[which], temperature=VR.KEYED_T)
        assert np.all(out[:, :, :, 2:] == 0)
        worst = VR.worst_cell(VR.history_counts(out[:, 1]), want, n)
        print("%s w_b=%d: worst history %.2f SE" % (which, c, worst))
        assert worst < 4
        for c2 in keys:                     # and the frequencies tell this key from the others
            if c2 != c:
                assert VR.worst_cell(VR.history_counts(out[:, 1]), VR.enumerate_redecoding(which, p, L, C, keys[0], c2)[0], n) > 4


# ------------------------------------------------------------------ 9. refusals through the C ABI, the public calls, the tools
def test_c_abi_refusals(dev):
    from clvae_amd import _lib, ops
    N, Tn = 2, 4
    nan, inf = float('nan'), float('inf')
    _, x0, _, w_dec = (_t(dev, a) for a in VR.case_inputs(N, Tn, 10))
    Xs = torch.zeros(N, Tn, D, device=dev)
    z2, z3 = torch.zeros(N, Tn, 2, device=dev), torch.zeros(N, Tn, 3, device=dev)
    eng, _ = _engine(dev, 'cl_vrnn', 2)
    P, off = eng.P, eng.off
    rows = lambda name, r: P.rows(P.params, name, r)

    def vrnn_call(inv_T=1.0, N=N, Tn=Tn, z=z2, w=w_dec, Xs=Xs):
        try:
            ops.vrnn_decode(N, Tn, D, 88, 2, 10, eng.gate_act, 1, z, x0, None, w, None, P.p('decoder_h/kernel'),
                            rows('decoder_h/kernel', off), rows('decoder_h/kernel', off + 2), P.p('decoder_h/bias'),
                            P.p('decoder_h/recurrent_kernel'), P.p('X_decoded_mean/kernel'), P.p('X_decoded_mean/bias'), Xs,
                            None, inv_T=inv_T)
        except _lib.ClvError as e:
            return str(e)
        return None
    ev, _ = _engine(dev, 'cl_vae', 3)
    Pv = ev.P
    w4 = _t(dev, np.eye(4)[[0, 1]])

    def vae_call(inv_T=1.0, N=N, Tn=Tn, z=z3, w=w4, Xs=Xs):
        try:
            ops.vae_decode(N, Tn, D, 88, 3, 4, True, 1, z, x0, None, w, None, Pv.p('decoder_h/kernel'), Pv.p('decoder_h/bias'),
                           Pv.p('x_decoded_mean/kernel'), Pv.p('x_decoded_mean/bias'), Xs, None, inv_T=inv_T)
        except _lib.ClvError as e:
            return str(e)
        return None
    for call in (vrnn_call, vae_call):
        assert call(1.25) is None and call(1.0) is None
        for kw in (dict(inv_T=0.0), dict(inv_T=-1.0), dict(inv_T=nan), dict(inv_T=inf), dict(N=0), dict(Tn=0), dict(N=-3),
                   dict(z=None), dict(w=None), dict(Xs=None), dict(N=2 ** 20, Tn=2 ** 11)):
            msg = call(**kw)
            assert msg is not None and '(-1)' in msg, (kw, msg)
    torch.cuda.synchronize()
    lib = _lib.lib()
    a = torch.zeros(2, 4, device=dev)
    i = torch.zeros(2, dtype=torch.int32, device=dev)
    al, out = torch.zeros(2, device=dev), torch.zeros(2, 4, device=dev)
    good = [a, i, a, i, al, out]
    for k in range(6):
        args = [ops._ptr(None if j == k else t) for j, t in enumerate(good)]
        assert lib.clv_lerp_rows(2, 4, *args, ops._stream()) == -1
    for R, n in ((0, 4), (2, 0), (-1, 4)):
        assert lib.clv_lerp_rows(R, n, *[ops._ptr(t) for t in good], ops._stream()) == -1
    # the Python layer refuses what the C side cannot see: a negative noise_rows entry
    with pytest.raises(ValueError):
        eng.decode_latents(z2, w_dec, noise_rows=[0, -1])


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_public_calls_return_float64_numpy(dev, which):
    from clvae_amd import morph as MO
    M, model = _model(which)
    C, L = 4, 2
    src, x0, w_enc, w_dec = VR.case_inputs(3, 11, C, data_seed=5)        # 11 frames: any length, not the training window's
    z, zm, zlv = M.encode_latents_device(model, src, w_enc, seed=3)
    assert all(x.dtype == np.float64 and x.shape == (3, 11, L) for x in (z, zm, zlv)) and not np.array_equal(z, zm)
    z0, zm0, _ = M.encode_latents_device(model, src, w_enc, seed=3, z_temperature=0.0)
    assert np.array_equal(z0, zm0) and np.array_equal(zm0, zm)
    Xs, xh, lat = M.vary_samples_device(model, src, w_enc, w_dec, x0=x0, seed=3, return_xhat=True, return_latents=True)
    assert all(np.array_equal(g, w) for g, w in zip(lat, (z, zm, zlv)))
    Xd, xhd = M.decode_latents_device(model, z, w_dec, x0=x0, seed=3, return_xhat=True)
    assert Xd.dtype == np.float64 and xhd.dtype == np.float64 and np.array_equal(Xd, Xs) and np.array_equal(xhd, xh)
    assert np.array_equal(MO.decode(model, z, w_dec, x0=x0, seed=3), Xs)
    np.random.seed(0)
    zi = MO.encode(model, src)[0]                                        # w inferred by the model's own w-encoder
    assert zi.shape == (3, 11, L)
    edited = MO.decode(model, z.mean(axis=0), w_dec[0], seed=3)          # an averaged path, one label row
    assert edited.shape == (1, 11, D) and set(np.unique(edited)) <= {0.0, 1.0}


@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_sample_tools_morph_end_to_end(dev, tmp_path, which):
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, HARMONIZE_FLAGS, MORPH_FLAGS, TEMPERATURE_FLAGS, VARY_FLAGS, parser_for
    from clvae_amd.utils import midi_utils
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    TRN = importlib.import_module('clvae_amd.%s.train' % which)
    data = write_jsb_pickle('all', str(tmp_path / "JSB Chorales_all.pickle"))
    mdir = str(tmp_path / "models")
    os.makedirs(mdir)
    extra = ['--latent_dim', '4'] if which == 'cl_vae' else ['--seq_length', '8']
    np.random.seed(0)
    TRN.train(TRN.build_parser().parse_args(['m', '--use_x_prev', '--num_epochs', '2', '--patience', '0', '--train_file', data,
                                             '--model_dir', mdir] + extra))
    parser = parser_for('%s.sample' % which, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS + TEMPERATURE_FLAGS + VARY_FLAGS + MORPH_FLAGS)
    outs = []
    for run in ('a', 'b'):
        sdir = str(tmp_path / run)
        os.makedirs(sdir)
        args = parser.parse_args(['v', '-n', '4', '-t', '8', '--seed', '4', '-i', os.path.join(mdir, 'm.h5'), '--train_file',
                                  data, '--sample_dir', sdir, '--morph', '4', '--temperature', '0.9', '--infer_w'])
        seen = []
        real = S.morph

        def spy(model, a, b, **kw):
            seen.append((np.asarray(a), np.asarray(b), kw))
            return real(model, a, b, **kw)
        S.morph = spy
        try:
            np.random.seed(3)
            rolls = S.sample(args)
        finally:
            S.morph = real
        assert len(rolls) == 2 and all(r.shape == (5, 8, D) and set(np.unique(r)) <= {0.0, 1.0} for r in rolls)
        assert len(seen) == 1 and seen[0][2]['steps'] == 4 and seen[0][2]['temperature'] == 0.9
        assert 'z_temperature' not in seen[0][2]                         # the posterior means are mixed
        files = sorted(os.listdir(sdir))
        assert files == sorted(['v_%d_%s.mid' % (j, s) for j in range(2) for s in ('a', 'b')]
                               + ['v_%d_morph%d.mid' % (j, k) for j in range(2) for k in range(5)])
        blobs = {f: open(os.path.join(sdir, f), 'rb').read() for f in files}
        assert all(b[:4] == b'MThd' for b in blobs.values())
        # utils/midi_utils writes MIDI and has no reader: every file is held to the bytes its writer gives for the roll
        for j in range(2):                                               # the _a / _b files are the pieces that were mixed
            for s, k in (('a', 0), ('b', 1)):
                midi_utils.write_sample(seen[0][k][j], sdir, 'check', True)
                assert open(os.path.join(sdir, 'check.mid'), 'rb').read() == blobs['v_%d_%s.mid' % (j, s)]
            for k in range(5):                                           # and the morph files the returned rolls
                midi_utils.write_sample(rolls[j][k], sdir, 'check', True)
                assert open(os.path.join(sdir, 'check.mid'), 'rb').read() == blobs['v_%d_morph%d.mid' % (j, k)]
        os.remove(os.path.join(sdir, 'check.mid'))
        outs.append(blobs)
    assert outs[0] == outs[1]                                           # the same --seed: identical bytes
