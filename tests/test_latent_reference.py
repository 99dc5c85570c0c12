"""CPU: the reference of latent paths in and out (tests/latent_reference.py): decoding an encoded path IS the
re-decoding of tests/vary_reference.py, a teacher-forced decode of the oracle's z is the oracle's forward pass, noise_rows,
the end points of lerp_rows, and the conditions on the inputs of tests/test_gpu_latent.py that need no device."""
import numpy as np
import pytest

import clvae_amd  # noqa: F401  (puts the package on the path the way the other reference tests do)
import latent_reference as LR
import vary_reference as VR
from oracle import clvae_oracle as O
from oracle import philox as OP

D = 88


def _case(which, L=None, use_x_prev=True, gate='hard_sigmoid', N=4, Tn=6):
    C = VR.classes_of(which)
    L = L or (2 if which == 'cl_vrnn' else 3)
    _, p = VR.case_params(which, L, C, use_x_prev, gate)
    return (p, L) + VR.case_inputs(N, Tn, C)


# ------------------------------------------------------------------------------- the two halves make the whole
@pytest.mark.parametrize("T,Tz", VR.FREE_RUN_TEMPS)
@pytest.mark.parametrize("history", ['own', 'source'])
@pytest.mark.parametrize("which,L,gate,use_x_prev", VR.IDENTITY_CASES)
def test_decode_of_the_encoded_path_is_vary_exactly(which, L, gate, use_x_prev, history, T, Tz):
    C = VR.classes_of(which)
    _, p = VR.case_params(which, L, C, use_x_prev, gate or 'hard_sigmoid')
    src, x0, w_enc, w_dec = VR.case_inputs(4, 6, C)
    clamp = VR.roll(4, 6, seed=2)
    want = VR.vary(which, p, src, w_enc, w_dec, x0=x0, history=history, seed=9, L=L, clamp=clamp, T=T, Tz=Tz, gate=gate)
    z, zm, zlv = LR.encode(which, p, src, w_enc, seed=9, L=L, Tz=Tz, gate=gate)
    got = LR.decode(which, p, z, w_dec, x0=x0, history='own' if history == 'own' else src, seed=9, L=L, clamp=clamp, T=T,
                    gate=gate)
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert z.shape == zm.shape == zlv.shape == (4, 6, L)
    z0, zm0, _ = LR.encode(which, p, src, w_enc, seed=9, L=L, Tz=0.0, gate=gate)
    assert np.array_equal(z0, zm0) and np.array_equal(zm0, zm)             # Tz = 0: the mean; the mean does not move with Tz
    assert not np.array_equal(LR.encode(which, p, src, w_dec, seed=9, L=L, Tz=Tz, gate=gate)[1], zm)      # w_enc reaches it


# ------------------------------------------------------------------------ the training forward pass of the oracle
def _given_label(monkeypatch, W):
    """the oracle's forward passes sample their label; here it is given (oracle/ stays as it is)"""
    monkeypatch.setattr(O, 'logistic_normal', lambda mean, log_var, eps: W)


@pytest.mark.parametrize("gate,use_x_prev,L", [('hard_sigmoid', True, 2), ('sigmoid', False, 2), ('sigmoid', True, 19)])
def test_teacher_forced_decode_of_the_oracles_z_is_vrnn_forward(monkeypatch, gate, use_x_prev, L):
    C, N, seed = 10, 4, 12
    cfg, p = VR.case_params('cl_vrnn', L, C, use_x_prev, gate)
    Tn = cfg['T']
    src, x0, w_enc, _ = VR.case_inputs(N, Tn, C)
    p64 = {k: np.asarray(v, np.float64) for k, v in p.items()}
    eps_Z = np.stack([OP.normal(N * L, seed, step=t, stream_id=0).reshape(N, L).astype(np.float64) for t in range(Tn)], 1)
    Xp = np.concatenate([x0[:, None], src[:, :-1]], 1)
    _given_label(monkeypatch, w_enc)
    c = O.vrnn_forward(p64, cfg, src, Xp, np.zeros((N, C - 1)), eps_Z)
    _, xh, lg = LR.decode('cl_vrnn', p, c['Z'], w_enc, x0=x0, history=src, seed=seed, L=L, gate=gate)
    np.testing.assert_allclose(lg, c['logits'], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(xh, c['X_hat'], rtol=1e-12, atol=0)
    z, zm, zlv = LR.encode('cl_vrnn', p, src, w_enc, seed=seed, L=L, gate=gate)             # and the encoder half
    np.testing.assert_allclose(zm, c['Z_mean'], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(zlv, c['Z_log_var'], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(z, c['Z'], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("use_x_prev,L", [(True, 3), (False, 8)])
def test_teacher_forced_decode_of_the_oracles_z_is_vae_forward(monkeypatch, use_x_prev, L):
    C, N, Tn, seed = 4, 5, 6, 12
    cfg, p = VR.case_params('cl_vae', L, C, use_x_prev)
    src, x0, w_enc, _ = VR.case_inputs(N, Tn, C)
    p64 = {k: np.asarray(v, np.float64) for k, v in p.items()}
    _given_label(monkeypatch, w_enc)
    cs = []
    for t in range(Tn):
        eps_z = OP.normal(N * L, seed, step=t, stream_id=0).reshape(N, L).astype(np.float64)
        cs.append(O.vae_forward(p64, cfg, src[:, t], x0 if t == 0 else src[:, t - 1], np.zeros((N, C - 1)), eps_z))
    Z = np.stack([c['z'] for c in cs], 1)
    _, xh, lg = LR.decode('cl_vae', p, Z, w_enc, x0=x0, history=src, seed=seed, L=L)
    np.testing.assert_allclose(lg, np.stack([c['logits'] for c in cs], 1), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(xh, np.stack([c['x_hat'] for c in cs], 1), rtol=1e-12, atol=0)
    z, zm, zlv = LR.encode('cl_vae', p, src, w_enc, seed=seed, L=L)
    np.testing.assert_allclose(z, Z, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(zm, np.stack([c['z_mean'] for c in cs], 1), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(zlv, np.stack([c['z_log_var'] for c in cs], 1), rtol=1e-12, atol=1e-12)


# -------------------------------------------------------------------------------------------------- noise_rows
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_noise_rows(which):
    p, L, src, x0, w_enc, w_dec = _case(which, N=5)
    z, _, _ = LR.encode(which, p, src, w_enc, seed=2, L=L)
    clamp = VR.roll(5, 6, seed=4)
    kw = dict(seed=6, L=L, T=0.8)
    base = LR.decode(which, p, z, w_dec, x0=x0, clamp=clamp, **kw)
    # None is arange(N)
    same = LR.decode(which, p, z, w_dec, x0=x0, clamp=clamp, noise_rows=np.arange(5), **kw)
    assert all(np.array_equal(a, b) for a, b in zip(base, same))
    # equal rows (inputs and noise_rows entry) give equal frames, and they are row 3's frames of the base run
    i = np.array([3, 3, 1, 3, 0])
    dup = LR.decode(which, p, z[i], w_dec[i], x0=x0[i], clamp=clamp[i], noise_rows=i, **kw)
    assert np.array_equal(dup[0][0], dup[0][1]) and np.array_equal(dup[0][0], dup[0][3])
    # a row moved to another position with its noise_rows entry keeps its frames (here: every row of a permutation)
    assert all(np.array_equal(a, b[i]) for a, b in zip(dup, base))
    # and without its entry it does not: the uniforms are the position's
    moved = LR.decode(which, p, z[i], w_dec[i], x0=x0[i], clamp=clamp[i], **kw)
    assert not np.array_equal(moved[0], base[0][i])
    # shared uniforms alone do not make rows equal
    shared = LR.decode(which, p, z, w_dec, x0=x0, clamp=clamp, noise_rows=np.zeros(5, int), **kw)
    assert not np.array_equal(shared[0][0], shared[0][1])


# --------------------------------------------------------------------------------------------------- lerp_rows
def test_lerp_rows_end_points_are_exact():
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal((4, 18)), rng.standard_normal((3, 18))
    ia, ib = np.array([0, 3, 3, 1, 2]), np.array([2, 0, 0, 1, 1])
    assert np.array_equal(LR.lerp_rows(a, ia, b, ib, np.zeros(5)), a[ia])
    assert np.array_equal(LR.lerp_rows(a, ia, b, ib, np.ones(5)), b[ib])
    al = np.array([0.0, 0.125, 0.5, 0.75, 1.0])
    np.testing.assert_allclose(LR.lerp_rows(a, ia, b, ib, al), (1 - al[:, None]) * a[ia] + al[:, None] * b[ib], rtol=0,
                               atol=1e-15)
    # the same arithmetic in float32 fmas keeps the end points too (what clv_lerp_rows computes)
    a32, b32 = a.astype(np.float32), b.astype(np.float32)
    for al1, want in ((0.0, a32[ia]), (1.0, b32[ib])):
        al32 = np.float32(al1)
        inner = (np.float64(-al32) * a32[ia] + a32[ia]).astype(np.float32)           # one rounding per fma
        out = (np.float64(al32) * b32[ib] + inner).astype(np.float32)
        assert np.array_equal(out, want)
    # a convex mix of two label rows stays on the simplex
    w = LR.lerp_rows(np.eye(4), [0, 0, 0], np.eye(4), [2, 2, 2], [0.0, 0.25, 1.0])
    assert np.all(w >= 0) and np.allclose(w.sum(1), 1.0, atol=1e-15)


# --------------------------------------------------------------- the conditions on the GPU test's inputs (no tolerance)
@pytest.mark.parametrize("T", [t for t, _ in VR.FREE_RUN_TEMPS])
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_flip_cap_holds_for_the_free_path_cases(which, T):
    """the decode reference in float32 against itself in float64 on the very inputs of GPU test 4: nothing outside the
    window and at most FLIP_CAP flips, so a float32 route that follows the definition can meet the same assertion"""
    fol = LR.flips_f32_against_f64(which, T)
    print("%s T=%g: %d flips, %d far" % (which, T, fol.flips, fol.far))
    assert fol.clamp_wrong == 0 and fol.far == 0 and fol.flips <= LR.FLIP_CAP
    p, z, x0, w_dec, clamp, L, seed = LR.free_path_case(which)
    Xs, _, _ = LR.decode(which, p, z, w_dec, x0=x0, seed=seed, L=L, clamp=clamp, T=T)
    free = clamp > 1
    assert 0 < Xs[free].mean() < 1 and abs((clamp <= 1).mean() - 0.3) < 0.03          # a live run, about 30 % clamped


@pytest.mark.parametrize("which,L,gate,use_x_prev", LR.LATENT_CASES)
def test_float32_reference_uses_under_a_tenth_of_the_latent_bound(which, L, gate, use_x_prev):
    """the latents' bound is the logit bound of tests/test_gpu_vary.py (2e-4); the issue keeps it as long as the float32
    numpy reference on the CPU stays under a tenth of it"""
    dev = LR.f32_latent_deviation(which, L, gate, use_x_prev)
    print("%s L=%d %s x_prev=%s: float32 reference deviates by %.3e (a tenth of the bound: %.0e)"
          % (which, L, gate, use_x_prev, dev, LR.LATENT_TOL / 10))
    assert dev < LR.LATENT_TOL / 10


@pytest.mark.parametrize("which,L,C", [('cl_vrnn', 2, 10), ('cl_vae', 3, 4)])
def test_keyed_morph_seed_samples_the_enumerated_distribution(which, L, C):
    """the reference's own sample of GPU test 8's alpha = 1 rows meets that test's criterion for every key"""
    _, p, keys = VR.keyed_params(which)
    for c in keys:
        want, _, other = VR.enumerate_redecoding(which, p, L, C, keys[0], c)
        Xs = LR.keyed_morph_rows(which, p, L, C, c, LR.KEYED_MORPH_SEED[which])
        worst = VR.worst_cell(VR.history_counts(Xs), want, VR.KEYED_ROWS)
        print("%s w_b=%d: worst history %.2f SE" % (which, c, worst))
        assert worst < 4 and np.all(Xs[:, :, 2:] == 0) and other < 1e-12
