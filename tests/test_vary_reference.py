"""CPU: the conventions of the re-decoding reference (tests/vary_reference.py), its agreement with the training
forward pass of the oracle, and the conditions on the inputs of tests/test_gpu_vary.py that need no device (flip cap,
logit range, power of the keyed enumeration, the sampled frequencies of the chosen seeds)."""
import numpy as np
import pytest

import clvae_amd  # noqa: F401  (puts the package on the path the way the other reference tests do)
import vary_reference as VR
from oracle import clvae_oracle as O
from oracle import philox as OP

D = 88


def _case(which, L=None, use_x_prev=True, gate='hard_sigmoid', N=4, Tn=6):
    C = VR.classes_of(which)
    L = L or (2 if which == 'cl_vrnn' else 3)
    cfg, p = VR.case_params(which, L, C, use_x_prev, gate)
    return (cfg, p, L) + VR.case_inputs(N, Tn, C)


# ------------------------------------------------------------------------------------------- the conventions
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_history_is_irrelevant_without_use_x_prev(which):
    _, p, L, src, x0, w_enc, w_dec = _case(which, use_x_prev=False)
    kw = dict(x0=x0, seed=5, L=L, clamp=VR.roll(4, 6, seed=1))
    a = VR.vary(which, p, src, w_enc, w_dec, history='own', **kw)
    b = VR.vary(which, p, src, w_enc, w_dec, history='source', **kw)
    c = VR.vary(which, p, src, w_enc, w_dec, history='own', **dict(kw, x0=None))
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x, y) for x, y in zip(a, c))
    _, p, L, src, x0, w_enc, w_dec = _case(which, use_x_prev=True)           # and it matters with it
    a = VR.vary(which, p, src, w_enc, w_dec, history='own', **kw)
    b = VR.vary(which, p, src, w_enc, w_dec, history='source', **kw)
    assert not np.array_equal(a[1], b[1])


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_zero_z_temperature_removes_eps(which):
    _, p, L, src, x0, w_enc, w_dec = _case(which)
    xh = lambda seed, Tz: VR.vary(which, p, src, w_enc, w_dec, x0=x0, history='source', seed=seed, L=L, Tz=Tz)[1]
    assert np.array_equal(xh(1, 0.0), xh(2, 0.0)) and not np.array_equal(xh(1, 1.0), xh(2, 1.0))


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_a_clamped_note_is_the_rolls_and_xhat_stays_unclamped(which):
    _, p, L, src, x0, w_enc, w_dec = _case(which)
    clamp = VR.roll(4, 6, seed=2)
    Xs, xh, _ = VR.vary(which, p, src, w_enc, w_dec, x0=x0, seed=3, L=L, clamp=clamp)
    fixed = clamp <= 1
    assert fixed.any() and np.array_equal(Xs[fixed], clamp[fixed].astype(np.float64))
    assert np.all((xh > 0) & (xh < 1))
    free = VR.vary(which, p, src, w_enc, w_dec, x0=x0, seed=3, L=L)
    allfree = VR.vary(which, p, src, w_enc, w_dec, x0=x0, seed=3, L=L, clamp=np.full((4, 6, D), VR.FREE, np.uint8))
    assert all(np.array_equal(x, y) for x, y in zip(free, allfree))
    assert np.array_equal(free[1][:, 0], xh[:, 0])                        # frame 0 has seen no clamped note yet


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_all_clamped_roll_equal_to_sources_under_own_is_source(which):
    _, p, L, src, x0, w_enc, w_dec = _case(which)
    for T, Tz in ((1.0, 1.0), (0.5, 2.0)):
        kw = dict(x0=x0, seed=8, L=L, T=T, Tz=Tz)
        own = VR.vary(which, p, src, w_enc, w_dec, history='own', clamp=src.astype(np.uint8), **kw)
        source = VR.vary(which, p, src, w_enc, w_dec, history='source', **kw)
        assert np.array_equal(own[0], src) and np.array_equal(own[1], source[1]) and np.array_equal(own[2], source[2])


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_labels_do_what_they_say_and_none_is_w_enc(which):
    _, p, L, src, x0, w_enc, w_dec = _case(which)
    kw = dict(x0=x0, history='source', seed=4, L=L)
    a = VR.vary(which, p, src, w_enc, None, **kw)
    b = VR.vary(which, p, src, w_enc, w_enc, **kw)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not np.array_equal(a[1], VR.vary(which, p, src, w_enc, w_dec, **kw)[1])
    assert not np.array_equal(a[1], VR.vary(which, p, src, w_dec, w_enc, **kw)[1])


# --------------------------------------------------------------- the conditions on the GPU test's inputs (no tolerance)
@pytest.mark.parametrize("T,Tz", VR.FREE_RUN_TEMPS)
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_flip_cap_holds_for_the_free_running_cases(which, T, Tz):
    """the reference in float32 against itself in float64 on the very inputs of GPU test 2: nothing outside the window and
    at most FLIP_CAP flips, so a float32 route that follows the definition can meet the same assertion"""
    fol = VR.flips_f32_against_f64(which, T, Tz)
    print("%s T=%g Tz=%g: %d flips, %d far" % (which, T, Tz, fol.flips, fol.far))
    assert fol.clamp_wrong == 0 and fol.far == 0 and fol.flips <= VR.FLIP_CAP
    _, p, src, x0, w_enc, w_dec, clamp, L, seed = VR.free_run_case(which)
    Xs, _, _ = VR.vary(which, p, src, w_enc, w_dec, x0=x0, seed=seed, L=L, clamp=clamp, T=T, Tz=Tz)
    free = clamp > 1
    assert 0 < Xs[free].mean() < 1 and abs((clamp <= 1).mean() - 0.3) < 0.03          # a live run, about 30 % clamped


@pytest.mark.parametrize("which,L,gate,use_x_prev", VR.IDENTITY_CASES)
def test_identity_cases_keep_their_logits_where_float32_probabilities_resolve_them(which, L, gate, use_x_prev):
    C = VR.classes_of(which)
    _, p = VR.case_params(which, L, C, use_x_prev, gate or 'hard_sigmoid')
    src, x0, w_enc, _ = VR.case_inputs(VR.IDENTITY_N, VR.IDENTITY_T, C)
    _, xh, lg = VR.vary(which, p, src, w_enc, None, x0=x0, history='source', seed=VR.IDENTITY_SEED, L=L, gate=gate)
    assert np.abs(lg).max() <= VR.IDENTITY_MAX_LOGIT, np.abs(lg).max()
    np.testing.assert_allclose(VR.logit_of(xh.astype(np.float32)), lg, rtol=0, atol=1e-5)


# ------------------------------------------------------------------------ the training forward pass of the oracle
def _given_label(monkeypatch, W):
    """the oracle's forward passes sample their label; here it is given (oracle/ stays as it is)"""
    monkeypatch.setattr(O, 'logistic_normal', lambda mean, log_var, eps: W)


@pytest.mark.parametrize("gate,use_x_prev,L", [('hard_sigmoid', True, 2), ('sigmoid', False, 2), ('sigmoid', True, 19)])
def test_source_history_is_the_oracles_vrnn_forward(monkeypatch, gate, use_x_prev, L):
    C, N, seed = 10, 4, 12
    cfg, p = VR.case_params('cl_vrnn', L, C, use_x_prev, gate)
    Tn = cfg['T']
    src, x0, w_enc, _ = VR.case_inputs(N, Tn, C)
    _, xh, lg = VR.vary('cl_vrnn', p, src, w_enc, None, x0=x0, history='source', seed=seed, L=L, gate=gate)
    p64 = {k: np.asarray(v, np.float64) for k, v in p.items()}
    eps_Z = np.stack([OP.normal(N * L, seed, step=t, stream_id=0).reshape(N, L).astype(np.float64) for t in range(Tn)], 1)
    Xp = np.concatenate([x0[:, None], src[:, :-1]], 1)
    _given_label(monkeypatch, w_enc)
    c = O.vrnn_forward(p64, cfg, src, Xp, np.zeros((N, C - 1)), eps_Z)
    np.testing.assert_allclose(lg, c['logits'], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(xh, c['X_hat'], rtol=1e-12, atol=0)


@pytest.mark.parametrize("use_x_prev,L", [(True, 3), (False, 8)])
def test_source_history_is_the_oracles_vae_forward(monkeypatch, use_x_prev, L):
    C, N, Tn, seed = 4, 5, 6, 12
    cfg, p = VR.case_params('cl_vae', L, C, use_x_prev)
    src, x0, w_enc, _ = VR.case_inputs(N, Tn, C)
    _, xh, lg = VR.vary('cl_vae', p, src, w_enc, None, x0=x0, history='source', seed=seed, L=L)
    p64 = {k: np.asarray(v, np.float64) for k, v in p.items()}
    _given_label(monkeypatch, w_enc)
    for t in range(Tn):
        eps_z = OP.normal(N * L, seed, step=t, stream_id=0).reshape(N, L).astype(np.float64)
        c = O.vae_forward(p64, cfg, src[:, t], x0 if t == 0 else src[:, t - 1], np.zeros((N, C - 1)), eps_z)
        np.testing.assert_allclose(lg[:, t], c['logits'], rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(xh[:, t], c['x_hat'], rtol=1e-12, atol=0)


# --------------------------------------------------------------------------------- the keyed enumerable models
KEYED = {'cl_vrnn': (2, 10), 'cl_vae': (3, 4)}


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_enumerated_redecoding_depends_on_w_dec_and_not_on_w_enc(which):
    L, C = KEYED[which]
    _, p, keys = VR.keyed_params(which)
    dist = {}
    for c in keys:
        dist[c], _, other = VR.enumerate_redecoding(which, p, L, C, keys[0], c)
        assert abs(dist[c].sum() - 1) < 1e-12 and other < 1e-12          # notes 2..87 (logit clipped at -30) never sound
        for c_enc in keys[1:]:
            again, _, _ = VR.enumerate_redecoding(which, p, L, C, c_enc, c)
            assert np.array_equal(again, dist[c])
    # power: two keys are told apart by some single history's probability
    gap = max(np.abs(dist[a] - dist[b]).max() for a in keys for b in keys)
    print("%s: largest difference of a history's probability between two keys %.4f" % (which, gap))
    assert gap >= 0.1


def keyed_reference_sample(which, c_enc, c_dec):
    """the reference's own 4096 re-decodings of the keyed source under (c_enc, c_dec), with the Philox seed of GPU test 5"""
    L, C = KEYED[which]
    _, p, _ = VR.keyed_params(which)
    n = VR.KEYED_ROWS
    src = np.repeat(VR.keyed_source()[None], n, 0)
    Xs, _, _ = VR.vary(which, p, src, np.eye(C)[np.full(n, c_enc)], np.eye(C)[np.full(n, c_dec)], seed=VR.KEYED_SEED[which],
                       L=L, T=VR.KEYED_T)
    return Xs


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_keyed_seed_samples_the_enumerated_distribution(which):
    """a condition on GPU test 5's seed: the reference's own sample with it meets the test's criterion (4 binomial standard
    errors in every history) for every key -- 256 cells per key, many with an expected count below one, are not all within
    4 standard errors for every seed"""
    L, C = KEYED[which]
    _, p, keys = VR.keyed_params(which)
    for c in keys:
        want, _, _ = VR.enumerate_redecoding(which, p, L, C, keys[0], c)
        Xs = keyed_reference_sample(which, keys[0], c)
        assert np.all(Xs[:, :, 2:] == 0)
        worst = VR.worst_cell(VR.history_counts(Xs), want, VR.KEYED_ROWS)
        print("%s key %d: worst history %.2f SE" % (which, c, worst))
        assert worst < 4
