"""-m gpu: whole cl_vae / cl_vrnn training steps on the HIP path vs the fp64 oracle.

North-star tolerances: |ELBO_gpu - ELBO_oracle| <= 1e-3 nats per frame on
identical weights, inputs and injected eps; per-note decoder logits max-abs error reported and
bounded; gradients to 1e-4 relative (of the tensor's max); three Adam-WN steps track the oracle.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import clvae_oracle as O
from oracle import philox as OP

pytestmark = pytest.mark.gpu

ELBO_TOL = 1e-3
LOGIT_TOL = 2e-4


@pytest.fixture(scope="module")
def dev():
    import clvae_amd
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def T(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def N(t):
    return t.detach().cpu().numpy().astype(np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def check_grads(got, ref, tol=1e-4):
    for k in ref:
        scale = np.abs(ref[k]).max() + 1e-8
        err = np.abs(got[k] - ref[k]).max() / scale
        assert err < tol, "%s: rel err %.3e" % (k, err)


def frames(rng, *shape):
    return (rng.random(shape) < 0.0443).astype(np.float64)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("B,L,Cn,use_x_prev,weights", [
    (100, 4, 2, True, (1.0, 1.0, 1.0, 0.0)),       # BASELINE config 1 shape
    (512, 4, 2, True, (1.0, 1.0, 1.0, 0.0)),       # config 2 shape (fp32 path)
    (48, 2, 10, False, (0.7, 0.3, 0.9, 0.4)),
    (37, 16, 16, True, (0.5, 0.8, 1.1, -0.2)),     # ragged last row tile, widest fused heads
])
def test_cl_vae_step_matches_oracle(dev, B, L, Cn, use_x_prev, weights, fused):
    """fused=True: the single-launch whole-step kernel (csrc/vae_fused.hip); False: the layer-by-layer chain."""
    from clvae_amd.engine import VaeEngine
    cw, klw, wklw, prior = weights
    cfg = O.vae_config(latent_dim=L, n_classes=Cn, use_x_prev=use_x_prev, class_weight=cw, kl_weight=klw,
                       w_kl_weight=wklw, w_log_var_prior=prior)
    cfg['fused_step'] = fused
    rng = np.random.default_rng(11)
    p = {k: f32(v) for k, v in O.vae_init_params(cfg, seed=1).items()}
    for k in p:
        if k.endswith('bias'):
            p[k] = f32(0.05 * rng.standard_normal(p[k].shape))
    x, xp = frames(rng, B, 88), frames(rng, B, 88)
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    ew, ez = f32(rng.standard_normal((B, Cn - 1))), f32(rng.standard_normal((B, L)))
    ref = O.vae_loss_and_grads(p, cfg, x, xp, wt, ew, ez)

    eng = VaeEngine(cfg, B, dev)
    assert eng.fused == fused
    eng.P.set_weights(p)
    args = (T(x, dev), T(xp, dev), T(wt, dev), T(ew, dev), T(ez, dev))
    eng.loss_and_grads(*args)
    torch.cuda.synchronize()
    got = eng.losses()
    logit_err = np.abs(N(eng.logits) - ref['cache']['logits']).max()
    print("cl_vae B=%d: ELBO gpu %.6f oracle %.6f |d|=%.2e  logits max-abs err %.2e"
          % (B, got['elbo'], ref['elbo'], abs(got['elbo'] - ref['elbo']), logit_err))
    assert abs(got['elbo'] - ref['elbo']) <= ELBO_TOL
    assert abs(got['total'] - ref['total']) <= ELBO_TOL
    for k in ('vae', 'kl_z', 'kl_w', 'w_rec'):
        assert abs(got[k] - ref[k]) <= ELBO_TOL, k
    assert abs(got['acc'] - ref['acc']) < 1e-6
    assert logit_err < LOGIT_TOL
    check_grads(eng.P.get_weights(eng.P.grads), ref['grads'])
    # three optimizer steps on the same batch
    st = O.adam_wn_init(p)
    for _ in range(3):
        r = O.vae_loss_and_grads(p, cfg, x, xp, wt, ew, ez)
        O.adam_wn_step(p, r['grads'], st)
        eng.loss_and_grads(*args)
        eng.P.adam_step()
    w = eng.P.get_weights()
    for k in p:
        np.testing.assert_allclose(w[k], p[k], rtol=2e-3, atol=2e-5, err_msg=k)


def _gi(G, prefix):
    return {k[len(prefix):]: G[k].astype(np.float64) for k in G.files if k.startswith(prefix)}


@pytest.mark.parametrize("fused", [True, False])
def test_cl_vae_matches_the_independent_fixture(dev, fused):
    """The HIP step against tests/golden/g4_independent.npz: losses, logits and gradients that a float64 torch.autograd
    graph written from cl_vae/model.py:130-224 (no import of oracle/) produced for real JSB frames -- a pin that is not
    the oracle grading itself.  One note column's logits lie far beyond both Bernoulli clip points."""
    from helpers import golden
    from clvae_amd.engine import VaeEngine
    G = golden("g4_independent.npz")
    cw, kw, wkw = G['vae/wts']
    cfg = O.vae_config(latent_dim=4, n_classes=2, use_x_prev=True, class_weight=cw, kl_weight=kw, w_kl_weight=wkw,
                       w_log_var_prior=float(G['vae/prior']))
    cfg['fused_step'] = fused
    B = G['vae/x'].shape[0]
    eng = VaeEngine(cfg, B, dev)
    assert eng.fused == fused
    eng.P.set_weights(_gi(G, 'vae/p/'))
    eng.loss_and_grads(T(G['vae/x'], dev), T(G['vae/xp'], dev), T(G['vae/wt'], dev), T(G['vae/ew'], dev), T(G['vae/ez'], dev))
    torch.cuda.synchronize()
    got = eng.losses()
    for k in ('vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
        assert abs(got[k] - float(G['vae/loss/' + k])) <= ELBO_TOL, (k, got[k], float(G['vae/loss/' + k]))
    assert abs(got['acc'] - float(G['vae/loss/acc'])) < 1e-6
    ref_l = G['vae/logits']
    assert np.abs(N(eng.logits) - ref_l).max() < LOGIT_TOL * max(1.0, np.abs(ref_l).max() / 16)
    check_grads(eng.P.get_weights(eng.P.grads), _gi(G, 'vae/g/'))


@pytest.mark.parametrize("pair", [True, False])
def test_cl_vrnn_matches_the_independent_fixture(dev, pair):
    """cl_vrnn against the independent fixture (float64 torch.autograd from cl_vrnn/model.py:164-267): every loss term,
    per-note logits (several note columns sit beyond, between and just inside the two Bernoulli clip points), both LSTMs'
    states (gate biases push units into the flat regions of the hard sigmoid) and every gradient tensor; the pair
    kernels and the separate sequence kernels."""
    from helpers import golden
    from clvae_amd.engine import VrnnEngine
    G = golden("g4_independent.npz")
    cw, kw, wkw = G['vrnn/wts']
    B, Tn = G['vrnn/X'].shape[:2]
    cfg = O.vrnn_config(latent_dim=2, seq_length=Tn, n_classes=10, use_x_prev=True, class_weight=cw, kl_weight=kw,
                        w_kl_weight=wkw, w_log_var_prior=float(G['vrnn/prior']))
    cfg['fuse_pair'] = pair
    eng = VrnnEngine(cfg, B, dev)
    assert eng.fuse_pair == pair
    eng.P.set_weights(_gi(G, 'vrnn/p/'))
    eng.loss_and_grads(T(G['vrnn/X'], dev), T(G['vrnn/Xp'], dev), T(G['vrnn/wt'], dev), T(G['vrnn/eW'], dev),
                       T(G['vrnn/eZ'].reshape(B * Tn, -1), dev))
    torch.cuda.synchronize()
    got = eng.losses()
    for k in ('vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
        assert abs(got[k] - float(G['vrnn/loss/' + k])) <= ELBO_TOL, (k, got[k], float(G['vrnn/loss/' + k]))
    assert np.abs(N(eng.logits).reshape(B, Tn, 88) - G['vrnn/logits']).max() < LOGIT_TOL
    np.testing.assert_allclose(N(eng.hs_enc).reshape(B, Tn, 88), G['vrnn/enc_h'], atol=2e-5)
    np.testing.assert_allclose(N(eng.hs_dec).reshape(B, Tn, 88), G['vrnn/dec_h'], atol=2e-5)
    check_grads(eng.P.get_weights(eng.P.grads), _gi(G, 'vrnn/g/'), tol=2e-4)


@pytest.mark.parametrize("use_x_prev", [True, False])
def test_cl_vae_without_hidden_layers_matches_oracle(dev, use_x_prev):
    """--intermediate_dim 0 (cl_vae/model.py:165-167,188): the latent heads read [x, w], the output layer [w, history, z]."""
    from clvae_amd.engine import VaeEngine
    B, L, Cn = 33, 3, 4
    cfg = O.vae_config(latent_dim=L, n_classes=Cn, use_x_prev=use_x_prev, intermediate_dim=0, class_weight=0.7,
                       kl_weight=0.4, w_kl_weight=0.8, w_log_var_prior=0.1)
    rng = np.random.default_rng(21)
    p = {k: f32(v) for k, v in O.vae_init_params(cfg, seed=6).items()}
    assert 'h/kernel' not in p and p['x_decoded_mean/kernel'].shape[0] == Cn + (88 if use_x_prev else 0) + L
    x, xp = frames(rng, B, 88), frames(rng, B, 88)
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    ew, ez = f32(rng.standard_normal((B, Cn - 1))), f32(rng.standard_normal((B, L)))
    ref = O.vae_loss_and_grads(p, cfg, x, xp, wt, ew, ez)
    eng = VaeEngine(cfg, B, dev)
    assert not eng.fused
    eng.P.set_weights(p)
    eng.loss_and_grads(T(x, dev), T(xp, dev), T(wt, dev), T(ew, dev), T(ez, dev))
    torch.cuda.synchronize()
    got = eng.losses()
    for k in ('vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
        assert abs(got[k] - ref[k]) <= ELBO_TOL, k
    assert np.abs(N(eng.logits) - ref['cache']['logits']).max() < LOGIT_TOL
    check_grads(eng.P.get_weights(eng.P.grads), ref['grads'])
    np.testing.assert_allclose(N(eng.x_hat()), ref['cache']['x_hat'], atol=2e-6)


@pytest.mark.parametrize("pair", [True, False])
@pytest.mark.parametrize("B,Tn,L,Cn,use_x_prev,gate", [
    (6, 5, 2, 10, True, 'hard_sigmoid'),
    (3, 1, 2, 10, True, 'hard_sigmoid'),        # one-step windows
    (3, 6, 8, 5, True, 'sigmoid'),              # widest latent the fused pair kernels carry
    (2, 4, 5, 3, False, 'hard_sigmoid'),        # odd latent_dim spanning two surplus lane groups
    (5, 7, 3, 4, False, 'hard_sigmoid'),
    (4, 9, 2, 10, True, 'sigmoid'),
    (4, 128, 2, 10, True, 'hard_sigmoid'),      # BASELINE config 3/4 shape at reduced batch
    (4, 32, 32, 10, True, 'hard_sigmoid'),      # config 5 latent size
    (1, 3, 1, 2, True, 'hard_sigmoid'),         # the smallest of everything: one sample, one latent, two classes
    (1, 1, 1, 2, False, 'sigmoid'),
    (3, 2, 4, 6, True, 'hard_sigmoid'),         # T = 2; L = 4: top of the pair forward's Z = 1 and backward's ZP = 8 variants
    (2, 7, 6, 4, False, 'sigmoid'),             # L = 6 at odd T: the backward's 16-column variant, one step of skew tail
])
def test_cl_vrnn_step_matches_oracle(dev, B, Tn, L, Cn, use_x_prev, gate, pair):
    """pair=True: both LSTMs + latent head in one persistent launch (csrc/lstm_pair.hip) where supported."""
    from clvae_amd.engine import VrnnEngine
    cfg = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=use_x_prev, class_weight=0.8,
                        kl_weight=0.6, w_kl_weight=0.9, w_log_var_prior=0.2, gate_act=gate)
    rng = np.random.default_rng(B * 1000 + Tn)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=2).items()}
    win = frames(rng, B, Tn + 1, 88)
    X, Xp = win[:, 1:].copy(), win[:, :-1].copy()
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    eW, eZ = f32(rng.standard_normal((B, Cn - 1))), f32(rng.standard_normal((B, Tn, L)))
    ref = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt, eW, eZ)

    cfg['fuse_pair'] = pair
    eng = VrnnEngine(cfg, B, dev)
    assert eng.fuse_pair == (pair and L <= 8)
    eng.P.set_weights(p)
    args = (T(X, dev), T(Xp, dev), T(wt, dev), T(eW, dev), T(eZ, dev))
    eng.loss_and_grads(*args)
    torch.cuda.synchronize()
    got = eng.losses()
    logit_err = np.abs(N(eng.logits).reshape(B, Tn, 88) - ref['cache']['logits']).max()
    print("cl_vrnn B=%d T=%d L=%d: ELBO gpu %.6f oracle %.6f |d|=%.2e  logits max-abs err %.2e"
          % (B, Tn, L, got['elbo'], ref['elbo'], abs(got['elbo'] - ref['elbo']), logit_err))
    assert abs(got['elbo'] - ref['elbo']) <= ELBO_TOL
    for k in ('vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
        assert abs(got[k] - ref[k]) <= ELBO_TOL, k
    assert logit_err < LOGIT_TOL
    np.testing.assert_allclose(N(eng.hs_enc).reshape(B, Tn, 88), ref['cache']['enc_h'], atol=2e-5)
    np.testing.assert_allclose(N(eng.hs_dec).reshape(B, Tn, 88), ref['cache']['dec_h'], atol=2e-5)
    check_grads(eng.P.get_weights(eng.P.grads), ref['grads'], tol=2e-4)
    st = O.adam_wn_init(p)
    for _ in range(2):
        r = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt, eW, eZ)
        O.adam_wn_step(p, r['grads'], st)
        eng.loss_and_grads(*args)
        eng.P.adam_step()
    w = eng.P.get_weights()
    for k in p:
        np.testing.assert_allclose(w[k], p[k], rtol=5e-3, atol=5e-5, err_msg=k)


@pytest.mark.parametrize("H,B,Tn,L,Cn,use_x_prev,gate", [
    (32, 6, 5, 2, 10, True, 'hard_sigmoid'),     # 8 k-slices per unit
    (64, 5, 9, 3, 4, True, 'sigmoid'),           # 4 slices
    (128, 4, 16, 2, 10, True, 'hard_sigmoid'),   # 2 slices; the CLI's default window (cl_vrnn/train.py:92)
    (128, 3, 7, 32, 10, False, 'hard_sigmoid'),  # no history frames, config-5 latent size
    (50, 4, 6, 2, 3, True, 'hard_sigmoid'),      # not a multiple of 4, ragged last slice
    (300, 2, 4, 2, 10, True, 'sigmoid'),         # more units than threads: two units per owner thread, one slice
    (88, 4, 6, 2, 10, True, 'hard_sigmoid'),     # the default width through the SAME generic chain (fuse_pair off, lstm_any forced)
])
def test_cl_vrnn_step_matches_oracle_at_any_intermediate_dim(dev, monkeypatch, H, B, Tn, L, Cn, use_x_prev, gate):
    """--intermediate_dim != 88 (cl_vrnn/train.py:90; LSTM(intermediate_dim) at cl_vrnn/model.py:196-199, 225-228): the
    step through the generic chain -- GEMM / row-gather input projections, csrc/lstm_any.hip for both recurrences, GEMM
    heads -- against the fp64 oracle: ELBO and every loss term, per-note logits, both LSTMs' states, every gradient
    tensor, and two Adam-WN steps."""
    from clvae_amd.engine import VrnnEngine
    cfg = O.vrnn_config(intermediate_dim=H, latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=use_x_prev,
                        class_weight=0.8, kl_weight=0.6, w_kl_weight=0.9, w_log_var_prior=0.2, gate_act=gate)
    rng = np.random.default_rng(H * 1000 + Tn)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=2).items()}
    win = frames(rng, B, Tn + 1, 88)
    X, Xp = win[:, 1:].copy(), win[:, :-1].copy()
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    eW, eZ = f32(rng.standard_normal((B, Cn - 1))), f32(rng.standard_normal((B, Tn, L)))
    ref = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt, eW, eZ)
    if H == 88:
        cfg['fuse_pair'] = False
        monkeypatch.setenv("CLV_LSTM_ANY", "1")
    eng = VrnnEngine(cfg, B, dev)
    assert not eng.fuse_pair and not eng.use_mx
    eng.P.set_weights(p)
    args = (T(X, dev), T(Xp, dev), T(wt, dev), T(eW, dev), T(eZ, dev))
    eng.loss_and_grads(*args)
    torch.cuda.synchronize()
    got = eng.losses()
    logit_err = np.abs(N(eng.logits).reshape(B, Tn, 88) - ref['cache']['logits']).max()
    print("cl_vrnn H=%d B=%d T=%d L=%d: ELBO gpu %.6f oracle %.6f |d|=%.2e  logits max-abs err %.2e"
          % (H, B, Tn, L, got['elbo'], ref['elbo'], abs(got['elbo'] - ref['elbo']), logit_err))
    for k in ('elbo', 'vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
        assert abs(got[k] - ref[k]) <= ELBO_TOL, k
    assert logit_err < LOGIT_TOL
    np.testing.assert_allclose(N(eng.hs_enc).reshape(B, Tn, H), ref['cache']['enc_h'], atol=2e-5)
    np.testing.assert_allclose(N(eng.hs_dec).reshape(B, Tn, H), ref['cache']['dec_h'], atol=2e-5)
    check_grads(eng.P.get_weights(eng.P.grads), ref['grads'], tol=2e-4)
    st = O.adam_wn_init(p)
    for _ in range(2):
        r = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt, eW, eZ)
        O.adam_wn_step(p, r['grads'], st)
        eng.loss_and_grads(*args)
        eng.P.adam_step()
    w = eng.P.get_weights()
    for k in p:
        np.testing.assert_allclose(w[k], p[k], rtol=5e-3, atol=5e-5, err_msg=k)


@pytest.mark.parametrize("H,B,Tn,L,Cn,use_x_prev,gate,rate", [
    (88, 5, 7, 2, 10, True, 'hard_sigmoid', 0.25),     # the default width: the generic chain instead of the pair kernels
    (88, 4, 16, 3, 4, False, 'sigmoid', 0.5),          # no history frames: the decoder's inputs are [z, W]
    (48, 3, 6, 2, 3, True, 'hard_sigmoid', 0.1),       # another width (csrc/lstm_any.hip)
])
def test_cl_vrnn_step_with_lstm_input_dropout_matches_oracle(dev, H, B, Tn, L, Cn, use_x_prev, gate, rate):
    """get_model(dropout=p) -> LSTM(..., dropout=p) for both LSTMs (cl_vrnn/model.py:164,198,227; Keras 2.0.0, implementation
    0: one input mask per gate and sample, constant over the time steps).  A training pass with INJECTED mask uniforms against
    the oracle with the same masks: every loss term, per-note logits, both LSTMs' states, every gradient tensor (incl. dZ and
    dW through the masks), two Adam-WN steps; a pass without gradients (validation / predict) takes no dropout."""
    from clvae_amd.engine import VrnnEngine
    cfg = O.vrnn_config(intermediate_dim=H, latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=use_x_prev,
                        class_weight=0.8, kl_weight=0.6, w_kl_weight=0.9, w_log_var_prior=0.2, gate_act=gate)
    rng = np.random.default_rng(H + Tn)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=4).items()}
    win = frames(rng, B, Tn + 1, 88)
    X, Xp = win[:, 1:].copy(), win[:, :-1].copy()
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    eW, eZ = f32(rng.standard_normal((B, Cn - 1))), f32(rng.standard_normal((B, Tn, L)))
    in_e, in_d = 88 + Cn, (88 if use_x_prev else 0) + L + Cn
    ue, ud = f32(rng.random((B, 4, in_e))), f32(rng.random((B, 4, in_d)))          # device layout [row][gate][input]
    masks = (O.dropout_masks(ue.transpose(1, 0, 2), rate), O.dropout_masks(ud.transpose(1, 0, 2), rate))
    assert 0.3 * rate < (masks[0] == 0).mean() < 3 * rate
    ref = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt, eW, eZ, masks=masks)
    plain = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt, eW, eZ, need_grads=False)
    assert abs(ref['vae'] - plain['vae']) > 1e-2                                    # the masks matter

    eng = VrnnEngine(dict(cfg, dropout=rate), B, dev)
    assert eng.dropout == rate and not eng.fuse_pair and not eng.use_mx
    eng.P.set_weights(p)
    args = (T(X, dev), T(Xp, dev), T(wt, dev), T(eW, dev), T(eZ, dev))
    with pytest.raises(RuntimeError):          # no masks yet (neither noise=... nor injected uniforms): refuse, do not read junk
        eng.loss_and_grads(*args)
    eng.set_dropout_uniforms(T(ue, dev), T(ud, dev))
    eng.loss_and_grads(*args)
    torch.cuda.synchronize()
    got = eng.losses()
    logit_err = np.abs(N(eng.logits).reshape(B, Tn, 88) - ref['cache']['logits']).max()
    print("cl_vrnn dropout %.2f H=%d: ELBO gpu %.6f oracle %.6f |d|=%.2e  logits max-abs err %.2e"
          % (rate, H, got['elbo'], ref['elbo'], abs(got['elbo'] - ref['elbo']), logit_err))
    for k in ('elbo', 'vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
        assert abs(got[k] - ref[k]) <= ELBO_TOL, k
    assert logit_err < LOGIT_TOL
    np.testing.assert_allclose(N(eng.hs_enc).reshape(B, Tn, H), ref['cache']['enc_h'], atol=2e-5)
    np.testing.assert_allclose(N(eng.hs_dec).reshape(B, Tn, H), ref['cache']['dec_h'], atol=2e-5)
    check_grads(eng.P.get_weights(eng.P.grads), ref['grads'], tol=2e-4)
    # an inference pass: no dropout
    eng.loss_and_grads(*args, need_grads=False)
    torch.cuda.synchronize()
    got = eng.losses()
    for k in ('vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
        assert abs(got[k] - plain[k]) <= ELBO_TOL, k
    st = O.adam_wn_init(p)
    for _ in range(2):
        r = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt, eW, eZ, masks=masks)
        O.adam_wn_step(p, r['grads'], st)
        eng.loss_and_grads(*args)
        eng.P.adam_step()
    w = eng.P.get_weights()
    for k in p:
        np.testing.assert_allclose(w[k], p[k], rtol=5e-3, atol=5e-5, err_msg=k)


def test_cl_vrnn_fit_with_dropout_draws_its_masks_from_philox(dev):
    """Model.fit on get_model(dropout=0.2): the captured step draws the masks' uniforms itself (Philox streams 2 / 3 at the
    step's counter, by global row) -- an oracle loop with oracle/philox.py's uniforms follows the epoch losses; validation
    takes no dropout."""
    from clvae_amd.cl_vrnn.model import get_model
    B, Tn, L, C, n, rate, seed = 4, 6, 2, 3, 12, 0.2, 91
    rng = np.random.default_rng(5)
    win = (rng.random((n, Tn + 1, 88)) < 0.05).astype(np.float64)
    X, Xp = win[:, 1:].copy(), win[:, :-1].copy()
    wt = np.eye(C)[rng.integers(0, C, n)]
    model, _ = get_model(B, 88, 88, L, Tn, C, True, 'adam-wn', dropout=rate, seed=seed)
    p = {k: f32(v) for k, v in model.engine.P.get_weights().items()}
    cfg = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=C, use_x_prev=True)
    hist = model.fit([X, Xp], [X, wt, wt, X], shuffle=False, epochs=2, batch_size=B, verbose=0,
                     validation_data=([X[:B], Xp[:B]], [X[:B], wt[:B], wt[:B], X[:B]]))
    in_e, in_d = 88 + C, 88 + L + C
    st, it, ref_epoch, ref_val = O.adam_wn_init(p), 0, [], []
    for ep in range(2):
        tot = 0.0
        for b0 in range(0, n, B):
            eW = OP.normal(B * (C - 1), seed, step=it, stream_id=0).reshape(B, C - 1).astype(np.float64)
            eZ = OP.normal(B * Tn * L, seed, step=it, stream_id=1).reshape(B, Tn, L).astype(np.float64)
            ue = OP.uniform(B * 4 * in_e, seed, step=it, stream_id=2).reshape(B, 4, in_e).astype(np.float64)
            ud = OP.uniform(B * 4 * in_d, seed, step=it, stream_id=3).reshape(B, 4, in_d).astype(np.float64)
            masks = (O.dropout_masks(ue.transpose(1, 0, 2), rate), O.dropout_masks(ud.transpose(1, 0, 2), rate))
            r = O.vrnn_loss_and_grads(p, cfg, X[b0:b0 + B], Xp[b0:b0 + B], wt[b0:b0 + B], eW, eZ, masks=masks)
            O.adam_wn_step(p, r['grads'], st)
            tot += r['total']
            it += 1
        ref_epoch.append(tot / (n // B))
        eW = OP.normal(B * (C - 1), seed, step=it, stream_id=4).reshape(B, C - 1).astype(np.float64)
        eZ = OP.normal(B * Tn * L, seed, step=it, stream_id=5).reshape(B, Tn, L).astype(np.float64)
        ref_val.append(O.vrnn_loss_and_grads(p, cfg, X[:B], Xp[:B], wt[:B], eW, eZ, need_grads=False)['total'])
    np.testing.assert_allclose(hist.history['loss'], ref_epoch, rtol=2e-4)
    np.testing.assert_allclose(hist.history['val_loss'], ref_val, rtol=2e-4)


@pytest.mark.parametrize("exact_frames", [False, True])
@pytest.mark.parametrize("B,Tn,L", [(256, 128, 2),         # BASELINE config 3 (and 4 per GPU): what bench.py times
                                    (1024, 256, 32),       # config 5 per GPU
                                    (1024, 32, 2)])        # the pair kernels at 1024 rows: four workgroups per CU
def test_cl_vrnn_full_size_step_matches_oracle(dev, B, Tn, L, exact_frames):
    """One step at the sizes the benchmark runs, against the fp64 oracle on the same weights, frames and noise: ELBO
    and every loss term to 1e-3, per-note logits, both LSTMs' states, every gradient tensor.
    exact_frames: what the bench and `fit()` on a uint8 data set run -- the frames are 0/1 bytes, so the engine is told
    that every frame value is exactly a bf16 number and the LSTM kernel gradients take the one-piece variants of the
    split-bf16 product (lstm_wgrad_bf16_kernel<6,1> at 256 x 128, <8,1> at 1024 x 256) inside the whole step."""
    from clvae_amd.engine import VrnnEngine
    Cn = 10
    cfg = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=True)
    cfg['frames_exact_bf16'] = exact_frames
    rng = np.random.default_rng(B + Tn)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=3).items()}
    win = frames(rng, B, Tn + 1, 88)
    X, Xp = win[:, 1:].copy(), win[:, :-1].copy()
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    eW, eZ = f32(rng.standard_normal((B, Cn - 1))), f32(rng.standard_normal((B, Tn, L)))
    ref = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt, eW, eZ)
    eng = VrnnEngine(cfg, B, dev)
    assert eng.fuse_pair == (L <= 8)
    assert eng.use_mx == (L > 8 and B >= 768)          # config 5: both LSTMs on the bf16 matrix cores (csrc/lstm_mx.hip)
    assert eng.frames_exact_bf16 == exact_frames and eng.bf16_wgrad
    assert set(np.unique(X)) <= {0.0, 1.0}                  # byte-valued frames: exact in one bf16 piece
    eng.P.set_weights(p)
    eng.loss_and_grads(T(X, dev), T(Xp, dev), T(wt, dev), T(eW, dev), T(eZ, dev))
    torch.cuda.synchronize()
    got = eng.losses()
    logit_err = np.abs(N(eng.logits).reshape(B, Tn, 88) - ref['cache']['logits']).max()
    print("cl_vrnn FULL SIZE B=%d T=%d L=%d: ELBO gpu %.6f oracle %.6f |d|=%.2e  logits max-abs err %.2e"
          % (B, Tn, L, got['elbo'], ref['elbo'], abs(got['elbo'] - ref['elbo']), logit_err))
    assert abs(got['elbo'] - ref['elbo']) <= ELBO_TOL
    for k in ('vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
        assert abs(got[k] - ref[k]) <= ELBO_TOL, k
    assert logit_err < LOGIT_TOL
    np.testing.assert_allclose(N(eng.hs_enc).reshape(B, Tn, 88), ref['cache']['enc_h'], atol=5e-5)
    np.testing.assert_allclose(N(eng.hs_dec).reshape(B, Tn, 88), ref['cache']['dec_h'], atol=5e-5)
    check_grads(eng.P.get_weights(eng.P.grads), ref['grads'], tol=3e-4)


@pytest.mark.parametrize("model", ["cl_vae_fused", "cl_vae_layers", "cl_vrnn_pair", "cl_vrnn_separate"])
def test_predict_next_scores_the_next_frame(dev, model):
    """--predict_next (cl_vae/train.py:15,66; cl_vrnn/train.py:15,66): the input is frame t, the reconstruction target
    frame t+1.  Losses and gradients with a separate target vs the oracle given the same target."""
    from clvae_amd.engine import VaeEngine, VrnnEngine
    rng = np.random.default_rng(5)
    if model.startswith("cl_vae"):
        B, L, Cn = 40, 3, 4
        cfg = O.vae_config(latent_dim=L, n_classes=Cn, use_x_prev=False)
        cfg['fused_step'] = model.endswith("fused")
        p = {k: f32(v) for k, v in O.vae_init_params(cfg, seed=4).items()}
        x, y = frames(rng, B, 88), frames(rng, B, 88)
        eZ = f32(rng.standard_normal((B, L)))
        fn, eng, xp = O.vae_loss_and_grads, VaeEngine(cfg, B, dev), x
    else:
        B, Tn, L, Cn = 5, 7, 2, 4
        cfg = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=False)
        cfg['fuse_pair'] = model.endswith("pair")
        p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=4).items()}
        win = frames(rng, B, Tn + 1, 88)
        x, y = win[:, :-1].copy(), win[:, 1:].copy()
        eZ = f32(rng.standard_normal((B, Tn, L)))
        fn, eng, xp = O.vrnn_loss_and_grads, VrnnEngine(cfg, B, dev), x
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    eW = f32(rng.standard_normal((B, Cn - 1)))
    ref = fn(p, cfg, x, xp, wt, eW, eZ, target=y)
    plain = fn(p, cfg, x, xp, wt, eW, eZ)
    ob = 'x_decoded_mean/bias' if model.startswith("cl_vae") else 'X_decoded_mean/bias'
    assert np.abs(ref['grads'][ob] - plain['grads'][ob]).max() > 1e-2      # the two targets really pull differently
    eng.P.set_weights(p)
    eng.loss_and_grads(T(x, dev), T(xp, dev), T(wt, dev), T(eW, dev), T(eZ, dev), target=T(y, dev))
    torch.cuda.synchronize()
    got = eng.losses()
    for k in ('vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
        assert abs(got[k] - ref[k]) <= ELBO_TOL, k
    check_grads(eng.P.get_weights(eng.P.grads), ref['grads'], tol=2e-4)


def test_cl_vrnn_fused_and_separate_output_head_agree(dev):
    """Output head as one launch (clv_out_head_train, default) == gemm_bce + dhs GEMM + weight-gradient GEMM."""
    from clvae_amd.engine import VrnnEngine
    B, Tn, L, Cn = 8, 40, 2, 10
    rng = np.random.default_rng(78)
    base = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=True)
    p = {k: f32(v) for k, v in O.vrnn_init_params(base, seed=4).items()}
    win = frames(rng, B, Tn + 1, 88)
    args_np = (win[:, 1:].copy(), win[:, :-1].copy(), np.eye(Cn)[rng.integers(0, Cn, B)],
               rng.standard_normal((B, Cn - 1)), rng.standard_normal((B, Tn, L)))
    res = []
    for flag in (True, False):
        cfg = dict(base)
        cfg['fuse_head'] = flag
        eng = VrnnEngine(cfg, B, dev)
        assert eng.fuse_head == flag
        eng.P.set_weights(p)
        eng.loss_and_grads(*(T(a, dev) for a in args_np))
        torch.cuda.synchronize()
        res.append((eng.losses(), eng.P.get_weights(eng.P.grads), N(eng.logits)))
    for k in res[0][0]:
        assert abs(res[0][0][k] - res[1][0][k]) <= 1e-4 * max(1.0, abs(res[1][0][k])), k
    np.testing.assert_allclose(res[0][2], res[1][2], rtol=1e-5, atol=1e-5)
    for k in res[0][1]:
        scale = np.abs(res[1][1][k]).max() + 1e-12
        assert np.abs(res[0][1][k] - res[1][1][k]).max() <= 2e-5 * scale, k


def test_cl_vrnn_step_is_graph_replayable(dev):
    """The whole step enqueues kernels only: capture once, replay, same numbers."""
    from clvae_amd import ops
    from clvae_amd.engine import VrnnEngine
    cfg = O.vrnn_config(latent_dim=2, seq_length=16, n_classes=10, use_x_prev=True)
    B, Tn = 8, 16
    rng = np.random.default_rng(5)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=3).items()}
    win = frames(rng, B, Tn + 1, 88)
    args_np = (win[:, 1:].copy(), win[:, :-1].copy(), np.eye(10)[rng.integers(0, 10, B)],
               rng.standard_normal((B, 9)), rng.standard_normal((B, Tn, 2)))
    eng = VrnnEngine(cfg, B, dev)
    eng.P.set_weights(p)
    args = tuple(T(a, dev) for a in args_np)
    eng.loss_and_grads(*args)              # warm-up: sizes every workspace
    eng.P.adam_step()
    torch.cuda.synchronize()
    eng.P.set_weights(p); eng.P.reset_optimizer()
    with ops.Graph() as gr:
        eng.loss_and_grads(*args)
        eng.P.adam_step()
    for _ in range(3):
        gr.launch()
    torch.cuda.synchronize()
    w_graph = eng.P.get_weights()
    eng.P.set_weights(p); eng.P.reset_optimizer()
    for _ in range(3):
        eng.loss_and_grads(*args)
        eng.P.adam_step()
    torch.cuda.synchronize()
    w_eager = eng.P.get_weights()
    for k in w_graph:
        np.testing.assert_array_equal(w_graph[k], w_eager[k])
    assert int(eng.P.iterations.item()) == 3


def test_cl_vrnn_dp_graph_schedule_matches_single_graph(dev, monkeypatch):
    """The multi-GPU schedule (three graphs around the two gradient buckets) gives the same weights as the
    single-graph step when the collectives are no-ops (one GPU)."""
    from clvae_amd.engine import VrnnEngine
    from clvae_amd.trainer import TrainStep
    cfg = O.vrnn_config(latent_dim=2, seq_length=12, n_classes=10, use_x_prev=True)
    B, Tn = 8, 12
    rng = np.random.default_rng(9)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=4).items()}
    win = frames(rng, B, Tn + 1, 88)
    X, Xp, wt = T(win[:, 1:], dev), T(win[:, :-1], dev), T(np.eye(10)[rng.integers(0, 10, B)], dev)
    out = []
    for force, fast in (('0', False), ('1', False), ('0', True), ('1', True)):
        monkeypatch.setenv('CLV_FORCE_DP_GRAPHS', force)
        eng = VrnnEngine(cfg, B, dev)
        eng.P.set_weights(p)
        ts = TrainStep(eng, seed=77, fast_adam=fast)
        assert (ts.ar is not None) == (force == '1')
        for _ in range(4):
            ts.stage_batch(X, Xp, wt)
            ts.step()
        torch.cuda.synchronize()
        assert eng.P.norms_valid          # whole steps and (round 3) the split ones keep the hW kernel's column norms
        assert ts.pre_in_tail             # ... and the optimizer's sum g.V travels with the hW kernel's gradient bucket
        out.append(eng.P.get_weights())
    for k in out[0]:
        np.testing.assert_array_equal(out[0][k], out[1][k])
        # the single-GPU default: Adam-WN of the hW kernel in two launches, its first column sums taken from the backward
        # pass (sum over the batch of pre-activation x gradient) and from the previous step's norms: the same update up to
        # the rounding of those sums
        np.testing.assert_allclose(out[2][k], out[0][k], rtol=2e-5, atol=2e-7, err_msg=k)
        # the multi-GPU schedule takes the same two-launch form for its hW piece (same kernels, same sums)
        np.testing.assert_array_equal(out[3][k], out[2][k])


def test_cl_vrnn_dp_graph_schedule_with_dense_inputs(dev, monkeypatch):
    """The replayed data-parallel schedule with the DENSE hW path (sparse_inputs=False): its backward pass never writes
    the optimizer's sum g.V, so the hW piece of the split update must take the five-launch form -- the replay used to
    claim the sum was fresh (round-3 advice).  Same weights as the single-graph step, bitwise."""
    from clvae_amd.engine import VrnnEngine
    from clvae_amd.trainer import TrainStep
    cfg = O.vrnn_config(latent_dim=2, seq_length=12, n_classes=10, use_x_prev=True)
    cfg['sparse_inputs'] = False
    B, Tn = 8, 12
    rng = np.random.default_rng(19)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=6).items()}
    win = frames(rng, B, Tn + 1, 88)
    X, Xp, wt = T(win[:, 1:], dev), T(win[:, :-1], dev), T(np.eye(10)[rng.integers(0, 10, B)], dev)
    out = []
    for force in ('0', '1'):
        monkeypatch.setenv('CLV_FORCE_DP_GRAPHS', force)
        eng = VrnnEngine(cfg, B, dev)
        assert not eng.sparse_inputs
        eng.P.set_weights(p)
        ts = TrainStep(eng, seed=78)
        for _ in range(5):
            ts.stage_batch(X, Xp, wt)
            ts.step()
        torch.cuda.synchronize()
        assert not eng.gdot_fresh
        if force == '1':
            assert ts._main_leaves_gdot is False
        out.append(eng.P.get_weights())
    for k in out[0]:
        np.testing.assert_array_equal(out[0][k], out[1][k])


def test_adam_step_in_two_pieces_is_bitwise_the_whole_step(dev):
    """FlatParams.adam_step(only=..., advance=False) then the rest == one call (per-tensor independence of Adam-WN,
    `iterations` advanced once): the multi-GPU schedule updates the hW kernel while the other bucket is still reduced."""
    from clvae_amd.engine import VrnnEngine
    cfg = O.vrnn_config(latent_dim=2, seq_length=6, n_classes=4, use_x_prev=True)
    rng = np.random.default_rng(3)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=5).items()}
    res = []
    for split in (False, True):
        eng = VrnnEngine(cfg, 4, dev)
        eng.P.set_weights(p)
        g = torch.as_tensor(np.random.default_rng(9).standard_normal(eng.P.n).astype(np.float32), device=dev)
        for it in range(3):
            eng.P.grads.copy_(g * (it + 1))
            if split:
                eng.P.adam_step(only=['hW/kernel'], advance=False)
                eng.P.adam_step(only=[n for n, _ in eng.P.shapes if n != 'hW/kernel'])
            else:
                eng.P.adam_step()
        torch.cuda.synchronize()
        assert int(eng.P.iterations.item()) == 3
        res.append((eng.P.get_weights(), eng.P.m.cpu().numpy(), eng.P.s.cpu().numpy()))
    for k in res[0][0]:
        np.testing.assert_array_equal(res[0][0][k], res[1][0][k])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    np.testing.assert_array_equal(res[0][2], res[1][2])


@pytest.mark.parametrize("B,L,Cn", [(100, 4, 2), (37, 16, 16), (1, 3, 5), (17, 1, 2)])
def test_cl_vae_fused_step_draws_its_own_noise_and_advances_the_counter(dev, B, L, Cn):
    """clv_vae_fused_step(opts): the in-kernel Philox draw writes the values clv_philox_normal2 writes (bit for bit), the
    folded loss means equal clv_loss_sums', and bump + adam_step(advanced=True) is adam_step()."""
    from clvae_amd import ops
    from clvae_amd.engine import VaeEngine
    cfg = O.vae_config(latent_dim=L, n_classes=Cn, use_x_prev=True)
    rng = np.random.default_rng(5)
    p = {k: f32(v) for k, v in O.vae_init_params(cfg, seed=2).items()}
    x, xp = frames(rng, B, 88), frames(rng, B, 88)
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    a, b = VaeEngine(cfg, B, dev), VaeEngine(cfg, B, dev)
    assert a.fused and a.folds_step(True)
    for e in (a, b):
        e.P.set_weights(p)
        e.P.iterations.fill_(7)
    xs = (T(x, dev), T(xp, dev), T(wt, dev))
    C1 = Cn - 1
    seed, sw, sz, fw, fz = 0x1234567890, 4, 5, 3 * C1, 3 * L
    ew, ez = torch.empty(B, C1, device=dev), torch.empty(B, L, device=dev)
    ops.philox_normal2(ew, B * C1, sw, fw, ez, B * L, sz, fz, seed, 0, step_dev=a.P.iterations)
    a.loss_and_grads(*xs, ew, ez)
    a.P.adam_step()
    ew2, ez2 = torch.zeros(B, C1, device=dev), torch.zeros(B, L, device=dev)
    b.loss_and_grads(*xs, ew2, ez2, noise=(seed, sw, sz, fw, fz, 0, b.P.iterations), bump=True)
    torch.cuda.synchronize()
    assert int(b.P.iterations.item()) == 8
    b.P.adam_step(advanced=True)
    torch.cuda.synchronize()
    assert torch.equal(ew, ew2) and torch.equal(ez, ez2)
    assert torch.equal(a.P.grads, b.P.grads)
    la, lb = a.losses(), b.losses()
    assert all(la[k] == lb[k] for k in la)
    assert int(a.P.iterations.item()) == int(b.P.iterations.item()) == 8
    assert torch.equal(a.P.params, b.P.params)
    # the means of the folded launch against a plain sum of the per-row arrays
    assert abs(lb['vae'] - float(b.rownll.double().mean())) < 1e-4 * max(1.0, abs(lb['vae']))
    assert abs(lb['kl_z'] - float(b.rowkl.double().mean())) < 1e-5 * max(1.0, abs(lb['kl_z']))


@pytest.mark.parametrize("B,Tn,L,pair", [(6, 16, 2, True), (5, 7, 8, True), (4, 8, 12, False)])
def test_cl_vrnn_step_draws_its_own_noise(dev, B, Tn, L, pair):
    """loss_and_grads(noise=...): eps_W is drawn inside the label kernel and eps_Z inside the pair kernel (no Philox launch
    in the step) -- bit for bit the values clv_philox_normal2 writes at the same (seed, streams, first indices, step),
    and therefore the same losses and gradients as a step that is given those tensors.  pair=False (latent_dim > 8):
    the engine falls back to one Philox launch of its own, same values."""
    from clvae_amd import ops
    from clvae_amd.engine import VrnnEngine
    Cn = 10
    cfg = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=True)
    rng = np.random.default_rng(B * 100 + L)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=4).items()}
    win = frames(rng, B, Tn + 1, 88)
    X, Xp = win[:, 1:].copy(), win[:, :-1].copy()
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    a, b = VrnnEngine(cfg, B, dev), VrnnEngine(cfg, B, dev)
    assert a.fuse_pair == pair and b.folds_noise() == pair
    for e in (a, b):
        e.P.set_weights(p)
        e.P.iterations.fill_(11)
    C1 = Cn - 1
    row0 = 3                                    # as if this were the second rank of a data-parallel group
    seed, sw, sz, fw, fz = 0xABCDEF012345, 2, 3, row0 * C1, row0 * Tn * L
    ew, ez = torch.empty(B, C1, device=dev), torch.empty(B * Tn, L, device=dev)
    ops.philox_normal2(ew, B * C1, sw, fw, ez, B * Tn * L, sz, fz, seed, 0, step_dev=a.P.iterations)
    xs = (T(X, dev), T(Xp, dev), T(wt, dev))
    a.loss_and_grads(*xs, ew, ez)
    ew2, ez2 = torch.zeros(B, C1, device=dev), torch.zeros(B * Tn, L, device=dev)
    b.loss_and_grads(*xs, ew2, ez2, noise=(seed, sw, sz, fw, fz, 0, b.P.iterations))
    torch.cuda.synchronize()
    assert torch.equal(ew, ew2) and torch.equal(ez, ez2)
    assert torch.equal(a.P.grads, b.P.grads)
    la, lb = a.losses(), b.losses()
    assert all(la[k] == lb[k] for k in la)


@pytest.mark.parametrize("B,Tn,L,use_x_prev,dense", [(6, 16, 2, True, 0.0443), (5, 7, 8, True, 0.15), (4, 9, 3, False, 0.0443),
                                                     (256, 128, 2, True, 0.0443)])
def test_cl_vrnn_step_from_note_lists_matches_oracle(dev, B, Tn, L, use_x_prev, dense):
    """The fused input projections (cfg['fuse_notes']): the batch is staged from byte frames, the staging launch writes
    the frames' note lists, and the pair forward kernel gathers both LSTM input projections from them (no projection
    launch); noise drawn in the kernels.  Against the fp64 oracle on the same frames / noise: losses, logits, states, every
    gradient.  Odd sequence lengths, frames with more than 8 notes (dense = 0.15: 13 on average), a decoder without
    history frames, and the benchmark's shape."""
    from clvae_amd import ops
    from clvae_amd.engine import VrnnEngine
    from clvae_amd.trainer import TrainStep
    Cn = 10
    cfg = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=use_x_prev)
    cfg['fuse_notes'] = True                # opt-in: slower than the projection launch on MI355X (see VrnnEngine)
    rng = np.random.default_rng(B + Tn + L)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=5).items()}
    win = (rng.random((B, Tn + 1, 88)) < dense).astype(np.uint8)
    win[0, 1] = 0                                           # a frame without notes
    if dense > 0.1:
        win[1, 2] = 1                                       # and one with all 88
    wt = np.eye(Cn, dtype=np.float32)[rng.integers(0, Cn, B)]
    eng = VrnnEngine(cfg, B, dev)
    assert eng.fuse_pair and eng.fuse_notes
    eng.P.set_weights(p)
    eng.P.iterations.fill_(3)
    ts = TrainStep(eng, seed=77, use_graph=False)
    d_win = torch.as_tensor(win, device=dev)
    ts.stage_batch(d_win[:, 1:].contiguous(), d_win[:, :-1].contiguous(), torch.as_tensor(wt, device=dev))
    assert eng.notes_valid
    ts._main()                                              # noise + forward + losses + backward (early part)
    ts._tail()
    torch.cuda.synchronize()
    X, Xp = win[:, 1:].astype(np.float64), win[:, :-1].astype(np.float64)
    eW, eZ = f32(N(ts.eps_w)), f32(N(ts.eps_z)).reshape(B, Tn, L)
    seed, sw, sz, fw, fz, step, _ = ts.noise_spec()
    np.testing.assert_allclose(N(ts.eps_z).ravel(), OP.normal(B * Tn * L, seed, 3, sz, fz), atol=2e-5)
    ref = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt.astype(np.float64), eW, eZ)
    got = eng.losses()
    for k in ('elbo', 'vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
        assert abs(got[k] - ref[k]) <= ELBO_TOL, (k, got[k], ref[k])
    assert np.abs(N(eng.logits).reshape(B, Tn, 88) - ref['cache']['logits']).max() < LOGIT_TOL
    np.testing.assert_allclose(N(eng.hs_enc).reshape(B, Tn, 88), ref['cache']['enc_h'], atol=5e-5)
    np.testing.assert_allclose(N(eng.hs_dec).reshape(B, Tn, 88), ref['cache']['dec_h'], atol=5e-5)
    check_grads(eng.P.get_weights(eng.P.grads), ref['grads'], tol=3e-4)
    # the same step from the same bytes without the lists (projection launch): the two paths agree to rounding
    eng2 = VrnnEngine(dict(cfg, fuse_notes=False), B, dev)
    eng2.P.set_weights(p)
    eng2.P.iterations.fill_(3)
    ts2 = TrainStep(eng2, seed=77, use_graph=False)
    ts2.stage_batch(d_win[:, 1:].contiguous(), d_win[:, :-1].contiguous(), torch.as_tensor(wt, device=dev))
    assert not eng2.fuse_notes and not eng2.notes_valid
    ts2._main(); ts2._tail()
    torch.cuda.synchronize()
    assert abs(eng2.losses()['elbo'] - got['elbo']) < 1e-4
    np.testing.assert_allclose(N(eng2.hs_dec), N(eng.hs_dec), atol=2e-5)


def test_cl_vae_bf16_step_tolerance(dev):
    """BASELINE configuration 2 names bf16 for the encoder / decoder products: cfg['bf16'] rounds the operands of every
    Dense product and weight-gradient product of the fused step to bf16 (fp32 accumulate, fp32 everything else).  Its
    distance from the fp64 oracle on the config-2 shape (measured: |dELBO| 7e-4 nats per frame, logits 5e-3, gradient
    tensors 5 % of their largest entry; the fp32 path: 2e-6, 3e-7, 1e-7) is bounded at about twice that."""
    from clvae_amd.engine import VaeEngine
    B, L, Cn = 512, 4, 2
    cfg = O.vae_config(latent_dim=L, n_classes=Cn, use_x_prev=True)
    rng = np.random.default_rng(21)
    p = {k: f32(v) for k, v in O.vae_init_params(cfg, seed=3).items()}
    x, xp = frames(rng, B, 88), frames(rng, B, 88)
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    ew, ez = f32(rng.standard_normal((B, Cn - 1))), f32(rng.standard_normal((B, L)))
    ref = O.vae_loss_and_grads(p, cfg, x, xp, wt, ew, ez)
    errs = {}
    for bf16 in (False, True):
        eng = VaeEngine(dict(cfg, bf16=bf16), B, dev)
        assert eng.fused
        eng.P.set_weights(p)
        eng.loss_and_grads(T(x, dev), T(xp, dev), T(wt, dev), T(ew, dev), T(ez, dev))
        torch.cuda.synchronize()
        got = eng.losses()
        g = eng.P.get_weights(eng.P.grads)
        errs[bf16] = (abs(got['elbo'] - ref['elbo']), np.abs(N(eng.logits) - ref['cache']['logits']).max(),
                      max(np.abs(g[k] - ref['grads'][k]).max() / (np.abs(ref['grads'][k]).max() + 1e-12) for k in ref['grads']))
    print("cl_vae config 2 vs fp64 oracle (|dELBO|, max |dlogit|, max rel grad err): fp32 %.2e %.2e %.2e | bf16 %.2e %.2e %.2e"
          % (errs[False] + errs[True]))
    assert errs[False][0] <= ELBO_TOL and errs[False][2] < 1e-4
    assert errs[True][0] <= 2e-3 and errs[True][1] <= 1e-2 and errs[True][2] <= 1e-1
    assert errs[True][2] > errs[False][2]          # the bf16 path really is the one that ran


def test_cl_vae_fused_loss_only_pass_takes_its_means_in_one_launch(dev):
    """need_grads=False through clv_vae_fused_step(opts): no gradients, no counter bump, the five loss means from the tail
    launch alone -- equal to the training pass's on the same inputs."""
    from clvae_amd.engine import VaeEngine
    B, L, Cn = 50, 4, 2
    cfg = O.vae_config(latent_dim=L, n_classes=Cn, use_x_prev=True)
    rng = np.random.default_rng(9)
    p = {k: f32(v) for k, v in O.vae_init_params(cfg, seed=4).items()}
    eng = VaeEngine(cfg, B, dev)
    eng.P.set_weights(p)
    args = (T(frames(rng, B, 88), dev), T(frames(rng, B, 88), dev), T(np.eye(Cn)[rng.integers(0, Cn, B)], dev),
            T(rng.standard_normal((B, Cn - 1)), dev), T(rng.standard_normal((B, L)), dev))
    eng.P.iterations.fill_(3)
    eng.loss_and_grads(*args)
    torch.cuda.synchronize()
    train = eng.losses()
    eng.P.grads.fill_(123.0)
    eng.loss_and_grads(*args, need_grads=False, bump=True)
    torch.cuda.synchronize()
    ev = eng.losses()
    assert all(train[k] == ev[k] for k in train)
    assert float(eng.P.grads.min()) == 123.0 and int(eng.P.iterations.item()) == 3
