"""CPU: tests/label_reference.py, the fp64 reference of the label head kernels, against the oracle's cl_vrnn step -- and the
sensitivity of the comparison tests/test_gpu_label_head.py makes (per-element bounds, hit outside near ties, per slice), so
that the GPU test is known to catch subtle faults without a GPU."""
import numpy as np
import pytest

from oracle import clvae_oracle as O
import label_reference as LR


def _oracle_step(use_x_prev, seed):
    cfg = O.vrnn_config(latent_dim=2, seq_length=3, n_classes=5, use_x_prev=use_x_prev, w_log_var_prior=0.3)
    rng = np.random.default_rng(seed)
    p = O.vrnn_init_params(cfg, seed=seed)
    B, T, D, L, C = 6, cfg['T'], cfg['D'], cfg['L'], cfg['C']
    win = (rng.random((B, T + 1, D)) < 0.1).astype(np.float64)
    X, Xp = win[:, 1:], win[:, :-1]
    wt = np.eye(C)[rng.integers(0, C, B)]
    eW, eZ = rng.standard_normal((B, C - 1)), rng.standard_normal((B, T, L))
    ref = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt, eW, eZ, need_grads=False)
    off = D if use_x_prev else 0
    Ke, Kd = p['encoder_h/kernel'], p['decoder_h/kernel']
    lab = LR.forward(p['Wargs/kernel'], p['Wargs/bias'], eW, wt, cfg['w_log_var_prior'], Ke[D:], p['encoder_h/bias'],
                     Kd[off + L:], p['decoder_h/bias'], X=X.reshape(B, T * D), Kh=p['hW/kernel'], bh=p['hW/bias'])
    return ref, lab, p, D, off, L


@pytest.mark.parametrize("use_x_prev", [True, False])
def test_label_reference_is_the_oracle_forward(use_x_prev):
    ref, lab, p, D, off, L = _oracle_step(use_x_prev, 3 + use_x_prev)
    c = ref['cache']
    tol = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lab['hW'], c['hW'], **tol)
    np.testing.assert_allclose(lab['wargs'], c['Wargs'], **tol)
    np.testing.assert_allclose(lab['W'], c['W'], **tol)
    np.testing.assert_allclose(lab['rowloss'][:, 0].mean(), ref['kl_w'], **tol)
    np.testing.assert_allclose(lab['rowloss'][:, 1].mean(), ref['w_rec'], **tol)
    assert lab['rowloss'][:, 2].mean() == ref['acc']
    # the per-row LSTM biases as tests/test_pair_reference.py forms them
    np.testing.assert_allclose(lab['rb_enc'], c['W'] @ p['encoder_h/kernel'][D:] + p['encoder_h/bias'], **tol)
    np.testing.assert_allclose(lab['rb_dec'], c['W'] @ p['decoder_h/kernel'][off + L:] + p['decoder_h/bias'], **tol)
    for k in LR.OUTPUTS:
        assert (lab['b_' + k] >= 0).all() and np.isfinite(lab['b_' + k]).all(), k


# ---- sensitivity ----
B, C, D, T = 9, 6, 12, 7          # nx = 84: a ragged last chunk of 20 inputs
NX = T * D
TIE, CLIP_LO, CLIP_HI = 4, 5, 6   # rows: exact tie (no notes, eps = 0), true class starved, true class saturated


def _case():
    rng = np.random.default_rng(11)
    X = (rng.random((B, NX)) < 0.15).astype(np.float64)
    X[:, -1] = 0.0
    X[0, -1] = 1.0                  # row 0's last input is its row's last element: inside the ragged chunk
    X[1, :] = 0.0                   # an empty row: hW = relu(bh)
    X[TIE, :] = 0.0
    f = lambda a: np.asarray(a, np.float32).astype(np.float64)
    Kh = f(rng.standard_normal((NX, D)) * 0.4)
    Kh[-1] = f(rng.standard_normal(D) * 0.4 + 1.0)
    bh = f(-np.abs(rng.standard_normal(D)) * 0.1)   # bh <= 0: the empty rows have hW = 0
    bh[:3] = 0.2
    Ka = f(rng.standard_normal((D, 2 * (C - 1))) * 0.3)
    Ka[:3] = 0.0                    # the empty rows get wargs = ba exactly
    ba = np.zeros(2 * (C - 1))
    eps = f(rng.standard_normal((B, C - 1)))
    eps[TIE] = 0.0                  # W = 1/C in every class, exactly
    onehot = np.eye(C)[rng.integers(0, C, B)]
    onehot[TIE] = np.eye(C)[0]      # first-index rule: hit = 1; the last index would give 0
    onehot[CLIP_LO] = np.eye(C)[0]
    onehot[CLIP_HI] = np.eye(C)[1]
    eps[CLIP_LO] = [-40.0, 0.0, 0.0, 0.0, 0.0]     # W[0] ~ e^-40 / C: n below 1e-7
    eps[CLIP_HI] = [0.0, 40.0, 0.0, 0.0, 0.0]      # W[1] ~ 1 - 4 e^-40: n above 1 - 1e-7
    Kenc_w, Kdec_w = f(rng.standard_normal((C, 40)) * 0.2), f(rng.standard_normal((C, 40)) * 0.2)
    benc, bdec = f(rng.standard_normal(40) * 0.1), f(rng.standard_normal(40) * 0.1)
    args = dict(Ka=Ka, ba=ba, eps=eps, onehot=onehot, prior=0.2, Kenc_w=Kenc_w, benc=benc, Kdec_w=Kdec_w, bdec=bdec,
                X=X, Kh=Kh, bh=bh)
    return args, LR.forward(**args), LR.forward(**args, dtype=np.float32)


@pytest.fixture(scope="module")
def case():
    return _case()


def test_the_case_exercises_the_edges(case):
    args, ref, _ = case
    assert (ref['hW'][1] == np.maximum(args['bh'], 0)).all() and (ref['hW'][TIE] == np.maximum(args['bh'], 0)).all()
    assert (ref['wargs'][TIE] == 0).all() and (ref['W'][TIE] == 1.0 / C).all() and not ref['tie'][TIE]
    assert ref['rowloss'][TIE, 2] == 1.0
    n = (ref['W'] + 1e-10) / (ref['W'] + 1e-10).sum(1, keepdims=True)
    assert n[CLIP_LO, 0] < O.EPS_K and n[CLIP_HI, 1] > 1 - O.EPS_K


def test_fp32_evaluation_passes(case):
    """the same contract evaluated in fp32 (another order of every sum) is within the bounds"""
    _, ref, got = case
    ratios = LR.check_forward(got, ref, 'fp32 ')
    assert max(ratios.values()) < 0.5, ratios


def _faulty(case, k):
    args, ref, got = case
    g = {kk: np.array(v, copy=True) for kk, v in got.items()}
    if k == 0:                                     # one rb_dec column off by 1e-4 relative
        g['rb_dec'][:, 7] *= 1 + 1e-4
    elif k == 1:                                   # two classes of W swapped
        g['W'][:, [2, 3]] = g['W'][:, [3, 2]]
    elif k == 2:                                   # the last input of the ragged row dropped from hW
        a = dict(args)
        a['X'] = args['X'].copy()
        a['X'][0, -1] = 0.0
        g = LR.forward(**a, dtype=np.float32)
    elif k == 3:                                   # eps read one row off
        eps = args['eps'].copy()
        eps[:TIE] = np.roll(eps[:TIE], 1, 0)      # (among the ordinary rows)
        a = dict(args, eps=eps)
        g = LR.forward(**a, dtype=np.float32)
    elif k == 4:                                   # w_rec without the clip
        W = g['W'].astype(np.float64)
        n = (W + 1e-10) / (W + 1e-10).sum(1, keepdims=True)
        g['rowloss'][:, 1] = -(C - 1) * (args['onehot'] * np.log(n)).sum(1)
    elif k == 5:                                   # a tie broken to the last index
        W = g['W']
        am = W.shape[1] - 1 - np.argmax(W[:, ::-1], 1)
        g['rowloss'][:, 2] = (am == np.argmax(args['onehot'], 1)).astype(np.float32)
    return g


FAULTS = ["rb_dec column off by 1e-4", "two W classes swapped", "ragged last input dropped", "eps one row off",
          "w_rec without the clip", "tie broken to the last index"]


@pytest.mark.parametrize("k", range(len(FAULTS)), ids=FAULTS)
def test_planted_fault_is_caught(case, k):
    _, ref, _ = case
    with pytest.raises(AssertionError):
        LR.check_forward(_faulty(case, k), ref, FAULTS[k] + ': ')


def test_near_tie_rows_are_flagged():
    """two classes whose fp64 W differ by less than their bounds: the row is flagged and its hit not judged"""
    C_ = 3
    Ka, ba = np.zeros((2, 2 * (C_ - 1))), np.zeros(2 * (C_ - 1))
    eps = np.array([[1e-9, 0.0], [0.5, 0.0]])
    r = LR.forward(Ka, ba, eps, np.eye(C_)[[1, 0]], 0.0, np.ones((C_, 8)), np.zeros(8), np.ones((C_, 8)), np.zeros(8),
                   hW=np.zeros((2, 2)))
    assert r['tie'].tolist() == [True, False]


def test_stage_rows_and_assembly():
    """the cursor's batch with step < step0 (the mathematical modulo), idx / row0, tables, strides and offsets, pieces"""
    assert LR.stage_rows(3, row0=5).tolist() == [5, 6, 7]
    # (1 - 8) mod 3 = 2: base = 2 * 4 + 1
    assert LR.stage_rows(2, row0=100, cursor=(1, 8, 3, 4, 1)).tolist() == [109, 110]
    idx = np.arange(40)[::-1]
    assert LR.stage_rows(2, idx=idx, row0=100, cursor=(1, 8, 3, 4, 1)).tolist() == [idx[9], idx[10]]
    store = np.arange(60, dtype=np.uint8)
    table = np.array([3, 0, 1, 2])
    a = LR.assemble(np.array([1, 3]), 4, (store, 10, 2, table), hist=(store, 8, 4, None), hist_chunk=2, hist_ld=3,
                    w_src=np.arange(8.0).reshape(4, 2))
    assert a['X8'].tolist() == [[2, 3, 4, 5], [22, 23, 24, 25]]
    assert a['Xh8'].tolist() == [[12, 13, 14, 15], [28, 29, 30, 31]]
    assert np.array_equal(a['Xh'][:, :2], [[12, 13], [14, 15], [28, 29], [30, 31]]) and np.isnan(a['Xh'][:, 2]).all()
    assert a['w_out'].tolist() == [[2, 3], [6, 7]]
