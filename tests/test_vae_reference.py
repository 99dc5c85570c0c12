"""CPU: tests/vae_reference.py, the fp64 reference of the fused cl_vae step, against the oracle's step -- and the sensitivity
of the comparison tests/test_gpu_vae_fused.py makes (every output element within its own bound, hit exactly outside near
ties): an fp32 evaluation of the contract passes it in each mode, planted faults do not."""
import numpy as np
import pytest

from oracle import clvae_oracle as O
import vae_reference as VR

# (B, D, H, Hc, C, L, use_x_prev, target)
SHAPES = [(9, 12, 20, 7, 3, 2, False, False), (17, 20, 24, 12, 5, 3, True, True), (6, 10, 6, 14, 16, 16, True, False),
          (5, 7, 9, 5, 2, 1, False, True), (33, 23, 17, 30, 7, 9, True, True)]


def _oracle(case):
    P, C, L = case['P'], case['onehot'].shape[1], case['eps_z'].shape[1]
    D, H, Hc = case['x'].shape[1], P[4].shape[1], P[0].shape[1]
    cfg = O.vae_config(original_dim=D, intermediate_dim=H, latent_dim=L, intermediate_class_dim=Hc, n_classes=C,
                       use_x_prev=case['use_x_prev'], class_weight=case['class_weight'], kl_weight=case['kl_weight'],
                       w_kl_weight=case['w_kl_weight'], w_log_var_prior=case['prior'])
    C1 = C - 1
    p = {'h_w/kernel': P[0], 'h_w/bias': P[1], 'w_mean/kernel': P[2][:, :C1], 'w_log_var/kernel': P[2][:, C1:],
         'w_mean/bias': P[3][:C1], 'w_log_var/bias': P[3][C1:], 'h/kernel': P[4], 'h/bias': P[5],
         'z_mean/kernel': P[6][:, :L], 'z_log_var/kernel': P[6][:, L:], 'z_mean/bias': P[7][:L], 'z_log_var/bias': P[7][L:],
         'decoder_h/kernel': P[8], 'decoder_h/bias': P[9], 'x_decoded_mean/kernel': P[10], 'x_decoded_mean/bias': P[11]}
    np.testing.assert_array_equal(np.concatenate([VR.fuse(p)[i].ravel() for i in range(12)]),
                                  np.concatenate([t.ravel() for t in P]))
    return O.vae_loss_and_grads(p, cfg, case['x'], case['xp'], case['onehot'], case['eps_w'], case['eps_z'],
                                target=case['target'])


@pytest.mark.parametrize("shape", SHAPES)
def test_vae_reference_is_the_oracle_step(shape):
    B, D, H, Hc, C, L, uxp, tgt = shape
    case = VR.make_case(B + D, B, D, H, Hc, C, L, uxp, target=tgt)
    ref, r = _oracle(case), VR.call(VR.reference, case)
    c = ref['cache']
    tol = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r['logits'], c['logits'], **tol)
    np.testing.assert_allclose(r['w'], c['w'], **tol)
    np.testing.assert_allclose(r['wargs'], np.concatenate([c['w_mean'], c['w_log_var']], 1), **tol)
    np.testing.assert_allclose(r['zargs'], np.concatenate([c['z_mean'], c['z_log_var']], 1), **tol)
    np.testing.assert_allclose(r['rownll'].mean(), ref['vae'], **tol)
    np.testing.assert_allclose(r['rowkl'].mean(), ref['kl_z'], **tol)
    np.testing.assert_allclose(r['rowloss'][:, 0].mean(), ref['kl_w'], **tol)
    np.testing.assert_allclose(r['rowloss'][:, 1].mean(), ref['w_rec'], **tol)
    assert r['rowloss'][:, 2].mean() == ref['acc']
    g = VR.unfuse_grads(r['grads'], C, L)
    for k, v in ref['grads'].items():
        np.testing.assert_allclose(g[k], v, err_msg=k, **tol)
    for k in VR.OUTPUTS:
        assert (r['b_' + k] >= 0).all() and np.isfinite(r['b_' + k]).all(), k
    assert all(np.isfinite(b).all() and (b >= 0).all() for b in r["b_grads"])


def test_vae_reference_scores_the_target_and_drops_w_rec_without_labels():
    case = VR.make_case(3, 12, 16, 10, 8, 4, 3, False, target=True)
    a = VR.call(VR.reference, case)
    b = VR.call(VR.reference, dict(case, target=None))
    assert not np.allclose(a['rownll'], b['rownll'])
    np.testing.assert_array_equal(a['logits'], b['logits'])
    n = VR.call(VR.reference, dict(case, onehot=None), need_grads=False)
    assert (n['rowloss'][:, 1:] == 0).all() and 'grads' not in n
    np.testing.assert_array_equal(n['rowloss'][:, 0], a['rowloss'][:, 0])


def test_layout_places_tensors_with_gaps():
    shp = VR.shapes(7, 5, 6, 3, 2, True)
    ts = [np.arange(np.prod(s), dtype=np.float64).reshape(s) + 100 * i for i, s in enumerate(shp)]
    order, gaps = list(range(11, -1, -1)), [3, 1, 5, 2, 7, 1, 1, 3, 2, 9, 1, 4]
    offs, n = VR.layout(shp, order, gaps)
    flat = VR.scatter(ts, offs, n, fill=np.nan, dtype=np.float64)
    for a, b in zip(VR.gather(flat, offs, shp), ts):
        np.testing.assert_array_equal(a, b)
    gm = VR.gap_mask(offs, shp, n)
    assert gm.sum() == sum(gaps) + gaps[-1] and np.isnan(flat[gm]).all()      # gaps[-1] also behind the last


# ---- fp32 evaluations against the bounds ----
def _check(got, ref, name):
    bad = VR.violations(got, ref)
    assert not bad, "%s: %s" % (name, bad)
    rt = VR.ratios(got, ref)
    print("%s: worst error / bound %.3g (%s), flags %s" % (name, max(rt.values()), max(rt, key=rt.get), VR.flag_counts(ref)))
    return rt


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", SHAPES + [(40, 94, 90, 70, 16, 16, False, True), (21, 88, 88, 88, 2, 4, True, False)])
def test_fp32_evaluation_stays_within_bounds(shape, bf16):
    B, D, H, Hc, C, L, uxp, tgt = shape
    case = VR.make_case(7 * B + C, B, D, H, Hc, C, L, uxp, target=tgt)
    ref = VR.call(VR.reference, case, bf16_mode=bf16)
    for seed in range(2):
        _check(VR.call(VR.evaluate32, case, bf16_mode=bf16, seed=seed), ref, "%s bf16=%d" % (shape, bf16))


@pytest.mark.parametrize("bf16", [False, True])
def test_edges_stay_within_bounds(bf16):
    case = VR.edge_case()
    ref = VR.call(VR.reference, case, bf16_mode=bf16)
    assert (ref['logits'][:, 0] > O.LOGIT_CLIP_HI).all() and (ref['logits'][:, 1] < O.LOGIT_CLIP_LO).all()
    assert (ref['grads'][11][:2] == 0).all()
    np.testing.assert_array_equal(ref['w'][2], np.full(5, 0.2))
    assert ref['rowloss'][2, 2] == 0 and ref['w'][3, 0] < 1e-20         # first index on both ties; row 3 clipped
    _check(VR.call(VR.evaluate32, case, bf16_mode=bf16, seed=1), ref, "edges bf16=%d" % bf16)


# ---- planted faults ----
BASE = (34, 20, 24, 12, 5, 3, True)            # D = 20: the output layer's last 16-column tile is partial (4 columns)


def _base(target=True):
    return VR.make_case(21, *BASE, target=target)


def _rejected(got, ref, what):
    bad = VR.violations(got, ref)
    assert bad, "planted fault not rejected: " + what
    print("%s -> rejected by %s" % (what, bad[:3]))


def test_planted_fault_last_partial_tile_column():
    case = _base()
    ref = VR.call(VR.reference, case)
    got = VR.call(VR.evaluate32, case)
    g = [a.astype(np.float64).copy() for a in got['grads']]
    g[10][:, 19] += 2 * ref['b_grads'][10][:, 19]
    _rejected(dict(got, grads=g), ref, "x_decoded_mean/kernel column 19 off by 2 bounds")


def test_planted_fault_rowkl_row_15():
    case = _base()
    ref = VR.call(VR.reference, case)
    _rejected(VR.call(VR.evaluate32, case, faults=('rowkl_drop_last',)), ref, "rowkl of row 31 without its last term")


def test_planted_fault_wargs_halves_swapped():
    case = _base()
    ref = VR.call(VR.reference, case)
    got = VR.call(VR.evaluate32, case)
    wa = got['wargs']
    C1 = wa.shape[1] // 2
    _rejected(dict(got, wargs=np.concatenate([wa[:, C1:], wa[:, :C1]], 1)), ref, "wargs halves swapped")


def test_planted_fault_padding_row_in_a_bias_gradient():
    case = _base()
    B = case['x'].shape[0]
    ref = VR.call(VR.reference, case)
    got = VR.call(VR.evaluate32, case)
    # what a padding row of the ragged last tile (no frames, no noise, no label) would add to the output layer's bias
    pad = {k: (v[:1] * 0 if isinstance(v, np.ndarray) and v.ndim and v.shape[0] == B else v) for k, v in case.items()}
    pr = VR.call(VR.reference, pad)
    g = [a.astype(np.float64).copy() for a in got['grads']]
    g[11] += pr['grads'][11] / B
    _rejected(dict(got, grads=g), ref, "a padding row in x_decoded_mean/bias")


def test_planted_fault_bce_gradient_outside_the_clip():
    case = VR.edge_case()
    ref = VR.call(VR.reference, case)
    _rejected(VR.call(VR.evaluate32, case, faults=('bce_grad_outside_clip',)), ref, "BCE gradient not zeroed outside the clip")


def test_planted_fault_predict_next_scored_against_x():
    case = _base(target=True)
    ref = VR.call(VR.reference, case)
    _rejected(VR.call(VR.evaluate32, case, faults=('score_against_x',)), ref, "predict-next scored against x")


def test_planted_fault_relu_mask_dropped():
    case = _base()
    ref = VR.call(VR.reference, case)
    _rejected(VR.call(VR.evaluate32, case, faults=('drop_relu_mask_dh',)), ref, "decoder_h relu mask dropped")


@pytest.mark.parametrize("shape", [BASE, (21, 88, 88, 88, 2, 4, True)])
def test_planted_fault_each_mode_tells_the_other_apart(shape):
    case = VR.make_case(21, *shape, target=True)
    _rejected(VR.call(VR.evaluate32, case, bf16_mode=True), VR.call(VR.reference, case), "a bf16 result in fp32 mode")
    _rejected(VR.call(VR.evaluate32, case), VR.call(VR.reference, case, bf16_mode=True), "an fp32 result in bf16 mode")
