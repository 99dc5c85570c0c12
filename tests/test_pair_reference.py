"""CPU: tests/pair_reference.py, the fp64 reference of the pair kernels, against the oracle's whole cl_vrnn step -- and the
sensitivity of its per-slice comparison, so that tests/test_gpu_pair.py is known to catch subtle faults without a GPU."""
import numpy as np
import pytest

from oracle import clvae_oracle as O
import pair_reference as PR

H, G4 = PR.H, PR.G4


def _step(B, T, L, Cn, use_x_prev, gate, seed):
    """the oracle's cl_vrnn step and the pair reference composed with the label path and the output head, same inputs"""
    cfg = O.vrnn_config(latent_dim=L, seq_length=T, n_classes=Cn, use_x_prev=use_x_prev, class_weight=0.8, kl_weight=0.6,
                        w_kl_weight=0.9, w_log_var_prior=0.2, gate_act=gate)
    rng = np.random.default_rng(seed)
    p = O.vrnn_init_params(cfg, seed=seed)
    D = cfg['D']
    win = (rng.random((B, T + 1, D)) < 0.1).astype(np.float64)
    X, Xp = win[:, 1:], win[:, :-1]
    wt = np.eye(Cn)[rng.integers(0, Cn, B)]
    eW, eZ = rng.standard_normal((B, Cn - 1)), rng.standard_normal((B, T, L))
    ref = O.vrnn_loss_and_grads(p, cfg, X, Xp, wt, eW, eZ)
    c = ref['cache']
    off = D if use_x_prev else 0
    Ke, Kd = p['encoder_h/kernel'], p['decoder_h/kernel']
    Wz = np.concatenate([p['Z_mean/kernel'], p['Z_log_var/kernel']], 1)
    bz = np.concatenate([p['Z_mean/bias'], p['Z_log_var/bias']])
    rb_e = c['W'] @ Ke[D:] + p['encoder_h/bias']
    rb_d = c['W'] @ Kd[off + L:] + p['decoder_h/bias']
    Kz = Kd[off:off + L]
    Ue, Ud = p['encoder_h/recurrent_kernel'], p['decoder_h/recurrent_kernel']
    fwd = PR.pair_forward(X @ Ke[:D], Xp @ Kd[:D] if use_x_prev else None, rb_e, rb_d, Ue, Ud, Kz, Wz, bz, eZ, gate)
    # the output head's dL/dh_dec (what clv_out_head_train hands the pair backward)
    inv_bt = 1.0 / (B * T)
    logits = fwd['hs_dec'] @ p['X_decoded_mean/kernel'] + p['X_decoded_mean/bias']
    _, dlogits = O.bce_from_logits_keras(logits, X)
    dhs = (dlogits * inv_bt) @ p['X_decoded_mean/kernel'].T
    kl = cfg['kl_weight'] * inv_bt
    bwd = PR.pair_backward_oracle(fwd, dhs, Ue, Ud, Kz, Wz, eZ, kl)
    lab = PR.label_backward(bwd['dzsum_enc'], bwd['dzsum_dec'], Ke[D:], Kd[off + L:], c['Wargs'], eW, wt, c['W'], c['hW'],
                            p['Wargs/kernel'], cfg['w_log_var_prior'], cfg['class_weight'], cfg['w_kl_weight'], 1.0 / B)
    return dict(ref=ref, fwd=fwd, bwd=bwd, lab=lab, Ue=Ue, Ud=Ud, Kz=Kz, Wz=Wz, eZ=eZ, dhs=dhs, kl=kl, B=B, T=T, L=L)


CASES = [(3, 5, 2, 4, True, 'hard_sigmoid', 1), (2, 4, 5, 3, False, 'sigmoid', 2)]


@pytest.fixture(scope="module", params=CASES, ids=["x_prev", "no_x_prev"])
def step(request):
    return _step(*request.param)


def _h_prev(hs):
    return np.concatenate([np.zeros_like(hs[:, :1]), hs[:, :-1]], 1).reshape(-1, H)


def test_pair_reference_reproduces_the_oracle_step(step):
    """states, KL term and every gradient the pair pass (with the label rider) produces, to 1e-10 of the oracle"""
    ref, fwd, bwd, lab = step['ref'], step['fwd'], step['bwd'], step['lab']
    c, g, B, T, L = ref['cache'], ref['grads'], step['B'], step['T'], step['L']
    tol = dict(rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(fwd['hs_enc'], c['enc_h'], **tol)
    np.testing.assert_allclose(fwd['hs_dec'], c['dec_h'], **tol)
    np.testing.assert_allclose(fwd['klterm'].mean(), ref['kl_z'], **tol)
    np.testing.assert_allclose(fwd['zargs'], np.concatenate([c['Z_mean'], c['Z_log_var']], -1), **tol)
    for chain, name in (('enc', 'encoder_h'), ('dec', 'decoder_h')):
        dz = bwd['dz_' + chain].reshape(B * T, G4)
        np.testing.assert_allclose(bwd['dzsum_' + chain].sum(0), g[name + '/bias'], **tol)
        hs = fwd['hs_' + chain]
        np.testing.assert_allclose(_h_prev(hs).T @ dz, g[name + '/recurrent_kernel'], **tol)
    np.testing.assert_allclose(bwd['dWz'], np.concatenate([g['Z_mean/kernel'], g['Z_log_var/kernel']], 1), **tol)
    np.testing.assert_allclose(bwd['dbz'], np.concatenate([g['Z_mean/bias'], g['Z_log_var/bias']]), **tol)
    np.testing.assert_allclose(lab['dKa'], g['Wargs/kernel'], **tol)
    np.testing.assert_allclose(lab['dba'], g['Wargs/bias'], **tol)


def test_coefficient_bptt_is_the_oracle_bptt(step):
    """(b) fed the reference's own coefficients is (a): the backward check on the kernel's records rests on this"""
    fwd, bwd = step['fwd'], step['bwd']
    b2 = PR.pair_backward_coef(fwd['gates_enc'], fwd['aux_enc'], fwd['gates_dec'], fwd['aux_dec'], fwd['zargs'], fwd['hs_enc'],
                               step['dhs'], step['Ue'], step['Ud'], step['Kz'], step['Wz'], step['eZ'], step['kl'])
    for k in ('dz_dec', 'dz_enc', 'dzsum_dec', 'dzsum_enc', 'dzargs', 'dWz', 'dbz'):
        np.testing.assert_allclose(b2[k], bwd[k], rtol=1e-10, atol=1e-14, err_msg=k)


def _swap_last_two(a, row):
    a = a.copy()
    a[row, [-1, -2]] = a[row, [-2, -1]]
    return a


def _faults(step):
    fwd, bwd, B, T, L = step['fwd'], step['bwd'], step['B'], step['T'], step['L']
    dzargs_col = bwd['dzargs'].copy()
    dzargs_col[..., L - 1] *= 1 + 1e-3
    nokl = PR.latent_backward(bwd['dZ'], fwd['zargs'], step['eZ'], 0.0)
    slab = fwd['hs_enc'][B - 1].T @ bwd['dzargs'][B - 1]
    dz0 = bwd['dz_dec'].copy()
    dz0[:, 0, 2 * H:3 * H] = 0.0
    shifted = fwd['hs_dec'].copy()
    shifted[:, 1:] = fwd['hs_dec'][:, :-1]
    return [
        ("last two steps of one row swapped", fwd['hs_enc'], _swap_last_two(fwd['hs_enc'], B - 1), (0, 1)),
        ("decoder shifted by one step", fwd['hs_dec'], shifted, (1,)),
        ("one latent column of dzargs scaled by 1 + 1e-3", bwd['dzargs'], dzargs_col, (2,)),
        ("KL part of dzargs dropped", bwd['dzargs'], nokl, (0, 1, 2)),
        ("row B-1's slab missing from dWz", bwd['dWz'], bwd['dWz'] - slab, (1,)),
        ("step 0 missing from dzsum", bwd['dzsum_dec'], bwd['dzsum_dec'] - bwd['dz_dec'][:, 0], (0,)),
        ("one gate block of dz at t = 0 zeroed", bwd['dz_dec'].reshape(B, T, 4, H), dz0.reshape(B, T, 4, H), (1, 2)),
    ]


@pytest.mark.parametrize("k", range(7))
def test_sliced_comparison_rejects_subtle_faults(step, k):
    name, ref, bad, axes = _faults(step)[k]
    assert not np.array_equal(ref, bad), name
    tol = dict(atol=PR.SLICE_ATOL * np.abs(ref).max(), rtol=PR.SLICE_RTOL, name=name)     # the GPU test's bounds
    PR.assert_close_sliced(ref * (1 + 1e-5), ref, axes, **tol)          # an fp32-sized error passes ...
    with pytest.raises(AssertionError):                                 # ... the fault does not
        PR.assert_close_sliced(bad, ref, axes, **tol)


def test_sliced_comparison_reports_kink_exclusions():
    pre = np.tile([2.5 + 1e-8, 0.3, -2.5 - 1e-9, 1.0], G4 // 4).reshape(1, 1, G4)
    m = PR.kink_mask(pre, 'hard_sigmoid', 1e-6)
    assert m[..., 2 * H:3 * H].sum() == 0 and m.sum() > 0
    got = np.where(m, 5.0, 1.0)
    assert PR.assert_close_sliced(got, np.ones_like(got), (2,), 0.0, 1e-6, exclude=m) == int(m.sum())
    with pytest.raises(AssertionError):
        PR.assert_close_sliced(got, np.ones_like(got), (2,), 0.0, 1e-6)
    assert not PR.kink_mask(pre, 'sigmoid', 1e-6).any()
