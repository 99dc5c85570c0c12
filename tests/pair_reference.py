"""fp64 reference of the cl_vrnn pair pass (include/clvae.h: clv_lstm_pair_fwd / clv_lstm_pair_bwd and the label rider).

Written from the header's contract, not from the kernels' structure, out of oracle/clvae_oracle.py pieces:

  forward   both LSTMs (O.lstm_forward on the given input projections), the fused latent head zargs = hs_enc . Wz + bz,
            z = mean + exp(log_var / 2) eps, klterm = L * KL_l, and the backward coefficients in the kernels' own layouts:
            gates [B,T,4H] gate-major (ki, kf, kg, ko) = (g i', c_{t-1} f', i g', tanh(c) o'),
            aux   [B*T,2,H] = (kcarry, kc) = (f, o (1 - tanh(c)^2)).
  backward  (a) oracle BPTT from the oracle's pre-activations (O.lstm_backward), end to end;
            (b) coefficient-driven BPTT from GIVEN coefficients (the kernel's own forward records):
                dc += dh kc; dz = (dc ki, dc kf, dc kg, dh ko); dc *= kcarry; dh_{t-1} += dz . U^T
            With (b) no element depends on which side of a hard-sigmoid kink an fp32 pre-activation landed.
            Outputs: dz of both LSTMs, dzsum_*, dzargs = [dZ + kl mean | dZ eps sd / 2 - kl (1 - sd^2) / 2], dWz, dbz.
  label     the label path's backward from dzsum_* (clv_vrnn_label_bwd): dwargs, dhW, dKa, dba.

assert_close_sliced compares per slice (time step, gate block, latent column, batch row) against the slice's own scale,
so that a wrong slice of small entries is not hidden under a tensor's largest ones.
"""
import numpy as np

from oracle import clvae_oracle as O

H = 88
G4 = 4 * H
KINK = 2.5          # hard_sigmoid(z) = clip(0.2 z + 0.5, 0, 1) has its kinks at z = +-2.5
# the per-slice bounds of tests/test_gpu_pair.py (tests/test_pair_reference.py shows that every planted fault exceeds them):
# max |got - ref| over a slice <= SLICE_ATOL * max |ref| over the whole tensor + SLICE_RTOL * max |ref| over the slice
SLICE_RTOL = 1e-4
SLICE_ATOL = 1e-6


def _act(gate_act):
    if gate_act == 'hard_sigmoid':
        return O.hard_sigmoid, O.hard_sigmoid_grad
    return O.sigmoid, (lambda z: O.sigmoid(z) * (1 - O.sigmoid(z)))


def coefficients(cache, gate_act):
    """(gates [B,T,4H] = (ki, kf, kg, ko) gate-major, aux [B*T,2,H] = (kcarry, kc)) of one O.lstm_forward cache"""
    Zp, Cs = cache['Z'], cache['C']
    B, T, _ = Zp.shape
    fa, da = _act(gate_act)
    zi, zf, zg, zo = (Zp[:, :, k * H:(k + 1) * H] for k in range(4))
    i, f, g, o = fa(zi), fa(zf), np.tanh(zg), fa(zo)
    cprev = np.concatenate([np.zeros((B, 1, H)), Cs[:, :-1]], 1)
    tc = np.tanh(Cs)
    gates = np.concatenate([g * da(zi), cprev * da(zf), i * (1 - g * g), tc * da(zo)], axis=-1)
    aux = np.stack([f, o * (1 - tc * tc)], axis=2).reshape(B * T, 2, H)
    return gates, aux


def latent_forward(hs_enc, Wz, bz, eps):
    """zargs [B,T,2L], Z [B,T,L], klterm [B,T,L] = L * KL_l"""
    L = eps.shape[-1]
    zargs = hs_enc @ Wz + bz
    m, lv = zargs[..., :L], zargs[..., L:]
    sd = np.exp(0.5 * lv)
    return zargs, m + sd * eps, -0.5 * L * (1 + lv - m * m - sd * sd)


def latent_backward(dZ, zargs, eps, kl_scale):
    """dzargs = [dZ + kl mean | dZ eps sd / 2 - kl (1 - sd^2) / 2]  (clvae.h, clv_lstm_pair_bwd)"""
    L = eps.shape[-1]
    m, lv = zargs[..., :L], zargs[..., L:]
    sd = np.exp(0.5 * lv)
    return np.concatenate([dZ + kl_scale * m, dZ * eps * 0.5 * sd - 0.5 * kl_scale * (1 - sd * sd)], axis=-1)


def pair_forward(xproj_enc, xproj_dec, rb_enc, rb_dec, U_enc, U_dec, Kz, Wz, bz, eps, gate_act='hard_sigmoid'):
    """xproj_enc [B,T,4H] = x_t . K_x; xproj_dec [B,T,4H] = x_{t-1} . K_x or None; rb_* [B,4H]; Kz [L,4H]; Wz [H,2L];
    bz [2L]; eps [B,T,L].  Zero initial states."""
    B, T, _ = xproj_enc.shape
    eye, zero = np.eye(G4), np.zeros(G4)
    xs_e = xproj_enc + rb_enc[:, None, :]
    hs_e, ce = O.lstm_forward(xs_e, eye, U_enc, zero, gate_act=gate_act)
    zargs, Z, klterm = latent_forward(hs_e, Wz, bz, eps)
    xs_d = rb_dec[:, None, :] + Z @ Kz
    if xproj_dec is not None:
        xs_d = xs_d + xproj_dec
    hs_d, cd = O.lstm_forward(xs_d, eye, U_dec, zero, gate_act=gate_act)
    gates_e, aux_e = coefficients(ce, gate_act)
    gates_d, aux_d = coefficients(cd, gate_act)
    return dict(hs_enc=hs_e, hs_dec=hs_d, gates_enc=gates_e, aux_enc=aux_e, gates_dec=gates_d, aux_dec=aux_d,
                zargs=zargs, Z=Z, klterm=klterm, pre_enc=ce['Z'], pre_dec=cd['Z'], cache_enc=ce, cache_dec=cd,
                gate_act=gate_act)


def bptt_from_coefficients(gates, aux, U, dhs):
    """(b): dz [B,T,4H] from the given coefficients gates [B,T,4H], aux [B*T,2,H] and dL/dh [B,T,H]"""
    B, T, _ = dhs.shape
    ax = aux.reshape(B, T, 2, H)
    dz = np.empty((B, T, G4))
    dc = np.zeros((B, H))
    dhrec = np.zeros((B, H))
    for t in range(T - 1, -1, -1):
        k = gates[:, t]
        dh = dhs[:, t] + dhrec
        dc = dc + dh * ax[:, t, 1]
        dz[:, t] = np.concatenate([dc * k[:, :H], dc * k[:, H:2 * H], dc * k[:, 2 * H:3 * H], dh * k[:, 3 * H:]], -1)
        dc = dc * ax[:, t, 0]
        dhrec = dz[:, t] @ U.T
    return dz


def _pair_backward(bptt_dec, bptt_enc, dhs_dec, zargs, eps, hs_enc, Kz, Wz, kl_scale):
    dz_d = bptt_dec(dhs_dec)
    dZ = dz_d @ Kz.T
    dzargs = latent_backward(dZ, zargs, eps, kl_scale)
    dz_e = bptt_enc(dzargs @ Wz.T)
    L2 = dzargs.shape[-1]
    return dict(dz_dec=dz_d, dz_enc=dz_e, dzsum_dec=dz_d.sum(1), dzsum_enc=dz_e.sum(1), dZ=dZ, dzargs=dzargs,
                dWz=hs_enc.reshape(-1, H).T @ dzargs.reshape(-1, L2), dbz=dzargs.reshape(-1, L2).sum(0))


def pair_backward_oracle(fwd, dhs_dec, U_enc, U_dec, Kz, Wz, eps, kl_scale):
    """(a): oracle BPTT end to end from the reference forward's own pre-activations"""
    eye = np.eye(G4)
    return _pair_backward(lambda d: O.lstm_backward(d, fwd['cache_dec'], eye, U_dec)[4],
                          lambda d: O.lstm_backward(d, fwd['cache_enc'], eye, U_enc)[4],
                          dhs_dec, fwd['zargs'], eps, fwd['hs_enc'], Kz, Wz, kl_scale)


def pair_backward_coef(gates_enc, aux_enc, gates_dec, aux_dec, zargs, hs_enc, dhs_dec, U_enc, U_dec, Kz, Wz, eps, kl_scale):
    """(b): the whole backward pass from given forward records (coefficients, zargs, hs_enc)"""
    return _pair_backward(lambda d: bptt_from_coefficients(gates_dec, aux_dec, U_dec, d),
                          lambda d: bptt_from_coefficients(gates_enc, aux_enc, U_enc, d),
                          dhs_dec, zargs, eps, hs_enc, Kz, Wz, kl_scale)


def label_backward(dzsum_enc, dzsum_dec, Kenc_w, Kdec_w, wargs, eps_w, onehot, W, hW, Ka, prior, class_weight, w_kl_weight,
                   inv_b):
    """the label path's backward of clv_vrnn_label_bwd (cl_vrnn/model.py:174-191, 244-252): Kenc_w / Kdec_w [C,4H] are the
    kernel rows that multiply W.  Returns dwargs [B,2(C-1)], dhW [B,D], dKa [D,2(C-1)], dba [2(C-1)]."""
    C1 = W.shape[1] - 1
    dW = dzsum_enc @ Kenc_w.T + dzsum_dec @ Kdec_w.T
    dW = dW + class_weight * inv_b * O.cce_keras(W, onehot, C1)[1]
    wm, wlv = wargs[:, :C1], wargs[:, C1:]
    ds, dlv = O.logistic_normal_bwd(W, dW, wlv, eps_w)
    _, dm_kl, dlv_kl = O.kl_w_prior(wm, wlv, prior)
    dwargs = np.concatenate([ds + w_kl_weight * inv_b * dm_kl, dlv + w_kl_weight * inv_b * dlv_kl], -1)
    return dict(dwargs=dwargs, dhW=(dwargs @ Ka.T) * (hW > 0), dKa=hW.T @ dwargs, dba=dwargs.sum(0))


def kink_mask(pre, gate_act, delta):
    """[B,T,4H] True where a coefficient depends on a hard-sigmoid derivative whose fp64 pre-activation lies within delta of
    a kink (gate blocks i, f, o; the g block is smooth).  All False for sigmoid gates."""
    m = np.zeros(pre.shape, bool)
    if gate_act == 'hard_sigmoid':
        near = np.abs(np.abs(pre) - KINK) < delta
        for k in (0, 1, 3):
            m[..., k * H:(k + 1) * H] = near[..., k * H:(k + 1) * H]
    return m


def saturated_fraction(pre):
    """fraction of the hard-sigmoid gates' (i, f, o) pre-activations beyond the kinks: the zero-derivative branch"""
    sig = np.concatenate([pre[..., :2 * H], pre[..., 3 * H:]], -1)
    return float((np.abs(sig) > KINK).mean())


def assert_close_sliced(got, ref, axes, atol, rtol, exclude=None, name=''):
    """Every slice of got along each axis in `axes` (one index of that axis, all others) must satisfy
        max |got - ref| <= atol + rtol * max |ref|        over that slice only
    so a wrong time step, gate block, latent column or batch row is judged against its own scale.  Non-finite values in
    got fail.  exclude: a boolean mask of elements left out (hard-sigmoid kinks, see kink_mask).  Returns the number of
    excluded elements (for the caller to report)."""
    got = np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: %d non-finite values" % (name, int((~np.isfinite(got)).sum()))
    err = np.abs(got - ref)
    mag = np.abs(ref)
    nex = 0
    if exclude is not None:
        exclude = np.broadcast_to(exclude, got.shape)
        nex = int(exclude.sum())
        err = np.where(exclude, 0.0, err)
        mag = np.where(exclude, 0.0, mag)
    for ax in axes:
        e = err.max(axis=tuple(a for a in range(err.ndim) if a != ax)) if err.ndim > 1 else err
        s = mag.max(axis=tuple(a for a in range(mag.ndim) if a != ax)) if mag.ndim > 1 else mag
        bad = np.flatnonzero(e > atol + rtol * s)
        if bad.size:
            j = int(bad[0])
            raise AssertionError("%s: %d slice(s) along axis %d off, first index %d: max err %.3e, slice scale %.3e "
                                 "(atol %.1e, rtol %.1e)" % (name, bad.size, ax, j, e[j], s[j], atol, rtol))
    return nex
