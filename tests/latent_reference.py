"""numpy reference of LATENT PATHS IN AND OUT (TEST ORACLE): the re-decoding loop of tests/vary_reference.py
cut in two.

    encode:  enc step on [sources[t], w_enc] -> zm, zlv;  z = zm + exp(zlv / 2) * (float32(Tz) * eps)          (per frame)
    decode:  xp = x0 if t == 0 else (Xs[t-1] if history == 'own' else history[t-1])
             dec step on [xp, z[t], w_dec] -> a;  x_hat = sigmoid(a * float32(1 / T))
             u = Philox(seed, step t, stream 1, index noise_rows[n] * 88 + note);  x = [u <= x_hat], then the clamp
    lerp_rows:  out[r] = alpha[r] * b[ib[r]] + (-alpha[r] * a[ia[r]] + a[ia[r]])

The encoder half IS vary_reference's stepper (its decoder half runs along and is ignored); the decoder half repeats that
stepper's decoder expressions term for term, so that decode(encode(src).z) equals vary(src) exactly in float64
(tests/test_latent_reference.py asserts it).  Comparator, window and flip cap are section 13's (tests/temper_reference.py)."""
import numpy as np

from oracle import philox as OP
import vary_reference as VR
from temper_reference import FLIP_CAP, FREE, Follow, _apply, _sigmoid, factors, roll, window  # noqa: F401

D, H = VR.D, VR.H
LATENT_TOL = 2e-4           # z_mean, z_log_var, z against float64: the bound tests/test_gpu_vary.py holds logits to
LOGIT_TOL = VR.LOGIT_TOL


def encode(which, p, sources, w_enc, seed=0, L=2, Tz=1.0, dtype=np.float64, gate='hard_sigmoid'):
    """(z, z_mean, z_log_var), each [N, T, L]: the latents of vary_reference.vary's loop (they do not depend on the decoder)"""
    sources = np.asarray(sources, dtype)
    N, Tn = sources.shape[:2]
    st = VR.STEPPER[which](p, w_enc, w_enc, seed, L, 1.0, Tz, dtype, gate)
    zs, zm, zlv = [], [], []
    for t in range(Tn):
        st.step(t, sources[:, t], np.zeros((N, D), dtype))
        m, lv = st.zargs
        eps, _ = VR.noise(N, L, seed, t, dtype)
        zs.append(m + np.exp(lv / 2) * (st.Tz * eps))       # the stepper's own expression for z
        zm.append(m)
        zlv.append(lv)
    return np.stack(zs, 1), np.stack(zm, 1), np.stack(zlv, 1)


class VrnnDecode:
    """the decoder half of vary_reference.VrnnVary, one frame at a time: step(z_t, xp) -> tempered x_hat; .logit its argument"""

    def __init__(self, p, w_dec, L, T=1.0, dtype=np.float64, gate='hard_sigmoid'):
        self.p = {k: np.asarray(v, np.float32).astype(dtype) for k, v in p.items()}
        self.w_dec, self.L, self.dtype, self.gate = np.asarray(w_dec, dtype), L, dtype, VR._gate(gate)
        self.inv_T = dtype(factors(T, 1.0)[0])
        N = self.w_dec.shape[0]
        self.hd, self.cd = np.zeros((N, H), dtype), np.zeros((N, H), dtype)
        self.use_x_prev = self.p['decoder_h/kernel'].shape[0] == D + L + self.w_dec.shape[1]

    def step(self, z, xp):
        p = self.p
        z, xp = np.asarray(z, self.dtype), np.asarray(xp, self.dtype)
        xin = np.concatenate([xp, z, self.w_dec], 1) if self.use_x_prev else np.concatenate([z, self.w_dec], 1)
        self.hd, self.cd = VR._cell(xin, self.hd, self.cd, p['decoder_h/kernel'], p['decoder_h/recurrent_kernel'],
                                    p['decoder_h/bias'], self.gate)
        self.logit = (self.hd @ p['X_decoded_mean/kernel'] + p['X_decoded_mean/bias']) * self.inv_T
        return _sigmoid(self.logit)


class VaeDecode:
    """the decoder half of vary_reference.VaeVary: the history xp is the frame directly before t"""

    def __init__(self, p, w_dec, L, T=1.0, dtype=np.float64, gate=None):
        self.p = {k: np.asarray(v, np.float32).astype(dtype) for k, v in p.items()}
        self.w_dec, self.L, self.dtype = np.asarray(w_dec, dtype), L, dtype
        self.inv_T = dtype(factors(T, 1.0)[0])
        self.use_x_prev = self.p['decoder_h/kernel'].shape[0] == D + L + self.w_dec.shape[1]

    def step(self, z, xp):
        p = self.p
        z, xp = np.asarray(z, self.dtype), np.asarray(xp, self.dtype)
        xin = np.concatenate([self.w_dec, xp, z], 1) if self.use_x_prev else np.concatenate([self.w_dec, z], 1)
        hd = np.maximum(xin @ p['decoder_h/kernel'] + p['decoder_h/bias'], 0)
        self.logit = (hd @ p['x_decoded_mean/kernel'] + p['x_decoded_mean/bias']) * self.inv_T
        return _sigmoid(self.logit)


DECODER = {'cl_vrnn': VrnnDecode, 'cl_vae': VaeDecode}


def uniforms(noise_rows, seed, t, dtype=np.float64):
    """u [N, D] of frame t: row n holds the uniforms of global row noise_rows[n]"""
    nr = np.asarray(noise_rows, np.int64)
    R = int(nr.max()) + 1
    return OP.uniform(R * D, seed, step=t, stream_id=1).reshape(R, D).astype(dtype)[nr]


def decode(which, p, z, w_dec, x0=None, history='own', seed=0, L=2, clamp=None, T=1.0, dtype=np.float64, follow=None,
           gate='hard_sigmoid', noise_rows=None):
    """the decoding loop of the definition.  Returns (Xs, x_hat, logit), each [N, T, D].  history: 'own' or an [N, T, D]
    array whose frame t-1 is the decoder's previous frame at t.  follow: as in vary_reference.vary."""
    z = np.asarray(z, dtype)
    N, Tn = z.shape[:2]
    assert z.shape[2] == L
    own = isinstance(history, str)
    assert (history == 'own') if own else np.shape(history) == (N, Tn, D)
    st = DECODER[which](p, w_dec, L, T, dtype, gate)
    nr = np.arange(N) if noise_rows is None else np.asarray(noise_rows)
    assert nr.shape == (N,) and nr.min() >= 0
    xp = np.zeros((N, D), dtype) if x0 is None else np.asarray(x0, dtype)
    Xs, xh, lg = [], [], []
    for t in range(Tn):
        xhat = st.step(z[:, t], xp)
        u = uniforms(nr, seed, t, dtype)
        x_t = (u <= xhat).astype(dtype)
        c = clamp[:, t] if clamp is not None else np.full((N, D), FREE, np.uint8)
        x_t = _apply(x_t, c)
        if follow is not None:
            x_t = follow.frame(t, x_t, u, xhat, c).astype(dtype)
        Xs.append(x_t)
        xh.append(xhat)
        lg.append(st.logit)
        xp = x_t if own else np.asarray(history, dtype)[:, t]
    return np.stack(Xs, 1), np.stack(xh, 1), np.stack(lg, 1)


def lerp_rows(a, ia, b, ib, alpha):
    """float64: out[r] = alpha[r] * b[ib[r]] + (-alpha[r] * a[ia[r]] + a[ia[r]])"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    al = np.asarray(alpha, np.float64)[:, None]
    av, bv = a[np.asarray(ia)], b[np.asarray(ib)]
    return al * bv + (-al * av + av)


def lerp_bound(a, ia, b, ib):
    """per element: 2^-23 (|a| + |b|), two roundings of half an ulp each (the inner fma's result is at most |a| in size,
    the outer's at most |a| + |b|)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return 2.0 ** -23 * (np.abs(a[np.asarray(ia)]) + np.abs(b[np.asarray(ib)]))


# ------------------------------------------------------------------------------------ the cases of the GPU tests
# the shapes of tests/test_gpu_vary.py: (which, L, gate, use_x_prev) = vary_reference.IDENTITY_CASES for the latents and the
# training identity; vary_reference.FREE_RUN's models, rolls and temperatures for the round trip and the free run
LATENT_CASES = VR.IDENTITY_CASES
LATENT_N, LATENT_T, LATENT_SEED = VR.IDENTITY_N, VR.IDENTITY_T, VR.IDENTITY_SEED

# 4. the free run on a RANDOM path (not an encoder's): standard normal latents scaled by 0.7.  The Philox seeds are INPUTS
# chosen so that the float32 run of decode() stays within the flip cap of its float64 run (test_latent_reference.py)
FREE_PATH = {'cl_vrnn': dict(L=2, N=5, Tn=9, seed=31, roll_seed=3, z_seed=8),
             'cl_vae': dict(L=3, N=6, Tn=9, seed=17, roll_seed=5, z_seed=8)}


def free_path_case(which):
    """(params, z, x0, w_dec, roll, L, Philox seed) of GPU test 4"""
    c = FREE_PATH[which]
    C = VR.classes_of(which)
    _, p = VR.case_params(which, c['L'], C)
    _, x0, _, w_dec = VR.case_inputs(c['N'], c['Tn'], C)
    z = 0.7 * np.random.default_rng(c['z_seed']).standard_normal((c['N'], c['Tn'], c['L']))
    z = z.astype(np.float32).astype(np.float64)              # the path as the device holds it
    return p, z, x0, w_dec, roll(c['N'], c['Tn'], seed=c['roll_seed']), c['L'], c['seed']


def flips_f32_against_f64(which, T):
    """the Follow of the float64 decode along the float32 decode's frames, for one run of GPU test 4"""
    p, z, x0, w_dec, clamp, L, seed = free_path_case(which)
    kw = dict(x0=x0, history='own', seed=seed, L=L, clamp=clamp, T=T)
    got, _, _ = decode(which, p, z, w_dec, dtype=np.float32, **kw)
    fol = Follow(got, window(T))
    decode(which, p, z, w_dec, follow=fol, **kw)
    return fol


def f32_latent_deviation(which, L, gate, use_x_prev):
    """max |float32 reference - float64 reference| over (z_mean, z_log_var, z) of a LATENT_CASES entry: how much of
    LATENT_TOL plain float32 arithmetic uses on the CPU"""
    C = VR.classes_of(which)
    _, p = VR.case_params(which, L, C, use_x_prev, gate or 'hard_sigmoid')
    src, _, w_enc, _ = VR.case_inputs(LATENT_N, LATENT_T, C)
    kw = dict(seed=LATENT_SEED, L=L, gate=gate)
    a = encode(which, p, src, w_enc, dtype=np.float32, **kw)
    b = encode(which, p, src, w_enc, **kw)
    return max(float(np.abs(x.astype(np.float64) - y).max()) for x, y in zip(a, b))


# 8. morph on the keyed enumerable models of vary_reference: one step, 4096 pairs, common_noise=False, so the alpha = 1 row of
# pair j is global row 2 j + 1.  Philox seeds: INPUTS chosen so that the reference's own sample meets the GPU test's
# criterion (4 binomial standard errors in every one of the 256 histories, most with an expected count below one) for every
# key; tests/test_latent_reference.py asserts it
KEYED_MORPH_SEED = {'cl_vrnn': 126, 'cl_vae': 100}


def keyed_morph_rows(which, p, L, C, w_b_class, seed):
    """the reference's frames of the alpha = 1 rows of GPU test 8 (the keyed decoders do not read z)"""
    n = VR.KEYED_ROWS
    Xs, _, _ = decode(which, p, np.zeros((n, VR.T4, L)), np.eye(C)[np.full(n, w_b_class)], seed=seed, L=L, T=VR.KEYED_T,
                      noise_rows=2 * np.arange(n) + 1)
    return Xs
