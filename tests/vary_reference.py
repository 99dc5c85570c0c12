"""numpy reference of RE-DECODING (TEST ORACLE): the frame loops of cl_vrnn and cl_vae with the encoder
teacher-forced on the source and the decoder fed separately, under two labels:

    enc step on [sources[t], w_enc] -> zm, zlv          z = zm + exp(zlv / 2) * (float32(Tz) * eps)
    xp = x0 if t == 0 else (Xs[t-1] if history == 'own' else sources[t-1])
    dec step on [xp, z, w_dec] -> a                     x_hat = sigmoid(a * float32(1 / T))
    x = [u <= x_hat], then the clamp; Xs[t] = x

eps, u: the Philox draws of oracle/philox.py (stream 0 / 1, step = frame, S = 0), in float64 or, for the flip-cap condition
of the GPU test, in float32.  The comparator, window and flip cap are those of tests/temper_reference.py; so are the
sigmoid's clip and the hard-sigmoid.  Also the exact enumeration of the re-decoded frames on the two keyed enumerable models
of tests/test_gpu_smc_key.py (z rows zero, only notes 0 and 1 feed back, decoder rows of w for three classes)."""
import itertools

import numpy as np

from oracle import philox as OP
from temper_reference import FLIP_CAP, FREE, Follow, _apply, _hard_sigmoid, _sigmoid, factors, roll, window  # noqa: F401

D, H = 88, 88
T4 = 4


def _gate(name):
    return _hard_sigmoid if name == 'hard_sigmoid' else (lambda z: z.dtype.type(1) / (z.dtype.type(1) + np.exp(-z)))


def _cell(x, h, c, k, r, b, gate):
    zz = x @ k + b + h @ r
    i, f_, g, o = gate(zz[:, :H]), gate(zz[:, H:2 * H]), np.tanh(zz[:, 2 * H:3 * H]), gate(zz[:, 3 * H:])
    c = f_ * c + i * g
    return o * np.tanh(c), c


def noise(N, L, seed, t, dtype=np.float64):
    eps = OP.normal(N * L, seed, step=t, stream_id=0).reshape(N, L).astype(dtype)
    u = OP.uniform(N * D, seed, step=t, stream_id=1).reshape(N, D).astype(dtype)
    return eps, u


class VrnnVary:
    """one cl_vrnn re-decoding frame at a time: step(t, x_src, xp) -> tempered x_hat [N, D]; .logit is its argument,
    .zargs = (zm, zlv), .u the frame's uniforms"""

    def __init__(self, p, w_enc, w_dec, seed, L, T=1.0, Tz=1.0, dtype=np.float64, gate='hard_sigmoid'):
        self.p = {k: np.asarray(v, np.float32).astype(dtype) for k, v in p.items()}
        self.w_enc, self.w_dec = np.asarray(w_enc, dtype), np.asarray(w_dec, dtype)
        self.seed, self.L, self.dtype, self.gate = seed, L, dtype, _gate(gate)
        inv_T, tz = factors(T, Tz)
        self.inv_T, self.Tz = dtype(inv_T), dtype(tz)
        N = self.w_enc.shape[0]
        self.he, self.ce, self.hd, self.cd = (np.zeros((N, H), dtype) for _ in range(4))
        self.use_x_prev = self.p['decoder_h/kernel'].shape[0] == D + L + self.w_dec.shape[1]

    def step(self, t, x_src, xp):
        p, N = self.p, self.w_enc.shape[0]
        x_src, xp = np.asarray(x_src, self.dtype), np.asarray(xp, self.dtype)
        self.he, self.ce = _cell(np.concatenate([x_src, self.w_enc], 1), self.he, self.ce, p['encoder_h/kernel'],
                                 p['encoder_h/recurrent_kernel'], p['encoder_h/bias'], self.gate)
        zm = self.he @ p['Z_mean/kernel'] + p['Z_mean/bias']
        zlv = self.he @ p['Z_log_var/kernel'] + p['Z_log_var/bias']
        self.zargs = (zm, zlv)
        eps, self.u = noise(N, self.L, self.seed, t, self.dtype)
        z = zm + np.exp(zlv / 2) * (self.Tz * eps)
        xin = np.concatenate([xp, z, self.w_dec], 1) if self.use_x_prev else np.concatenate([z, self.w_dec], 1)
        self.hd, self.cd = _cell(xin, self.hd, self.cd, p['decoder_h/kernel'], p['decoder_h/recurrent_kernel'],
                                 p['decoder_h/bias'], self.gate)
        self.logit = (self.hd @ p['X_decoded_mean/kernel'] + p['X_decoded_mean/bias']) * self.inv_T
        return _sigmoid(self.logit)


class VaeVary:
    """one cl_vae re-decoding frame at a time: the decoder's history xp is the frame directly before t, as in training"""

    def __init__(self, p, w_enc, w_dec, seed, L, T=1.0, Tz=1.0, dtype=np.float64, gate=None):
        self.p = {k: np.asarray(v, np.float32).astype(dtype) for k, v in p.items()}
        self.w_enc, self.w_dec = np.asarray(w_enc, dtype), np.asarray(w_dec, dtype)
        self.seed, self.L, self.dtype = seed, L, dtype
        inv_T, tz = factors(T, Tz)
        self.inv_T, self.Tz = dtype(inv_T), dtype(tz)
        self.use_x_prev = self.p['decoder_h/kernel'].shape[0] == D + L + self.w_dec.shape[1]

    def step(self, t, x_src, xp):
        p, N = self.p, self.w_enc.shape[0]
        x_src, xp = np.asarray(x_src, self.dtype), np.asarray(xp, self.dtype)
        h = np.maximum(np.concatenate([x_src, self.w_enc], 1) @ p['h/kernel'] + p['h/bias'], 0)
        zm, zlv = h @ p['z_mean/kernel'] + p['z_mean/bias'], h @ p['z_log_var/kernel'] + p['z_log_var/bias']
        self.zargs = (zm, zlv)
        eps, self.u = noise(N, self.L, self.seed, t, self.dtype)
        z = zm + np.exp(zlv / 2) * (self.Tz * eps)
        xin = np.concatenate([self.w_dec, xp, z], 1) if self.use_x_prev else np.concatenate([self.w_dec, z], 1)
        hd = np.maximum(xin @ p['decoder_h/kernel'] + p['decoder_h/bias'], 0)
        self.logit = (hd @ p['x_decoded_mean/kernel'] + p['x_decoded_mean/bias']) * self.inv_T
        return _sigmoid(self.logit)


STEPPER = {'cl_vrnn': VrnnVary, 'cl_vae': VaeVary}


def vary(which, p, sources, w_enc, w_dec=None, x0=None, history='own', seed=0, L=2, clamp=None, T=1.0, Tz=1.0,
         dtype=np.float64, follow=None, gate='hard_sigmoid'):
    """the re-decoding loop of the definition.  Returns (Xs, x_hat, logit), each [N, T, D]: the clamped frames, the unclamped
    tempered probabilities and their arguments.  follow: a Follow whose frames replace the reference's own after the
    comparison (the reference then continues from the route's frames)."""
    assert history in ('own', 'source')
    sources = np.asarray(sources, dtype)
    N, Tn = sources.shape[:2]
    st = STEPPER[which](p, w_enc, w_enc if w_dec is None else w_dec, seed, L, T, Tz, dtype, gate)
    xp = np.zeros((N, D), dtype) if x0 is None else np.asarray(x0, dtype)
    Xs, xh, lg = [], [], []
    for t in range(Tn):
        xhat = st.step(t, sources[:, t], xp)
        x_t = (st.u <= xhat).astype(dtype)
        c = clamp[:, t] if clamp is not None else np.full((N, D), FREE, np.uint8)
        x_t = _apply(x_t, c)
        if follow is not None:
            x_t = follow.frame(t, x_t, st.u, xhat, c).astype(dtype)
        Xs.append(x_t)
        xh.append(xhat)
        lg.append(st.logit)
        xp = x_t if history == 'own' else sources[:, t]
    return np.stack(Xs, 1), np.stack(xh, 1), np.stack(lg, 1)


def logit_of(p):
    """float32 probabilities -> their logits in float64 (the GPU test compares on the logit side)"""
    p = np.asarray(p, np.float64)
    return np.log(p) - np.log1p(-p)


# ------------------------------------------------------------------------------------ the cases of the GPU tests
# Models: the initialisers' draw plus noise for livelier probabilities (as tests/temper_reference.case_params); cl_vae's
# output bias lowered to piano-roll densities.  Sources are sparse binary frames.
def case_params(which, L, C, use_x_prev=True, gate='hard_sigmoid', model_seed=9):
    from oracle import clvae_oracle as O
    rng = np.random.default_rng(model_seed)
    if which == 'cl_vrnn':
        cfg = O.vrnn_config(latent_dim=L, seq_length=8, n_classes=C, use_x_prev=use_x_prev, gate_act=gate)
        p = {k: np.asarray(v, np.float32) for k, v in O.vrnn_init_params(cfg, seed=model_seed).items()}
        for k in p:
            if not k.startswith('hW'):
                p[k] = (p[k] + 0.15 * rng.standard_normal(p[k].shape)).astype(np.float32)
        return cfg, p
    cfg = O.vae_config(latent_dim=L, n_classes=C, use_x_prev=use_x_prev)
    p = {k: np.asarray(v, np.float32) for k, v in O.vae_init_params(cfg, seed=model_seed).items()}
    for k in p:
        p[k] = (p[k] + 0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    p['x_decoded_mean/bias'] = (p['x_decoded_mean/bias'] - 2.0).astype(np.float32)
    return cfg, p


def case_inputs(N, Tn, C, data_seed=4, density=0.06):
    """(sources [N, Tn, D], x0 [N, D], w_enc [N, C] one-hot, w_dec [N, C] another one-hot)"""
    rng = np.random.default_rng(data_seed)
    frames = (rng.random((N, Tn + 1, D)) < density).astype(np.float64)
    k = rng.integers(0, C, N)
    return frames[:, 1:], frames[:, 0], np.eye(C)[k], np.eye(C)[(k + 1 + rng.integers(0, C - 1, N)) % C]


# 1. the training identity: (which, L, gate, use_x_prev); C = 10 for cl_vrnn, 4 for cl_vae
IDENTITY_CASES = [('cl_vrnn', 2, 'hard_sigmoid', True), ('cl_vrnn', 2, 'sigmoid', False), ('cl_vrnn', 19, 'hard_sigmoid', False),
                  ('cl_vrnn', 19, 'sigmoid', True), ('cl_vae', 3, None, True), ('cl_vae', 8, None, False)]
IDENTITY_N, IDENTITY_T, IDENTITY_SEED = 5, 8, 23
# fp32 probabilities resolve a logit to well under the 2e-4 tolerance only away from p = 1: half an ulp of 1.0 (3e-8) over
# 1 - p must stay below 1e-5, that is 1 - p >= 3e-3, |logit| <= 5.8; tests/test_vary_reference.py asserts it of every case
IDENTITY_MAX_LOGIT = 5.8
LOGIT_TOL = 2e-4                              # per-note decoder logits


def classes_of(which):
    return 10 if which == 'cl_vrnn' else 4


# 2. the free-running loop: (T, Tz) of the issue; the Philox seeds are INPUTS chosen so that the float32 run of the loop
# above stays within the flip cap of its float64 run (tests/test_vary_reference.py asserts it)
FREE_RUN_TEMPS = [(1.0, 1.0), (0.5, 0.5), (2.0, 0.5)]
FREE_RUN = {'cl_vrnn': dict(L=2, N=5, Tn=9, seed=31, roll_seed=3), 'cl_vae': dict(L=3, N=6, Tn=9, seed=17, roll_seed=5)}


def free_run_case(which):
    """(cfg, params, sources, x0, w_enc, w_dec, roll, L, Philox seed) of GPU test 2"""
    c = FREE_RUN[which]
    C = classes_of(which)
    cfg, p = case_params(which, c['L'], C)
    sources, x0, w_enc, w_dec = case_inputs(c['N'], c['Tn'], C)
    return cfg, p, sources, x0, w_enc, w_dec, roll(c['N'], c['Tn'], seed=c['roll_seed']), c['L'], c['seed']


def flips_f32_against_f64(which, T, Tz):
    """the Follow of the float64 loop along the float32 loop's frames, for one run of GPU test 2"""
    _, p, sources, x0, w_enc, w_dec, clamp, L, seed = free_run_case(which)
    kw = dict(x0=x0, history='own', seed=seed, L=L, clamp=clamp, T=T, Tz=Tz)
    got, _, _ = vary(which, p, sources, w_enc, w_dec, dtype=np.float32, **kw)
    fol = Follow(got, window(T))
    vary(which, p, sources, w_enc, w_dec, follow=fol, **kw)
    return fol


# ------------------------------------------------------------------------- the two keyed enumerable models, exactly
def keyed_params(which):
    """(cfg, params, the three keyed classes) of tests/test_gpu_smc_key.py's enumerable models; no device is touched"""
    import test_gpu_smc_key as TK
    if which == 'cl_vrnn':
        return TK.enumerable_vrnn_params() + (TK.KEYS_VRNN,)
    return TK.enumerable_vae_params() + (TK.KEYS_VAE,)


def histories():
    """the 4^T4 histories of notes 0 / 1 as [n, T4, 2] and as frames [n, T4, D]"""
    hs = np.array(list(itertools.product((0.0, 1.0), repeat=2 * T4))).reshape(-1, T4, 2)
    frames = np.zeros((len(hs), T4, D))
    frames[:, :, :2] = hs
    return hs, frames


def keyed_source():
    """one source piece [T4, D] with notes 0 / 1 only"""
    src = np.zeros((T4, D))
    src[:, :2] = [[1, 0], [0, 1], [1, 1], [0, 0]]
    return src


# The keyed models were built to tell keys apart through a filter's evidence; per history their classes differ little at
# T = 1 (cl_vrnn: at most 0.064 in any one history).  A note temperature of 0.5 doubles every logit and with it the keys'
# offsets, which is a use of the feature under test, not a change of the models; tests/test_vary_reference.py asserts the
# power (some history's probability differs by >= 0.1 between two classes) at this value.
KEYED_T = 0.5


def enumerate_redecoding(which, p, L, C, w_enc_class, w_dec_class, T=KEYED_T):
    """probability of each of the 4^T4 histories of the re-decoded frames (history='own', x0 = 0, note temperature T) of
    keyed_source() under encoder label w_enc_class and decoder label w_dec_class: x_hat of frame t given the history's
    frames before t comes from the reference stepper itself, fed that history as the decoder's input; notes 2..87 have
    logit -40 / T and never sound.  Returns (prob [n], histories [n, T4, 2], max p(note >= 2))."""
    hs, frames = histories()
    n = len(hs)
    src = np.repeat(keyed_source()[None], n, 0)
    st = STEPPER[which](p, np.eye(C)[np.full(n, w_enc_class)], np.eye(C)[np.full(n, w_dec_class)], 0, L, T=T)
    prob, other = np.ones(n), 0.0
    for t in range(T4):
        xp = np.zeros((n, D)) if t == 0 else frames[:, t - 1]
        xh = st.step(t, src[:, t], xp)
        prob *= np.prod(np.where(hs[:, t] == 1, xh[:, :2], 1 - xh[:, :2]), axis=1)
        other = max(other, float(xh[:, 2:].max()))
    return prob, hs, other


def history_counts(Xs):
    """relative frequency of each of the 4^T4 histories (in histories()' order) among frames Xs [N, T4, D]"""
    x = np.asarray(Xs)[:, :, :2].reshape(len(Xs), -1).astype(int)
    idx = (x * (2 ** np.arange(2 * T4 - 1, -1, -1))).sum(axis=1)
    return np.bincount(idx, minlength=4 ** T4) / len(Xs)


KEYED_ROWS = 4096                       # rows of one source per class in GPU test 5
# Philox seeds of GPU test 5: INPUTS chosen so that the reference's own sample meets the test's criterion for every key
# (tests/test_vary_reference.py asserts it; most of the 256 histories have an expected count below one)
KEYED_SEED = {'cl_vrnn': 115, 'cl_vae': 114}


def worst_cell(got, want, n):
    """the largest |got - want| over the histories in binomial standard errors sqrt(want (1 - want) / n) of the exact value"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    se = np.sqrt(want * (1 - want) / n)
    dev = np.abs(got - want)
    return float(np.max(np.where(dev == 0, 0.0, dev / np.maximum(se, 1e-300))))
