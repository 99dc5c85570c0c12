"""numpy reference of the TEMPERED samplers of DESIGN.md 13 (TEST ORACLE): the frame loops of cl_vrnn and cl_vae with

    inv_T = float32(1 / T)            a' = a * inv_T            x_hat = sigmoid(clip(a', -30, 30))
    eps'  = float32(Tz) * eps         z  = m + exp(lv / 2) * eps'          x = [u <= x_hat], then the clamp

(a: the output head's pre-activation; eps, u: the Philox draws of oracle/philox.py, stream 0 / 1, step = frame), in float64
or, for the flip-cap condition of the GPU test, in float32; and the exact enumeration of the tempered distribution on the
two enumerable models of tests/test_gpu_smc.py (z rows zero, only notes 0 and 1 feed back, 4^4 histories)."""
import itertools

import numpy as np

from oracle import philox as OP

D, H = 88, 88
FREE = 255
T4 = 4
ROLL01 = np.array([[FREE, FREE], [FREE, 1], [0, 1], [FREE, 1]], np.uint8)      # tests/test_gpu_smc.py's constraint


def factors(T, Tz):
    """(inv_T, Tz) as the float32 values every route multiplies by: 1 / T formed in double and rounded once"""
    return np.float32(1.0 / float(T)), np.float32(Tz)


def window(T):
    """how close to its probability a free draw must lie before fp32 rounding may flip it: the untempered suites' 1e-5,
    times max(1, 1 / T) because a logit difference grows by 1 / T before the sigmoid"""
    return 1e-5 * max(1.0, 1.0 / float(T))


def roll(N, nsteps, frac=0.3, on=0.3, seed=0):
    """about `frac` of the notes clamped, a fraction `on` of those forced on (tests/test_gpu_clamped_generation.py's _roll)"""
    r = np.random.default_rng(seed).random((N, nsteps, D))
    return np.where(r < frac, (r < frac * on).astype(np.uint8), np.uint8(FREE)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- dtype-preserving math
def _sigmoid(a):
    a = np.clip(a, -30.0, 30.0)                   # the routes' sigmoid clips its argument
    one = a.dtype.type(1)
    return one / (one + np.exp(-a))


def _hard_sigmoid(z):
    t = z.dtype.type
    return np.clip(t(0.2) * z + t(0.5), t(0), t(1))


def _cell(x, h, c, k, r, b):
    zz = x @ k + b + h @ r
    i, f_, g, o = _hard_sigmoid(zz[:, :H]), _hard_sigmoid(zz[:, H:2 * H]), np.tanh(zz[:, 2 * H:3 * H]), _hard_sigmoid(zz[:, 3 * H:])
    c = f_ * c + i * g
    return o * np.tanh(c), c


def _noise(N, L, seed, t, dtype):
    eps = OP.normal(N * L, seed, step=t, stream_id=0).reshape(N, L).astype(dtype)
    u = OP.uniform(N * D, seed, step=t, stream_id=1).reshape(N, D).astype(dtype)
    return eps, u


class VrnnStepper:
    """one cl_vrnn frame at a time (hard-sigmoid gates): step(t, x_prev) -> tempered x_hat [N, D] of step t"""

    def __init__(self, p, w, seed, L, T=1.0, Tz=1.0, dtype=np.float64, z_prior=False):
        self.p = {k: np.asarray(v, np.float32).astype(dtype) for k, v in p.items()}
        self.w, self.seed, self.L, self.dtype, self.z_prior = np.asarray(w, dtype), seed, L, dtype, z_prior
        inv_T, tz = factors(T, Tz)
        self.inv_T, self.Tz = dtype(inv_T), dtype(tz)
        N = self.w.shape[0]
        self.he, self.ce, self.hd, self.cd = (np.zeros((N, H), dtype) for _ in range(4))

    def step(self, t, x_prev):
        p, w, N = self.p, self.w, self.w.shape[0]
        x_prev = np.asarray(x_prev, self.dtype)
        self.he, self.ce = _cell(np.concatenate([x_prev, w], 1), self.he, self.ce, p['encoder_h/kernel'],
                                 p['encoder_h/recurrent_kernel'], p['encoder_h/bias'])
        zm = self.he @ p['Z_mean/kernel'] + p['Z_mean/bias']
        zlv = self.he @ p['Z_log_var/kernel'] + p['Z_log_var/bias']
        if self.z_prior:
            zm, zlv = np.zeros_like(zm), np.zeros_like(zlv)
        eps, self.u = _noise(N, self.L, self.seed, t, self.dtype)
        z = zm + np.exp(zlv / 2) * (self.Tz * eps)
        xin = np.concatenate([x_prev, z, w], 1) if p['decoder_h/kernel'].shape[0] == D + self.L + w.shape[1] \
            else np.concatenate([z, w], 1)
        self.hd, self.cd = _cell(xin, self.hd, self.cd, p['decoder_h/kernel'], p['decoder_h/recurrent_kernel'],
                                 p['decoder_h/bias'])
        return _sigmoid((self.hd @ p['X_decoded_mean/kernel'] + p['X_decoded_mean/bias']) * self.inv_T)


class VaeStepper:
    """one cl_vae frame at a time (use_x_prev): step(t, x_in, hist) -> tempered x_hat [N, D] of frame t"""

    def __init__(self, p, w, seed, L, T=1.0, Tz=1.0, dtype=np.float64, z_prior=False):
        self.p = {k: np.asarray(v, np.float32).astype(dtype) for k, v in p.items()}
        self.w, self.seed, self.L, self.dtype, self.z_prior = np.asarray(w, dtype), seed, L, dtype, z_prior
        inv_T, tz = factors(T, Tz)
        self.inv_T, self.Tz = dtype(inv_T), dtype(tz)

    def step(self, t, x_in, hist):
        p, w, N = self.p, self.w, self.w.shape[0]
        x_in, hist = np.asarray(x_in, self.dtype), np.asarray(hist, self.dtype)
        h = np.maximum(np.concatenate([x_in, w], 1) @ p['h/kernel'] + p['h/bias'], 0)
        zm, zlv = h @ p['z_mean/kernel'] + p['z_mean/bias'], h @ p['z_log_var/kernel'] + p['z_log_var/bias']
        if self.z_prior:
            zm, zlv = np.zeros_like(zm), np.zeros_like(zlv)
        eps, self.u = _noise(N, self.L, self.seed, t, self.dtype)
        z = zm + np.exp(zlv / 2) * (self.Tz * eps)
        hd = np.maximum(np.concatenate([w, hist, z], 1) @ p['decoder_h/kernel'] + p['decoder_h/bias'], 0)
        return _sigmoid((hd @ p['x_decoded_mean/kernel'] + p['x_decoded_mean/bias']) * self.inv_T)


def _apply(x_t, c):
    return np.where(c <= 1, c.astype(x_t.dtype), x_t)


class Follow:
    """compare a route's frames `got` with the reference's own draw, frame by frame, by the rule of the untempered suites:
    clamped notes exact; a free note may differ only where |u - x_hat| < win; the reference then continues from `got`"""

    def __init__(self, got, win):
        self.got, self.win, self.flips, self.far, self.clamp_wrong = np.asarray(got, np.float64), win, 0, 0, 0

    def frame(self, j, x_t, u, xhat, c):
        got = self.got[:, j]
        self.clamp_wrong += int((got[c <= 1] != c[c <= 1]).sum())
        diff = got != x_t
        self.far += int((diff & ~(np.abs(u.astype(np.float64) - xhat.astype(np.float64)) < self.win)).sum())
        self.flips += int(diff.sum())
        return got


def vrnn_generate(p, seeds, w, nsteps, seed, L, clamp=None, T=1.0, Tz=1.0, dtype=np.float64, follow=None, z_prior=False):
    """the frame loop of cl_vrnn on the tempered model: seeds [N, S, D] teacher-forced, then nsteps samples under the roll
    (row j constrains the sample of step S + j; the bridge stays free).  Returns (Xs [N, nsteps, D], x_hat [N, S+nsteps, D]).
    follow: a Follow whose frames replace the reference's own after the comparison."""
    N, S = seeds.shape[:2]
    st = VrnnStepper(p, w, seed, L, T, Tz, dtype, z_prior)
    x_prev, Xs, xh = np.zeros((N, D), dtype), [], []
    for t in range(S + nsteps):
        if t < S:
            x_prev = seeds[:, t]
        xhat = st.step(t, x_prev)
        xh.append(xhat)
        x_t = (st.u <= xhat).astype(dtype)
        if t >= S:
            if clamp is not None:
                x_t = _apply(x_t, clamp[:, t - S])
            if follow is not None:
                x_t = follow.frame(t - S, x_t, st.u, xhat, clamp[:, t - S] if clamp is not None else np.full((N, D), FREE)) \
                    .astype(dtype)
            Xs.append(x_t)
        x_prev = x_t
    return np.stack(Xs, 1) if Xs else np.zeros((N, 0, D), dtype), np.stack(xh, 1)


def vae_generate(p, seeds, w, nsteps, seed, L, clamp=None, T=1.0, Tz=1.0, dtype=np.float64, follow=None, z_prior=False):
    """the frame loop of cl_vae on the tempered model: seeds [N, D] is frame -1 (and the decoder's first history); row t of
    the roll constrains frame t.  Returns (Xs, x_hat), both [N, nsteps, D]."""
    N = seeds.shape[0]
    st = VaeStepper(p, w, seed, L, T, Tz, dtype, z_prior)
    x_in, hist, Xs, xh = seeds, seeds, [], []
    for t in range(nsteps):
        xhat = st.step(t, x_in, hist)
        xh.append(xhat)
        x_t = (st.u <= xhat).astype(dtype)
        if clamp is not None:
            x_t = _apply(x_t, clamp[:, t])
        if follow is not None:
            x_t = follow.frame(t, x_t, st.u, xhat, clamp[:, t] if clamp is not None else np.full((N, D), FREE)).astype(dtype)
        Xs.append(x_t)
        hist, x_in = x_in, x_t
    return np.stack(Xs, 1), np.stack(xh, 1)


def vrnn_xhat_along(p, inputs, w, seed, L, T=1.0, Tz=1.0, z_prior=False):
    """fp64 tempered x_hat of every step given each step's input frame, inputs [N, T, D]"""
    st = VrnnStepper(p, w, seed, L, T, Tz, np.float64, z_prior)
    return np.stack([st.step(t, inputs[:, t]) for t in range(inputs.shape[1])], 1)


def vae_xhat_along(p, seeds, frames, w, seed, L, T=1.0, Tz=1.0, z_prior=False):
    """fp64 tempered x_hat of every frame of cl_vae fed its own frames [N, T, D]"""
    st = VaeStepper(p, w, seed, L, T, Tz, np.float64, z_prior)
    x_in, hist, out = seeds, seeds, []
    for t in range(frames.shape[1]):
        out.append(st.step(t, x_in, hist))
        hist, x_in = x_in, frames[:, t]
    return np.stack(out, 1)


# ------------------------------------------------------------------------------- the two enumerable models, exactly
def enumerable_params(which):
    """the weights of tests/test_gpu_smc.py's _enumerable_vrnn / _enumerable_vae without a device: the helper is run with
    the engine class replaced by a recorder of set_weights"""
    import clvae_amd.engine as E
    import test_gpu_smc as TS
    name = {'cl_vrnn': 'VrnnEngine', 'cl_vae': 'VaeEngine'}[which]

    class Recorder:
        def __init__(self, *a):
            self.P = self

        def set_weights(self, p):
            self.weights = p

    real = getattr(E, name)
    setattr(E, name, Recorder)
    try:
        _, p = (TS._enumerable_vrnn if which == 'cl_vrnn' else TS._enumerable_vae)(None, 1)
    finally:
        setattr(E, name, real)
    return p


LAG = {'cl_vrnn': 1, 'cl_vae': 2}          # frames between a note and the note it steers (cl_vae's decoder history lags)


def xhat_of(which, p, T=1.0):
    """frames [n, T4, D] -> tempered x_hat of every frame given the frames before it (zero seed, label 0: neither the
    label nor z reaches the output in these models)"""
    def f(frames):
        n = frames.shape[0]
        if which == 'cl_vrnn':
            inputs = np.concatenate([np.zeros((n, 1, D)), frames[:, :-1]], 1)
            return vrnn_xhat_along(p, inputs, np.eye(10)[np.zeros(n, int)], 0, 2, T)
        return vae_xhat_along(p, np.zeros((n, D)), frames, np.eye(4)[np.zeros(n, int)], 0, 3, T)
    return f


def histories():
    """the 4^T4 histories of notes 0 / 1 as [n, T4, 2] and as frames [n, T4, D]"""
    hs = np.array(list(itertools.product((0.0, 1.0), repeat=2 * T4))).reshape(-1, T4, 2)
    frames = np.zeros((len(hs), T4, D))
    frames[:, :, :2] = hs
    return hs, frames


def exact_free(which, p, T):
    """the unconstrained tempered distribution over notes 0 / 1: (probability of every history [n], the histories
    [n, T4, 2], p(note >= 2 sounds) per draw)"""
    hs, frames = histories()
    xh = xhat_of(which, p, T)(frames)
    bern = np.where(hs == 1, xh[:, :, :2], 1 - xh[:, :, :2])
    return np.prod(bern, axis=(1, 2)), hs, float(xh[:, :, 2:].max())


def free_cells(which, p, T):
    """the statistics of GPU test 6 as a dict name -> exact probability: the frequency of notes 0 and 1 per frame, and per
    frame t >= lag the 2 x 2 tables of (note 0 at t-lag, note 1 at t) and (note 1 at t-lag, note 0 at t)"""
    pr, hs, _ = exact_free(which, p, T)
    lag, cells = LAG[which], {}
    for t in range(T4):
        for k in (0, 1):
            cells['freq', t, k] = float((pr * hs[:, t, k]).sum())
        if t >= lag:
            for a, b in ((0, 1), (1, 0)):
                for va in (0, 1):
                    for vb in (0, 1):
                        cells['pair', t, a, b, va, vb] = float((pr * (hs[:, t - lag, a] == va) * (hs[:, t, b] == vb)).sum())
    return cells


def cell_counts(which, Xs):
    """the same statistics measured on frames Xs [N, T4, D] (numpy): dict name -> relative frequency"""
    x = np.asarray(Xs)[:, :, :2]
    lag, cells = LAG[which], {}
    for t in range(T4):
        for k in (0, 1):
            cells['freq', t, k] = float(x[:, t, k].mean())
        if t >= lag:
            for a, b in ((0, 1), (1, 0)):
                for va in (0, 1):
                    for vb in (0, 1):
                        cells['pair', t, a, b, va, vb] = float(((x[:, t - lag, a] == va) & (x[:, t, b] == vb)).mean())
    return cells


def cell_se(prob, N):
    """binomial standard error from the exact value, the variance floored at 0.01 as test_gpu_smc._check_exactness does"""
    return np.sqrt(max(prob * (1 - prob), 0.01) / N)


def exact_constrained(xhat_fn):
    """test_gpu_smc._exact for any x_hat function: (p(ROLL01), exact posterior marginals, clamped-ancestral marginals
    [T4, 2])"""
    hs, frames = histories()
    xh = xhat_fn(frames)[:, :, :2]
    bern = np.where(hs == 1, xh, 1 - xh)
    clamped = ROLL01 <= 1
    consistent = np.all(~clamped[None] | (hs == ROLL01[None]), axis=(1, 2))
    joint = np.prod(bern, axis=(1, 2)) * consistent
    anc = np.prod(np.where(clamped[None], 1.0, bern), axis=(1, 2)) * consistent
    Z = joint.sum()
    return Z, (joint[:, None, None] * hs).sum(0) / Z, (anc[:, None, None] * hs).sum(0) / anc.sum()


# ------------------------------------------------------------------------- the cases of GPU test 4 (fp64 frame loops)
# (T, Tz) and the Philox seed of each run.  The seeds are INPUTS chosen so that the float32 run of the loop above stays
# within the flip cap of its float64 run (tests/test_temper_reference.py asserts it); the models, seed frames, labels and
# rolls are those of the untempered oracle tests.
VRNN_CASE = dict(T_len=8, L=2, C=10, N=5, S=3, nsteps=6, model_seed=9, data_seed=4, roll_seed=3)
VAE_CASE = dict(L=3, C=4, N=6, nsteps=7, model_seed=2, data_seed=8, roll_seed=5)
ORACLE_RUNS = [(0.5, 0.5, 31), (2.0, 0.5, 31)]           # (T, Tz, seed) for cl_vrnn
ORACLE_RUNS_VAE = [(0.5, 0.5, 17), (2.0, 0.5, 17)]
FLIP_CAP = 2


def vrnn_case_inputs():
    c = VRNN_CASE
    rng = np.random.default_rng(c['data_seed'])
    seeds = (rng.random((c['N'], c['S'], D)) < 0.06).astype(np.float64)
    w = np.eye(c['C'])[rng.integers(0, c['C'], c['N'])]
    return seeds, w, roll(c['N'], c['nsteps'], seed=c['roll_seed'])


def vae_case_inputs():
    c = VAE_CASE
    rng = np.random.default_rng(c['data_seed'])
    seeds = (rng.random((c['N'], D)) < 0.06).astype(np.float64)
    w = np.eye(c['C'])[rng.integers(0, c['C'], c['N'])]
    return seeds, w, roll(c['N'], c['nsteps'], seed=c['roll_seed'])


def case_params(which):
    """the weights of those runs, made on the host (the GPU test loads them into its model): the initialisers' draw plus
    noise for livelier probabilities, the output bias of cl_vae lowered to piano-roll densities"""
    from oracle import clvae_oracle as O
    if which == 'cl_vrnn':
        c = VRNN_CASE
        cfg = O.vrnn_config(latent_dim=c['L'], seq_length=c['T_len'], n_classes=c['C'], use_x_prev=True, gate_act='hard_sigmoid')
        p = {k: np.asarray(v, np.float32) for k, v in O.vrnn_init_params(cfg, seed=c['model_seed']).items()}
        rng = np.random.default_rng(c['model_seed'])
        for k in p:
            if not k.startswith('hW'):
                p[k] = (p[k] + 0.15 * rng.standard_normal(p[k].shape)).astype(np.float32)
        return p
    c = VAE_CASE
    cfg = O.vae_config(latent_dim=c['L'], n_classes=c['C'], use_x_prev=True)
    p = {k: np.asarray(v, np.float32) for k, v in O.vae_init_params(cfg, seed=c['model_seed']).items()}
    rng = np.random.default_rng(c['model_seed'])
    for k in p:
        p[k] = (p[k] + 0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    p['x_decoded_mean/bias'] = (p['x_decoded_mean/bias'] - 2.0).astype(np.float32)
    return p


def flips_f32_against_f64(which, T, Tz, seed):
    """the Follow of the float64 loop along the float32 loop's frames, for one run of the cases above"""
    p = case_params(which)
    if which == 'cl_vrnn':
        seeds, w, clamp = vrnn_case_inputs()
        c, gen = VRNN_CASE, vrnn_generate
    else:
        seeds, w, clamp = vae_case_inputs()
        c, gen = VAE_CASE, vae_generate
    got, _ = gen(p, seeds.astype(np.float32), w, c['nsteps'], seed, c['L'], clamp, T, Tz, dtype=np.float32)
    fol = Follow(got, window(T))
    gen(p, seeds, w, c['nsteps'], seed, c['L'], clamp, T, Tz, follow=fol)
    return fol
