"""numpy reference of the two PERSISTENT SAMPLING KERNELS (csrc/generate.hip, csrc/vae_generate.hip; TEST ORACLE): one
stepper per family that covers every mode of the kernels -- generate (plain, clamped, tempered), vary, vary_latents,
decode and resume -- with both gates, use_x_prev both ways, z_prior, two labels, x0, history own / source / given, a given
latent path with noise_rows, and a start from (and a return of) a state at Philox step t0.

    enc step on [x_enc, w_enc] -> zm, zlv (z_prior: both 0)      z = zm + exp(zlv / 2) * (float32(Tz) * eps)     (or z_in[t])
    dec step on [x_dec, z, w_dec] -> a                            logit = a * float32(1 / T)    x_hat = sigmoid(clip(logit, +-30))
    x = [u <= x_hat], then the roll (row t - S, from step S on)

The steppers generalise temper_reference.VrnnStepper / VaeStepper (they ARE those classes with another step()): the NOISE
IS INJECTED (eps[t] [N, L] and u[t] [N, 88] as arrays), not drawn inside, so that the GPU test can pass what the device's own
clv_philox_normal / _uniform write and the oracle's 2e-5 of slack on a normal draw is in no bound; frame entries MULTIPLY
(cl_vrnn reads a frame entry by its value; cl_vae reads frames as on / off and its callers refuse anything else, so that
there the two readings agree).  Every result exists in float64 and in float32 (same operations in that dtype).

run() is the frame loop of every mode, on its own path or ALONG given samples; check() is the comparison the GPU test makes
(tests/test_gpu_generate.py), and the CPU self-test (tests/test_generate_reference.py) feeds it planted faults:

    bound_t = 4 x max |ref32_t - ref64_t|   per output tensor and per frame t of a case, the reference stepped on the inputs
                                            that the launch itself saw (seed / source frames, its own samples, a state's row)

4 is tests/test_gpu_resume.py::test_state_against_fp64's factor (the kernels sum in four k-slices and a lane tree, not in
numpy's order).  x_hat is compared on the logit side (vary_reference.logit_of of the float32 probabilities, the device's and
the float32 reference's alike, so that the rounding of a stored probability is part of the reference's own deviation) where
|logit_ref| <= 5.8, elsewhere on the probability side with |dp| <= p (1 - p) bound_t + 2^-24.  The samples are then EXACT:
[u <= x_hat_device] with the device's own uniform, then the roll.

The float32 stepper HAD TO TAKE THE KERNELS' FORMULAS to keep the factor at 4 (kernel_math, the default in float32):
common.h's fast_tanh, 1 - 2 rcp(exp2(2 x log2 e) + 1), whose accuracy near 0 is absolute, not relative, and sigmoidf_,
rcp(1 + exp(-clip(x, +-30))), which is TR._sigmoid, for the sigmoid gates too.  With numpy's tanh the reference's own float32
deviation is too small to stand for the kernel's on a frame of few elements: on an MI355X cl_vrnn's z_mean reached 1.68 and
z_log_var 1.25 times the bound (vary_latents, L = 1, N = 5: five numbers per frame), everything else stayed below 0.87.
(cl_vrnn's x_hat: 0.45 on the logit side, 0.69 on the probability side, the '-far' case.)
With the formulas the largest measured device / bound ratios (tests/test_gpu_generate.py prints them per test; 1.0 is the
bound) are MEASURED below; the float64 stepper is numpy's throughout."""
import numpy as np

from oracle import philox as OP
import temper_reference as TR
import vary_reference as VR
import latent_reference as LR  # noqa: F401  (the three earlier references stay importable from here, unchanged)

D, H = TR.D, TR.H
FREE = TR.FREE
FACTOR = 4.0
MAX_LOGIT = VR.IDENTITY_MAX_LOGIT
HALF_ULP_1 = 2.0 ** -24
# device / bound, the largest over all cases of tests/test_gpu_generate.py on an MI355X, per output kind.  x_hat's figure is
# against a bound that holds the rounding of the stored float32 probability (logit_of of both sides): over the cases' frames
# that bound is 1.6 x (median; up to 10 x on a frame with a logit near +5.8) the one of the float32 logit alone, still of
# order 1e-6
MEASURED = {'cl_vrnn': dict(xhat=0.687, z_mean=0.718, z_log_var=0.860, z=0.483, z_formula=0.216, state=0.525),
            'cl_vae': dict(xhat=0.430, z_mean=0.565, z_log_var=0.456, z=0.722, z_formula=0.597)}


# ------------------------------------------------------------------------------------------------------ the steppers
def _tanh_kernel(x):
    """common.h's fast_tanh in float32: 1 - 2 rcp(exp2(x * 2 log2 e) + 1)"""
    t = x.dtype.type
    return t(1) - t(2) * (t(1) / (np.exp2(x * t(2.885390082)) + t(1)))


def _cell(x, h, c, k, r, b, gate, tanh):
    zz = x @ k + b + h @ r
    i, f_, g, o = gate(zz[:, :H]), gate(zz[:, H:2 * H]), tanh(zz[:, 2 * H:3 * H]), gate(zz[:, 3 * H:])
    c = f_ * c + i * g
    return o * tanh(c), c


class Frame:
    """one frame's results: zm, zlv, z [N, L]; logit (after inv_T), xhat [N, 88]"""

    def __init__(self, zm, zlv, z, logit, xhat):
        self.zm, self.zlv, self.z, self.logit, self.xhat = zm, zlv, z, logit, xhat


class _Common:
    def _setup(self, w_dec, gate, kernel_math, mean_tempered):
        self.w_dec = self.w if w_dec is None else np.asarray(w_dec, self.dtype)
        if kernel_math is None:
            kernel_math = self.dtype == np.float32
        self.gate = TR._sigmoid if (kernel_math and gate == 'sigmoid') else VR._gate(gate or 'hard_sigmoid')
        self.tanh = _tanh_kernel if kernel_math else np.tanh
        self.mean_tempered = mean_tempered                  # a planted fault: Tz also applied to the mean

    def _latent(self, zm, zlv, eps, z_given):
        if z_given is not None:
            return None, None, np.asarray(z_given, self.dtype)
        if self.z_prior:
            zm, zlv = np.zeros_like(zm), np.zeros_like(zlv)
        z = (self.Tz * zm if self.mean_tempered else zm) + np.exp(zlv / 2) * (self.Tz * np.asarray(eps, self.dtype))
        return zm, zlv, z


class VrnnStepper(_Common, TR.VrnnStepper):
    """TR.VrnnStepper with the noise injected and every option of csrc/generate.hip: step(x_enc, x_dec, eps, z_given) ->
    Frame.  x_enc None: no encoder (decode).  state: [N, 5, 88] rows h_enc, c_enc, h_dec, c_dec, x or None (zeros)."""

    def __init__(self, p, w_enc, L, w_dec=None, T=1.0, Tz=1.0, dtype=np.float64, z_prior=False, gate='hard_sigmoid', state=None,
                 kernel_math=None, mean_tempered=False):
        TR.VrnnStepper.__init__(self, p, w_enc, 0, L, T, Tz, dtype, z_prior)
        self._setup(w_dec, gate, kernel_math, mean_tempered)
        if state is not None:
            self.he, self.ce, self.hd, self.cd = (np.asarray(state[:, i]).astype(dtype) for i in range(4))
        self.use_x_prev = self.p['decoder_h/kernel'].shape[0] == D + L + self.w_dec.shape[1]

    def step(self, x_enc, x_dec, eps, z_given=None):
        p, zm, zlv = self.p, None, None
        if x_enc is not None:
            x_enc = np.asarray(x_enc, self.dtype)
            self.he, self.ce = _cell(np.concatenate([x_enc, self.w], 1), self.he, self.ce, p['encoder_h/kernel'],
                                     p['encoder_h/recurrent_kernel'], p['encoder_h/bias'], self.gate, self.tanh)
            zm = self.he @ p['Z_mean/kernel'] + p['Z_mean/bias']
            zlv = self.he @ p['Z_log_var/kernel'] + p['Z_log_var/bias']
        zm, zlv, z = self._latent(zm, zlv, eps, z_given)
        xd = np.asarray(x_dec, self.dtype)
        xin = np.concatenate([xd, z, self.w_dec], 1) if self.use_x_prev else np.concatenate([z, self.w_dec], 1)
        self.hd, self.cd = _cell(xin, self.hd, self.cd, p['decoder_h/kernel'], p['decoder_h/recurrent_kernel'],
                                 p['decoder_h/bias'], self.gate, self.tanh)
        logit = (self.hd @ p['X_decoded_mean/kernel'] + p['X_decoded_mean/bias']) * self.inv_T
        return Frame(zm, zlv, z, logit, TR._sigmoid(logit))

    def state(self):
        return np.stack([self.he, self.ce, self.hd, self.cd], 1)


class VaeStepper(_Common, TR.VaeStepper):
    """TR.VaeStepper with the noise injected and every option of csrc/vae_generate.hip: step(x_enc, x_dec, eps, z_given)"""

    def __init__(self, p, w_enc, L, w_dec=None, T=1.0, Tz=1.0, dtype=np.float64, z_prior=False, gate=None, state=None,
                 kernel_math=None, mean_tempered=False):
        TR.VaeStepper.__init__(self, p, w_enc, 0, L, T, Tz, dtype, z_prior)
        self._setup(w_dec, gate, kernel_math, mean_tempered)
        self.use_x_prev = self.p['decoder_h/kernel'].shape[0] == D + L + self.w_dec.shape[1]

    def step(self, x_enc, x_dec, eps, z_given=None):
        p, zm, zlv = self.p, None, None
        if x_enc is not None:
            x_enc = np.asarray(x_enc, self.dtype)
            h = np.maximum(np.concatenate([x_enc, self.w], 1) @ p['h/kernel'] + p['h/bias'], 0)
            zm, zlv = h @ p['z_mean/kernel'] + p['z_mean/bias'], h @ p['z_log_var/kernel'] + p['z_log_var/bias']
        zm, zlv, z = self._latent(zm, zlv, eps, z_given)
        xd = np.asarray(x_dec, self.dtype)
        xin = np.concatenate([self.w_dec, xd, z], 1) if self.use_x_prev else np.concatenate([self.w_dec, z], 1)
        hd = np.maximum(xin @ p['decoder_h/kernel'] + p['decoder_h/bias'], 0)
        logit = (hd @ p['x_decoded_mean/kernel'] + p['x_decoded_mean/bias']) * self.inv_T
        return Frame(zm, zlv, z, logit, TR._sigmoid(logit))


STEPPER = {'cl_vrnn': VrnnStepper, 'cl_vae': VaeStepper}
GENERATE_MODES = ('plain', 'CL', 'TP', 'CL+TP')
MODES = GENERATE_MODES + ('vary', 'vary_latents', 'decode', 'resume')


# --------------------------------------------------------------------------------------------------------- the noise
def noise(c, normal=OP.normal, uniform=OP.uniform):
    """(eps [T, N, L] float32, u [T, N, 88] float32) of case c: Philox (seed, step t0 + t, stream 0 / 1, index n L + l /
    row(n) 88 + k), row(n) = noise_rows[n] or n.  normal / uniform: (count, seed, step=, stream_id=) -> flat float32; the
    oracle's by default, the GPU test passes the device's."""
    N, L, Tn = c['N'], c['L'], frames_of(c)
    rows = np.arange(N) if c.get('noise_rows') is None else np.asarray(c['noise_rows'])
    R = int(rows.max()) + 1
    eps = np.stack([np.asarray(normal(N * L, c['seed'], step=c['t0'] + t, stream_id=0), np.float32).reshape(N, L)
                    for t in range(Tn)])
    u = np.stack([np.asarray(uniform(R * D, c['seed'], step=c['t0'] + t, stream_id=1), np.float32).reshape(R, D)[rows]
                  for t in range(Tn)])
    return eps, u


def frames_of(c):
    return c['S'] + c['nsteps']


# ------------------------------------------------------------------------------------------------------ the frame loop
class Run:
    """run()'s results: zm, zlv, z [N, T, L] (None without an encoder: z is then the given path); logit, xhat [N, T, 88];
    samples [N, T, 88] (every step's draw after the roll, seed steps included); Xs = samples[:, S:]; state (cl_vrnn [N, 5, 88],
    cl_vae [N, 2, 88]) after the last frame"""


def _apply(x_t, row):
    return np.where(row <= 1, row.astype(x_t.dtype), x_t)


def run(c, p, eps, u, dtype=np.float64, along=None, kernel_math=None, fault=None):
    """the frame loop of case c (make_case) with weights p and the injected noise.  along [N, T, 88]: the samples some route
    produced (after the roll); the loop is then fed those instead of its own, which are still formed and returned.
    kernel_math: the kernels' tanh and sigmoid formulas instead of numpy's (None: in float32, see the module's docstring).
    fault: a planted fault of the loop itself (FAULTS; the self-test's), None otherwise."""
    which, mode, N, S, Tn, L = c['which'], c['mode'], c['N'], c['S'], frames_of(c), c['L']
    T_, Tz = c['temper'] if c['temper'] is not None else (1.0, 1.0)
    vary, decode, resume = mode in ('vary', 'vary_latents'), mode == 'decode', mode == 'resume'
    z_prior = c['z_prior'] and fault != 'z_prior_ignored'
    w_dec = c['w'] if fault == 'dec_w_enc' else c.get('w_dec')
    state_in = c.get('state_in')
    st = STEPPER[which](p, c['w'], L, w_dec, T_, Tz, dtype, z_prior, c['gate'], state_in if which == 'cl_vrnn' else None,
                        kernel_math, fault == 'mean_tempered')
    f = lambda a: None if a is None else np.asarray(a, np.float32).astype(dtype)
    if fault == 'half_as_one':
        f = lambda a: None if a is None else (np.asarray(a) != 0).astype(dtype)
    seeds, sources, x0, hist, z_in, clamp = f(c.get('seeds')), f(c.get('sources')), f(c.get('x0')), f(c.get('history')), \
        f(c.get('z_in')), c.get('clamp')
    zero = np.zeros((N, D), dtype)
    if which == 'cl_vae' and not (vary or decode):            # x_in, hist: the seed frame twice, or the state's two rows
        x_in, x_lag = (f(state_in[:, 0]), f(state_in[:, 1])) if resume else (seeds, seeds)
    else:
        x_in = f(state_in[:, 4]) if (resume and state_in is not None) else zero
    prev, recs, samples = (zero if x0 is None else x0), [], []
    for t in range(Tn):
        if vary or decode:
            x_enc = sources[:, t] if vary else None
            x_dec = prev
        elif which == 'cl_vrnn':
            x_enc = x_dec = seeds[:, t] if t < S else x_in
        else:
            x_enc, x_dec = x_in, (x_in if fault == 'no_lag' else x_lag)
        fr = st.step(x_enc, x_dec, eps[t], z_in[:, t] if decode else None)
        if fault == 'inv_T_after_sigmoid':
            fr.xhat = (TR._sigmoid(fr.logit / st.inv_T) * st.inv_T).astype(dtype)
        x_t = (np.asarray(u[t], dtype) <= fr.xhat).astype(dtype)
        j = t - S - (1 if fault == 'roll_off_by_one' else 0)
        if clamp is not None and t >= S and 0 <= j:
            x_t = _apply(x_t, clamp[:, j])
        recs.append(fr)
        samples.append(x_t)
        fed = x_t if along is None else np.asarray(along[:, t], dtype)
        if vary:
            prev = sources[:, t] if c['hist_source'] else fed
        elif decode:
            prev = hist[:, t] if hist is not None else fed
        elif which == 'cl_vrnn':
            x_stale, x_in = x_in if t >= S else seeds[:, t], fed
        else:
            x_lag, x_in = x_in, fed
    r = Run()
    stack = lambda k: None if getattr(recs[0], k) is None else np.stack([getattr(fr, k) for fr in recs], 1)
    r.zm, r.zlv, r.z, r.logit, r.xhat = (stack(k) for k in ('zm', 'zlv', 'z', 'logit', 'xhat'))
    r.samples = np.stack(samples, 1)
    r.Xs = r.samples[:, S:]
    if which == 'cl_vrnn':
        rows = st.state()
        if fault == 'state_h_c_swapped':
            rows = rows[:, [1, 0, 3, 2]]
        r.state = np.concatenate([rows, (x_stale if fault == 'state_x_stale' else x_in)[:, None]], 1)
    elif not (vary or decode):
        r.state = np.stack([x_lag if fault == 'state_x_stale' else x_in, x_lag], 1)
    else:
        r.state = None
    return r


# ------------------------------------------------------------------------------------------------------ the comparison
def outputs_of(r, c):
    """a Run as the launch's output tensors: Xs, xhat, zout [3, N, T, L] (vary_latents), state (resume), float32"""
    out = dict(Xs=r.Xs.astype(np.float32), xhat=r.xhat.astype(np.float32))
    if c['mode'] == 'vary_latents':
        out['zout'] = np.stack([r.zm, r.zlv, r.z]).astype(np.float32)
    if c['mode'] == 'resume':
        out['state'] = r.state.astype(np.float32)
    return out


def along_of(c, got, u):
    """the samples the launch fed itself, [N, T, 88]: steps before S are not returned, the bridge sample among them; they
    are [u <= x_hat] of the launch's own x_hat (no roll constrains them)"""
    S = c['S']
    early = (u[:S].transpose(1, 0, 2) <= got['xhat'][:, :S]).astype(np.float32)
    Xs = got['Xs'] if got.get('Xs') is not None else np.zeros((c['N'], 0, D), np.float32)
    return np.concatenate([early, Xs], 1)


def check(c, p, eps, u, got, kernel_math=None):
    """the GPU test's comparison of a launch's outputs `got` (float32: Xs [N, nsteps, 88] or None, xhat [N, T, 88], zout,
    state) with the reference stepped along the launch's own path.  Returns (ratio, ref_dev, wrong): ratio[kind] the largest
    deviation / bound_t over frames and elements (1.0 is the bound), ref_dev[kind] the smallest max |ref32_t - ref64_t| over
    the frames, wrong[kind] counts of entries that must be exact and are not (Xs, the state's frame rows)."""
    which, mode, N, S, Tn = c['which'], c['mode'], c['N'], c['S'], frames_of(c)
    u = np.asarray(u, np.float32)
    along = along_of(c, got, u)
    r64 = run(c, p, eps, u, np.float64, along)
    r32 = run(c, p, eps, u, np.float32, along, kernel_math)
    ratio, ref_dev, wrong = {}, {}, {}

    def per_frame(kind, dev, a32, a64):
        """dev, a32, a64 [N, T, ...]: per frame max |dev - a64| against 4 x max |a32 - a64|"""
        ax = tuple(i for i in range(a64.ndim) if i != 1)
        rd = np.abs(a32.astype(np.float64) - a64).max(axis=ax)
        dv = np.abs(np.asarray(dev, np.float64) - a64).max(axis=ax)
        ref_dev[kind] = float(rd.min())
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio[kind] = float(np.max(np.where(dv == 0, 0.0, dv / (FACTOR * rd))))
        return FACTOR * rd

    # x_hat: logit side where |logit_ref| <= 5.8, probability side elsewhere, one bound per frame.  The cases' weights keep
    # nearly every logit on the logit side; the probability side is reached by the two '-far' cases (all_cases)
    xh = np.asarray(got['xhat'], np.float32)
    l64, p64 = r64.logit, r64.xhat
    near = np.abs(l64) <= MAX_LOGIT
    with np.errstate(divide='ignore', invalid='ignore'):
        ref_err = np.where(near, np.abs(VR.logit_of(r32.xhat) - l64), np.abs(r32.logit.astype(np.float64) - l64))
        rd = ref_err.max(axis=(0, 2))
        bound = (FACTOR * rd)[None, :, None]
        on_logit = np.abs(VR.logit_of(xh) - l64) / bound
        on_prob = np.abs(xh.astype(np.float64) - p64) / (p64 * (1 - p64) * bound + HALF_ULP_1)
        rat = np.where(near, on_logit, on_prob)
        exact = np.where(near, VR.logit_of(xh), xh.astype(np.float64)) == np.where(near, l64, p64)
    rat = np.where(np.isnan(rat), np.inf, rat)
    rat[exact] = 0.0
    ratio['xhat'], ref_dev['xhat'] = float(rat.max()), float(rd.min())
    # the samples: free notes [u <= x_hat_device] with the device's own uniform, clamped notes the roll
    if c['nsteps'] > 0:
        want = (u[S:].transpose(1, 0, 2) <= xh[:, S:]).astype(np.float32)
        if c.get('clamp') is not None:
            want = _apply(want, c['clamp'])
        wrong['Xs'] = int((np.asarray(got['Xs'], np.float32) != want).sum())
    if mode == 'vary_latents':
        zo = np.asarray(got['zout'], np.float32)
        per_frame('z_mean', zo[0], r32.zm, r64.zm)
        per_frame('z_log_var', zo[1], r32.zlv, r64.zlv)
        bz = per_frame('z', zo[2], r32.z, r64.z)
        # z = fl(mean + exp(lv / 2) fl(Tz eps)) of the launch's OWN mean and log-variance
        Tz32 = np.float32(TR.factors(*c['temper'])[1]) if c['temper'] is not None else np.float32(1)
        e = (Tz32 * eps.astype(np.float32)).astype(np.float64).transpose(1, 0, 2)
        own = zo[0].astype(np.float64) + np.exp(zo[1].astype(np.float64) / 2) * e
        dv = np.abs(zo[2].astype(np.float64) - own).max(axis=(0, 2))
        with np.errstate(divide='ignore', invalid='ignore'):
            ratio['z_formula'] = float(np.max(np.where(dv == 0, 0.0, dv / bz)))
    if mode == 'resume' and got.get('state') is not None:
        stt = np.asarray(got['state'], np.float32)
        if which == 'cl_vrnn':
            per_frame('state', stt[:, None, :4], r32.state[:, None, :4], r64.state[:, None, :4])
            wrong['state_x'] = int((stt[:, 4] != along[:, -1]).sum())
        else:
            x_in, x_lag = along[:, -1], (along[:, -2] if Tn > 1 else np.asarray(c['state_in'], np.float32)[:, 0])
            wrong['state_x'] = int((stt[:, 0] != x_in).sum() + (stt[:, 1] != x_lag).sum())
    return ratio, ref_dev, wrong


# ----------------------------------------------------------------------------------------------------------- the cases
# Frames at which the kernels' two ballot masks (notes 0..63 / 64..87) and cl_vae's gather_rows (two notes at a time in the
# low mask, one at a time in the high one) can go wrong
def _frame(notes):
    x = np.zeros(D, np.float32)
    x[list(notes)] = 1.0
    return x


EDGE_FRAMES = [_frame([]), _frame(range(D)), _frame([0]), _frame([63]), _frame([64]), _frame([87])]
EDGE_FRAMES_VAE = EDGE_FRAMES + [_frame([5]), _frame([5, 40]), _frame([0, 31, 62]), _frame([1, 2, 33, 63]), _frame([70]),
                                 _frame([64, 87])]
TEMPERS = [(1.0, 1.0), (0.5, 1.5), (2.0, 0.5), (1.25, 0.0)]          # (T, Tz); the first goes through the tempered entry
ROLLS = ['random', 'free', 'fixed']
LATENTS = {'cl_vrnn': [1, 17, 2, 32, 16, 17], 'cl_vae': [1, 3, 32, 3, 1, 32]}        # cl_vrnn: narrow / wide alternate
GATES = ['hard_sigmoid', 'hard_sigmoid', 'sigmoid', 'sigmoid', 'hard_sigmoid', 'sigmoid']
CLASSES = {'cl_vrnn': [1, 10, 32], 'cl_vae': [1, 4, 32]}
SHAPES = [(5, 0), (1, 1), (5, 7)]                                    # cl_vrnn generate: (S, nsteps)
SHAPES_CL = [(1, 1), (5, 7), (2, 3)]                                 # a roll constrains at least one step
SHAPES_RESUME = [(0, 6), (5, 0), (1, 1), (5, 7), (0, 1), (0, 12)]
LENGTHS = [1, 7, 12]                                                 # cl_vae, vary, decode: T
T0S = [0, 7, None]                                                   # None: 2^32 - 1 - T, the largest the launcher accepts
CASES_PER_MODE = 6
# Weight scales: the initialisers' draw + 0.15 N(0, 1) (cl_vae 0.1, output bias - 2) as vary_reference.case_params makes
# them, the output kernel and bias then scaled so that the fully teacher-forced and fully clamped cases keep |logit| <= 5.8 at
# T = 0.5 (tests/test_generate_reference.py asserts it)
OUT_SCALE = {'cl_vrnn': 1.0, 'cl_vae': 0.45}


FAR_SCALE = 4.0        # the 'far' cases: the output layer scaled up once more, so that logits pass +-5.8 (free-running cases only)


def params(which, L, C, use_x_prev, gate, model_seed=9, out_scale=1.0):
    _, p = VR.case_params(which, L, C, use_x_prev, gate or 'hard_sigmoid', model_seed)
    p = {k: v for k, v in p.items() if not k.startswith(('hW', 'Wargs', 'h_w', 'w_mean', 'w_log_var'))}
    out = 'X_decoded_mean' if which == 'cl_vrnn' else 'x_decoded_mean'
    for k in (out + '/kernel', out + '/bias'):
        p[k] = (p[k] * (OUT_SCALE[which] * out_scale)).astype(np.float32)
    return p


def params_of(c):
    """the weights of a case"""
    return params(c['which'], c['L'], c['C'], c['use_x_prev'], c['gate'], out_scale=c.get('out_scale', 1.0))


def _labels(rng, N, C):
    """dense label rows (a softmax of N(0, 1)): every class row of the label kernels then reaches every sequence"""
    e = np.exp(rng.standard_normal((N, C)))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def _frames(rng, *shape):
    return (rng.random(shape + (D,)) < 0.06).astype(np.float32)


def _valued(x, rng):
    """entries 0.5 and 2.0 among a frame array's notes (and at notes 0 and 87 of its first frame)"""
    x = x.copy()
    first = x.reshape(-1, D)[0]
    first[0], first[87] = 0.5, 2.0
    on = np.argwhere(x == 1.0)
    for i, ix in enumerate(on[::2]):
        x[tuple(ix)] = (0.5, 2.0)[i % 2]
    return x


def make_case(which, mode, k, N=None, T_len=None):
    """case k (0 .. CASES_PER_MODE - 1) of a mode: every list above is walked at its own stride, offset by the mode, so
    that every value meets every mode.  N, T_len: the large-batch case's overrides."""
    m = MODES.index(mode)
    rng = np.random.default_rng(1000 * m + 10 * k + (which == 'cl_vae'))
    edges = EDGE_FRAMES if which == 'cl_vrnn' else EDGE_FRAMES_VAE
    E = len(edges)
    edge = lambda n: edges[(n + 2 * k + m) % E]

    def edged(a, shift):
        """every other frame of a [N, T, 88] becomes an edge frame, the kinds walked along n and t"""
        for n in range(a.shape[0]):
            for t in range((n + k) % 2, a.shape[1], 2):
                a[n, t] = edge(n + shift + t // 2)
        return a

    big = N is not None
    c = dict(which=which, mode=mode, k=k, L=LATENTS[which][k], C=CLASSES[which][(k + m) % 3], N=N or (1, 5)[(k + m) % 2],
             gate=GATES[k] if which == 'cl_vrnn' else None, use_x_prev=bool((k + m // 2) % 2), z_prior=False, seed=11 + 7 * k + m,
             t0=0, temper=None, clamp=None, S=0, hist_source=False)
    c['id'] = '%s-%s-%d' % (which, mode, k) + ('-big' if big else '')
    N, L, C = c['N'], c['L'], c['C']
    c['w'] = _labels(rng, N, C)
    gen = mode in GENERATE_MODES or mode == 'resume'
    if gen:
        c['z_prior'] = bool((k + m) % 3 == 2)
        if which == 'cl_vrnn':
            c['S'], c['nsteps'] = (SHAPES_RESUME[k] if mode == 'resume' else (SHAPES_CL if 'CL' in mode else SHAPES)[(k + m) % 3])
            if big:
                c['S'], c['nsteps'] = 1, T_len - 1
        else:
            c['nsteps'] = T_len or LENGTHS[(k + m) % 3]
    else:
        c['nsteps'] = T_len or LENGTHS[(k + m) % 3]
    S, ns = c['S'], c['nsteps']
    Tn = S + ns
    # ---- the frames that go in, an edge frame per sequence at every place the mode has
    if gen and which == 'cl_vrnn' and S > 0:
        c['seeds'] = edged(_frames(rng, N, S), 0)
    if gen and which == 'cl_vae' and mode != 'resume':
        c['seeds'] = np.stack([edge(n) if (n + k) % 2 == 0 else _frames(rng) for n in range(N)])
    if mode in ('vary', 'vary_latents'):
        c['sources'] = edged(_frames(rng, N, Tn), 0)
        c['hist_source'] = bool((k + m) % 2)
        c['w_dec'] = _labels(rng, N, C) if C > 1 else (c['w'] * np.float32(0.75))
    if mode == 'decode':
        c['z_in'] = (0.7 * rng.standard_normal((N, Tn, L))).astype(np.float32)
        c['w_dec'] = c['w']
        if k % 3 != 1:
            c['history'] = edged(_frames(rng, N, Tn), 1)
        if k % 3 != 0:                              # a map that is not the identity and repeats a row
            c['noise_rows'] = np.array([3, 0, 3, 7, 1] if N == 5 else [2], np.int32)
    if mode in ('vary', 'vary_latents', 'decode') and (k + m) % 3 != 1:
        c['x0'] = np.stack([edge(n + 2) for n in range(N)])
    if mode == 'resume':
        c['t0'] = T0S[(k + m) % 3] if T0S[(k + m) % 3] is not None else 2 ** 32 - 1 - Tn
        if which == 'cl_vae':
            c['state_in'] = np.stack([np.stack([edge(n), edge(n + 3)]) for n in range(N)])
        elif k % 3 != 2:                            # None: the zero start
            st = np.concatenate([rng.uniform(-0.95, 0.95, (N, 1, H)), rng.standard_normal((N, 1, H)),
                                 rng.uniform(-0.95, 0.95, (N, 1, H)), rng.standard_normal((N, 1, H)),
                                 np.stack([edge(n) for n in range(N)])[:, None]], 1)
            c['state_in'] = st.astype(np.float32)
    # ---- cl_vrnn reads a frame entry by its value: one case per place carries 0.5 and 2.0
    c['valued'] = which == 'cl_vrnn' and k == 4 and mode in ('plain', 'vary', 'resume')
    if c['valued']:
        for name in ('seeds', 'sources', 'x0'):
            if c.get(name) is not None:
                c[name] = _valued(c[name], rng)
        if c.get('state_in') is not None:
            c['state_in'][:, 4] = _valued(c['state_in'][:, 4], rng)
    # ---- the roll and the temperatures
    tempered = mode in ('TP', 'CL+TP') or (mode not in GENERATE_MODES and k % 2 == 1)
    if tempered:
        c['temper'] = TEMPERS[(k + m) % 4] if mode != 'decode' else (TEMPERS[(k + m) % 4][0], 1.0)
    rolled = mode in ('CL', 'CL+TP') or (mode not in GENERATE_MODES and (k + m) % 4 != 3)
    if rolled and ns > 0:
        kind = ROLLS[(k + m // 2) % 3]
        c['roll'] = kind
        r = TR.roll(N, ns, seed=50 + k) if kind == 'random' else np.full((N, ns, D), FREE, np.uint8) if kind == 'free' \
            else _frames(np.random.default_rng(60 + k), N, ns).astype(np.uint8)
        if kind != 'free':                          # a fully clamped row that is an edge frame: it is fed back
            for n in range(N):
                r[n, (n + k) % ns] = edge(n + 4).astype(np.uint8)
        c['clamp'] = np.ascontiguousarray(r)
    return c


def all_cases():
    out = []
    for which in ('cl_vrnn', 'cl_vae'):
        for mode in MODES:
            out += [make_case(which, mode, k) for k in range(CASES_PER_MODE)]
        # more workgroups than the card has CUs: the per-sequence base offsets of Xs, xhat, zout, the roll and the states
        out += [make_case(which, 'vary_latents', 1, N=260, T_len=3), make_case(which, 'resume', 3, N=260, T_len=3)]
        # livelier output weights on a free-running case: logits beyond +-5.8, where check() compares probabilities
        far = make_case(which, 'plain', 5)
        far.update(id=far['id'] + '-far', out_scale=FAR_SCALE)
        out.append(far)
    # xhat = NULL gives the same frames: launched on the first case of every (family, mode) that returns frames
    seen = set()
    for c in out:
        c['xhat_none'] = c['nsteps'] > 0 and (c['which'], c['mode']) not in seen
        if c['xhat_none']:
            seen.add((c['which'], c['mode']))
    return out


def teacher_forced(c):
    """no sample of the case's own reaches a later frame: every x_hat is a function of the inputs alone"""
    if c['mode'] in ('vary', 'vary_latents'):
        return c['hist_source'] or not c['use_x_prev'] or c.get('roll') == 'fixed'
    if c['mode'] == 'decode':
        return c.get('history') is not None or not c['use_x_prev'] or c.get('roll') == 'fixed'
    return c['nsteps'] <= (1 if c['which'] == 'cl_vae' else 0) or c.get('roll') == 'fixed'


def instance_of(c):
    """the template instance a case launches, as the docstring table of tests/test_gpu_generate.py names it"""
    tail = {'plain': '', 'CL': 'CL', 'TP': 'TP', 'CL+TP': 'CL,TP', 'vary': 'VR', 'vary_latents': 'VR,ZO', 'decode': 'VR,ZG',
            'resume': 'ST'}[c['mode']]
    if c['which'] == 'cl_vae':
        return 'vae<%s>' % tail
    return 'vrnn<%s,%s%s>' % ('hs' if c['gate'] == 'hard_sigmoid' else 's', 'wide' if c['L'] > 16 else 'narrow',
                              ',' + tail if tail else '')


# ------------------------------------------------------------------------------------------------- the planted faults
def _zero_rows(name, rows):
    def f(c, p):
        p = dict(p)
        a = p[name(c)].copy()
        a[rows(c)] = 0
        p[name(c)] = a
        return p
    return f


def _enc_kernel(c):
    return 'encoder_h/kernel' if c['which'] == 'cl_vrnn' else 'h/kernel'


def _dec_x_row(c, note):
    return note if c['which'] == 'cl_vrnn' else c['C'] + note


def _dec_z_row(c):
    xp = D if c['use_x_prev'] else 0
    return (xp + c['L'] - 1) if c['which'] == 'cl_vrnn' else (c['C'] + xp + c['L'] - 1)


def _label_rows(c, p):
    """the last class row of both label kernels"""
    p = dict(p)
    e = p[_enc_kernel(c)].copy()
    e[D + c['C'] - 1] = 0
    p[_enc_kernel(c)] = e
    d = p['decoder_h/kernel'].copy()
    d[(D if c['use_x_prev'] else 0) + c['L'] + c['C'] - 1 if c['which'] == 'cl_vrnn' else c['C'] - 1] = 0
    p['decoder_h/kernel'] = d
    return p


def _head_bias(c, p):
    p = dict(p)
    name = 'Z_log_var/bias' if c['which'] == 'cl_vrnn' else 'z_log_var/bias'
    b = p[name].copy()
    b[c['L'] - 1] = 0
    p[name] = b
    return p


def _has_note(c, note, places):
    """some frame that feeds the product in question has the note on"""
    for name in places:
        a = c.get(name)
        if name == 'state_in' and a is not None and c['which'] == 'cl_vrnn':
            a = a[:, 4]
        if a is not None and np.any(np.asarray(a).reshape(-1, D)[:, note] != 0):
            return True
    cl = c.get('clamp')
    return 'clamp' in places and cl is not None and bool(np.any(cl[..., note] == 1))


ENC_PLACES = ('seeds', 'sources', 'state_in', 'clamp')
DEC_PLACES = ('seeds', 'x0', 'history', 'state_in', 'clamp')
has_enc = lambda c: c['mode'] != 'decode' and not c['z_prior']
draws_eps = lambda c: c['mode'] != 'decode' and (c['temper'] is None or c['temper'][1] != 0.0)
# name -> (applies to a case, weights(c, p) or None, noise(eps) or None, the loop's fault or None)
FAULTS = {}
for _note in (0, 63, 64, 87):
    FAULTS['enc_row_%d' % _note] = (lambda c, n=_note: has_enc(c) and _has_note(c, n, ENC_PLACES),
                                    _zero_rows(_enc_kernel, lambda c, n=_note: n), None, None)
    FAULTS['dec_row_%d' % _note] = (lambda c, n=_note: c['use_x_prev'] and _has_note(c, n, DEC_PLACES),
                                    _zero_rows(lambda c: 'decoder_h/kernel', lambda c, n=_note: _dec_x_row(c, n)), None, None)
for _C in (1, 32):
    FAULTS['label_row_C%d' % _C] = (lambda c, C=_C: c['C'] == C, _label_rows, None, None)
for _L in (1, 16, 17, 32):
    FAULTS['latent_col_L%d' % _L] = (lambda c, L=_L: c['L'] == L and c['which'] == 'cl_vrnn',
                                     _zero_rows(lambda c: 'decoder_h/kernel', _dec_z_row), None, None)
FAULTS['latent_col_vae'] = (lambda c: c['which'] == 'cl_vae', _zero_rows(lambda c: 'decoder_h/kernel', _dec_z_row), None, None)
FAULTS.update({
    'dec_w_enc': (lambda c: c['mode'] in ('vary', 'vary_latents'), None, None, 'dec_w_enc'),
    'head_bias': (has_enc, _head_bias, None, None),
    'eps_next_step': (lambda c: draws_eps(c) and frames_of(c) > 1, None, lambda e: np.roll(e, -1, 0), None),
    'eps_transposed': (lambda c: draws_eps(c) and c['N'] > 1 and c['L'] > 1, None,
                       lambda e: np.stack([x.reshape(-1).reshape(x.shape[1], x.shape[0]).T for x in e]), None),
    'mean_tempered': (lambda c: has_enc(c) and c['temper'] is not None and c['temper'][1] != 1.0, None, None, 'mean_tempered'),
    'inv_T_after_sigmoid': (lambda c: c['temper'] is not None and c['temper'][0] != 1.0, None, None, 'inv_T_after_sigmoid'),
    'z_prior_ignored': (lambda c: c['z_prior'], None, None, 'z_prior_ignored'),
    'no_lag': (lambda c: c['which'] == 'cl_vae' and c['use_x_prev'] and c['mode'] in GENERATE_MODES + ('resume',), None, None,
               'no_lag'),
    'state_h_c_swapped': (lambda c: c['which'] == 'cl_vrnn' and c['mode'] == 'resume', None, None, 'state_h_c_swapped'),
    'state_x_stale': (lambda c: c['mode'] == 'resume', None, None, 'state_x_stale'),
    'roll_off_by_one': (lambda c: c.get('roll') in ('random', 'fixed') and c['nsteps'] > 1, None, None, 'roll_off_by_one'),
    'half_as_one': (lambda c: c['valued'], None, None, 'half_as_one'),
})


def planted(c, p, eps, u, name):
    """check() of the float32 loop with fault `name` planted, on its own path: what a kernel with that fault would return"""
    _, weights, noise_f, loop = FAULTS[name]
    bad = run(c, weights(c, p) if weights else p, noise_f(eps) if noise_f else eps, u, np.float32, fault=loop)
    return check(c, p, eps, u, outputs_of(bad, c))
