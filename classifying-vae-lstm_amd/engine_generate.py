"""Sampling on the device: the frame loops of generate_sample (cl_vae/model.py:9-42, cl_vrnn/model.py:9-60) for N sequences
at once, and the stateful single-step sub-models of cl_vrnn (cl_vrnn/model.py:116-162).  Mixins of engine.VaeEngine /
engine.VrnnEngine: they use the engines' buffers, parameters and forward pieces."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from .ops import ACT_NONE, ACT_RELU, ACT_SIGMOID


def device_f32(a, device):
    """a host array or a tensor as a contiguous float32 tensor on the device"""
    if not isinstance(a, torch.Tensor):
        a = torch.as_tensor(np.ascontiguousarray(np.asarray(a), dtype=np.float32))
    return a.to(dtype=torch.float32, device=device).contiguous()


def binary_frames(**frames):
    """cl_vae reads every frame it is given as on / off: the persistent kernel (csrc/vae_generate.hip) forms a note mask and
    adds kernel rows unweighted, the frame chain multiplies by the value, so the two routes are the same sampler only on
    frames of 0 and 1.  ValueError for a frame tensor with any other entry (NaN included); None passes.  One device
    reduction per tensor, before any launch.  cl_vrnn multiplies by the value on both routes and takes any float."""
    for name, x in frames.items():
        if x is not None and bool(((x != 0) & (x != 1)).any()):
            raise ValueError("cl_vae reads frames as on/off: %s has an entry other than 0 and 1" % name)


def clamp_roll(clamp, N, nsteps, D, device):
    """A constraint roll for generate(clamp=...): uint8 [N, nsteps, D], one row per returned frame; 0 forces the note off,
    1 forces it on, any other value (harmonize.FREE = 255) leaves it free.  numpy or torch in, contiguous device tensor out;
    ValueError on a wrong shape or dtype.  A Constraints (roll and / or voice counts) in the same place: one
    without voices comes back as its roll (or None), one with voices as itself, checked and on the device (resolve)."""
    if clamp is None:
        return None
    if isinstance(clamp, Constraints):
        return clamp.resolve(N, nsteps, D, device)
    if isinstance(clamp, torch.Tensor):
        if clamp.dtype != torch.uint8:
            raise ValueError("clamp must be uint8, got %s" % clamp.dtype)
    else:
        clamp = np.asarray(clamp)
        if clamp.dtype != np.uint8:
            raise ValueError("clamp must be uint8, got %s" % clamp.dtype)
        clamp = torch.from_numpy(np.ascontiguousarray(clamp))
    if tuple(clamp.shape) != (int(N), int(nsteps), int(D)):
        raise ValueError("clamp must have shape %s, got %s" % ((int(N), int(nsteps), int(D)), tuple(clamp.shape)))
    return clamp.to(device).contiguous()


VOICES_FREE = (0, 255)          # the pair of a frame without a count
VOICES_MAX = 15                 # the largest hi: the kernel's lanes hold the counts 0 .. 15
VOICES_MAX_D = 128              # VOICES_MAX_D of csrc/voices.hip: two notes per lane


def _count_pair(lo, hi):
    for v in (lo, hi):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError("a voice count is an integer, got %r" % (v,))
    if not 0 <= lo <= hi <= VOICES_MAX:
        raise ValueError("voice counts must satisfy 0 <= lo <= hi <= %d, got (%d, %d)" % (VOICES_MAX, lo, hi))
    return int(lo), int(hi)


class Constraints:
    """What a device sampler's frames must satisfy, passed as the value of clamp=: a constraint roll (uint8
    [N, nsteps, D], clamp_roll) and / or voice counts.  voices: uint8 [N, nsteps, 2] holding (lo, hi) per returned frame --
    the frame then has lo <= sounding notes <= hi, 0 <= lo <= hi <= 15, drawn exactly from p(frame | roll row, count in
    range); the pair (0, 255) leaves a frame free -- or an int k (exactly k in every frame) or a pair (lo, hi) for every
    frame.  numpy or torch.  Row j of the counts applies where row j of the roll applies; seed steps and the bridge carry
    none.  exactly(k), between(lo, hi) and as_in(source_rolls) (every frame as many notes as the source frame has) build
    one; each takes roll= too.  Without voices a Constraints is its roll, launch for launch.  With voices the call runs on
    the frame chain (persistent=True takes the chain too: the persistent kernels do not carry the count) or in the particle
    filter, whose weight increment gains log P(count in range | forced notes).  A frame is infeasible when more notes are
    forced on than hi, or forced-on plus free notes are fewer than lo: ValueError before any launch (resolve)."""

    def __init__(self, roll=None, voices=None):
        if isinstance(voices, (int, np.integer)) and not isinstance(voices, (bool, np.bool_)):
            voices = _count_pair(voices, voices)
        elif isinstance(voices, (tuple, list)):
            if len(voices) != 2:
                raise ValueError("voices must be an int, a pair (lo, hi) or a uint8 array [N, nsteps, 2], got %r" % (voices,))
            voices = _count_pair(*voices)
        elif voices is not None and not isinstance(voices, (np.ndarray, torch.Tensor)):
            raise ValueError("voices must be an int, a pair (lo, hi) or a uint8 array [N, nsteps, 2], got %r" % (voices,))
        if isinstance(roll, Constraints):
            raise ValueError("roll must be a uint8 array, not a Constraints")
        self.roll, self.voices, self._key = roll, voices, None

    @classmethod
    def exactly(cls, k, roll=None):
        """every returned frame has exactly k sounding notes"""
        return cls(roll, _count_pair(k, k))

    @classmethod
    def between(cls, lo, hi, roll=None):
        """every returned frame has lo .. hi sounding notes"""
        return cls(roll, _count_pair(lo, hi))

    @classmethod
    def as_in(cls, source_rolls, roll=None):
        """frame (n, t) has as many sounding notes as source_rolls[n, t] ([N, nsteps, D], nonzero = sounding)"""
        src = np.asarray(source_rolls.cpu() if isinstance(source_rolls, torch.Tensor) else source_rolls)
        if src.ndim != 3:
            raise ValueError("source_rolls must be [N, nsteps, D], got shape %s" % (src.shape,))
        n = (src != 0).sum(axis=-1)
        if n.size and n.max() > VOICES_MAX:
            raise ValueError("a source frame has %d sounding notes: voice counts go up to %d" % (n.max(), VOICES_MAX))
        return cls(roll, np.ascontiguousarray(np.stack([n, n], axis=-1).astype(np.uint8)))

    def __getitem__(self, index):
        """the constraints of some sequences and frames: c[m0:m1], c[:, a:b] (the index goes to the roll and to the counts)"""
        take = lambda a: a if a is None or isinstance(a, tuple) else a[index]
        out = Constraints(take(self.roll), take(self.voices))
        if self._key is not None:           # a part of a checked whole is checked: only its shape is new
            for name in ('roll', 'voices'):
                if getattr(out, name) is not None:
                    setattr(out, name, getattr(out, name).contiguous())
            v = out.voices
            out._key = (int(v.shape[0]), int(v.shape[1]), self._key[2], self._key[3])
        return out

    def repeat_rows(self, k):
        """every sequence's constraints k times in a row (morph: the rows of a pair)"""
        rep = lambda a: a if a is None or isinstance(a, tuple) else (
            a.repeat_interleave(k, 0) if isinstance(a, torch.Tensor) else np.repeat(np.asarray(a), k, axis=0))
        return Constraints(rep(self.roll), rep(self.voices))

    def resolve(self, N, nsteps, D, device):
        """Check against a call of N sequences x nsteps returned frames x D notes and move to the device.  Returns None
        (nothing given), the roll as clamp_roll returns it (no voices), or a Constraints whose roll (or None) and voices are
        contiguous uint8 device tensors.  ValueError for a wrong shape or dtype, D > 128, a pair that is neither (0, 255)
        nor 0 <= lo <= hi <= 15, and an infeasible frame.  One device reduction, before any launch."""
        key = (int(N), int(nsteps), int(D), str(device))
        if self._key == key:
            return self
        roll = clamp_roll(self.roll, N, nsteps, D, device)
        v = self.voices
        if v is None:
            return roll
        if D > VOICES_MAX_D:
            raise ValueError("voice counts need D <= %d notes, got %d" % (VOICES_MAX_D, D))
        if isinstance(v, tuple):
            v = torch.tensor(v, dtype=torch.uint8).expand(int(N), int(nsteps), 2)
        else:
            if not isinstance(v, torch.Tensor):
                v = np.asarray(v)
                if v.dtype != np.uint8:
                    raise ValueError("voices must be uint8, got %s" % v.dtype)
                v = torch.from_numpy(np.ascontiguousarray(v))
            if v.dtype != torch.uint8:
                raise ValueError("voices must be uint8, got %s" % v.dtype)
            if tuple(v.shape) != (int(N), int(nsteps), 2):
                raise ValueError("voices must have shape %s, got %s" % ((int(N), int(nsteps), 2), tuple(v.shape)))
        v = v.to(device).contiguous()
        lo, hi = v[..., 0].to(torch.int32), v[..., 1].to(torch.int32)
        counted = ~((lo == VOICES_FREE[0]) & (hi == VOICES_FREE[1]))
        bad = counted & ((lo > hi) | (hi > VOICES_MAX))
        if roll is None:
            on, open_ = torch.zeros_like(lo), torch.full_like(lo, int(D))
        else:
            on, open_ = (roll == 1).sum(-1).to(torch.int32), (roll > 1).sum(-1).to(torch.int32)
        over, under = counted & ~bad & (on > hi), counted & ~bad & (on + open_ < lo)
        wrong = bad | over | under
        if wrong.numel() and bool(wrong.any()):
            n, t = [int(i) for i in wrong.nonzero()[0]]
            a, b, k, f = int(lo[n, t]), int(hi[n, t]), int(on[n, t]), int(open_[n, t])
            if bool(bad[n, t]):
                raise ValueError("voices[%d, %d] = (%d, %d): a pair is (0, 255) (free) or 0 <= lo <= hi <= %d"
                                 % (n, t, a, b, VOICES_MAX))
            if bool(over[n, t]):
                raise ValueError("frame %d of sequence %d is infeasible: the roll forces %d notes on, more than hi = %d"
                                 % (t, n, k, b))
            raise ValueError("frame %d of sequence %d is infeasible: %d notes forced on and %d free are fewer than lo = %d"
                             % (t, n, k, f, a))
        out = Constraints(roll, v)
        out._key = key
        return out


def clamp_parts(clamp):
    """(roll, voices) of what clamp_roll returned: None, a roll, or a resolved Constraints"""
    if isinstance(clamp, Constraints):
        return clamp.roll, clamp.voices
    return clamp, None


SmcResult = namedtuple('SmcResult', 'Xs log_evidence ess resamples')
SmcResult.__doc__ = """generate_smc's outputs (device tensors): Xs [N, n_out, nsteps, D] fp32 frames, log_evidence [N] fp64 (log Z:
the estimate of log p(constraints | seed, w)), ess [N, nsteps] fp64 (after each frame's reweighting), resamples [N] int32."""

SmcKeyResult = namedtuple('SmcKeyResult', SmcResult._fields + ('w_posterior', 'w_out'))
SmcKeyResult.__doc__ = """generate_smc(w_prior=...)'s outputs (DESIGN.md 12): SmcResult's four fields, log_evidence now the estimate
of log p(constraints | seed) with the key marginalised out, then w_posterior [N, nsteps, C] fp64 (the weighted mean of the
particles' label rows after each step: p(key | seed, constraints so far) for a categorical prior) and w_out [N, n_out, C]
fp32 (the label row each returned path carried).  SmcResult itself keeps four fields: callers iterate over it."""

GibbsResult = namedtuple('GibbsResult', 'Xs log_evidence renewed z')
GibbsResult.__doc__ = """generate_gibbs's outputs (device tensors, DESIGN.md 19): Xs [N, K, nsteps, D] fp32, the retained path after
every sweep; log_evidence [N, K] fp64, each sweep's log Z -- only column 0 (the unconditional filter) is an unbiased
estimate of the evidence, a conditional sweep's log Z is conditioned on the retained path; renewed [N, K, nsteps] bool,
frame k of sweep s was not taken from the pinned particle (sweep 0: all true); z [N, S + nsteps, L] fp32, the latents the
decoder was fed along the last path."""

GIBBS_SEED_STEP = 0x9E3779B97F4A7C15        # sweep s runs its whole chain under seed + s * this (mod 2^64)


def gibbs_seed(seed, s):
    """the Philox key of sweep s of a call with key `seed`"""
    return (int(seed) + int(s) * GIBBS_SEED_STEP) % 2 ** 64


def gibbs_args(sweeps, w_prior=None):
    """Validate generate_gibbs's own arguments: sweeps an integer >= 1, and no key per particle"""
    if isinstance(sweeps, (bool, np.bool_)) or not isinstance(sweeps, (int, np.integer)) or sweeps < 1:
        raise ValueError("sweeps must be an integer >= 1, got %r" % (sweeps,))
    if w_prior is not None:
        raise ValueError("sweeps do not combine with w_prior: a conditional sweep pins no label row (a key per particle "
                         "under particle Gibbs is not built)")
    return int(sweeps)


SMC_MAX_PARTICLES = 1024            # one workgroup of clv_smc_resample holds a melody's particles
SMC_MAX_CLASSES = 32                # SMC_MAX_C of csrc/smc.hip


class WPrior:
    """A prior over the label w of each of N melodies, from which generate_smc draws a w per particle.
    categorical(probs [N, C]): a key per particle, w its one-hot row.  logistic_normal(mean, log_var [N, C-1]):
    w = softmax([mean + exp(log_var / 2) * eps, 0]), the label path's own sample."""

    def __init__(self, kind, N, C, probs=None, mean=None, log_var=None):
        self.kind, self.N, self.C, self.probs, self.mean, self.log_var = kind, N, C, probs, mean, log_var

    @classmethod
    def categorical(cls, probs):
        p = np.array(probs, dtype=np.float64, ndmin=2)
        if p.ndim != 2 or p.shape[0] < 1 or not 2 <= p.shape[1] <= SMC_MAX_CLASSES:
            raise ValueError("probs must be [N, C] with 2 <= C <= %d, got shape %s" % (SMC_MAX_CLASSES, p.shape))
        if not np.all(np.isfinite(p)) or np.any(p < 0):
            raise ValueError("probs must be finite and >= 0")
        tot = p.sum(axis=1)
        if np.any(np.abs(tot - 1.0) > 1e-6):
            raise ValueError("every row of probs must sum to 1 (within 1e-6), got sums in [%r, %r]" % (tot.min(), tot.max()))
        # the last bits of the sum: P * cum_C must pass u0 + P - 1 so that the tail rule never hands out a class of mass 0
        return cls('categorical', p.shape[0], p.shape[1], probs=np.ascontiguousarray(p / tot[:, None]))

    @classmethod
    def logistic_normal(cls, mean, log_var):
        m, lv = np.array(mean, dtype=np.float32, ndmin=2), np.array(log_var, dtype=np.float32, ndmin=2)
        if m.ndim != 2 or m.shape != lv.shape or m.shape[0] < 1 or not 1 <= m.shape[1] < SMC_MAX_CLASSES:
            raise ValueError("mean and log_var must both be [N, C-1] with 2 <= C <= %d, got shapes %s and %s"
                             % (SMC_MAX_CLASSES, m.shape, lv.shape))
        if not (np.all(np.isfinite(m)) and np.all(np.isfinite(lv))):
            raise ValueError("mean and log_var must be finite")
        return cls('logistic_normal', m.shape[0], m.shape[1] + 1, mean=np.ascontiguousarray(m), log_var=np.ascontiguousarray(lv))

    @classmethod
    def uniform(cls, N, C):
        """every key equally likely"""
        return cls.categorical(np.full((int(N), int(C)), 1.0 / int(C)))

    def to(self, device):
        """the prior's arrays as device tensors (probs float64; mean, log_var float32)"""
        t = lambda a: None if a is None else torch.from_numpy(a).to(device)
        return WPrior(self.kind, self.N, self.C, t(self.probs), t(self.mean), t(self.log_var))

    def init_rows(self, m0, m1, P, seed, wr):
        """draw the label rows wr [(m1-m0) * P, C] of melodies m0 .. m1-1 (device arrays: call on the result of to())"""
        sl = lambda a: None if a is None else a[m0:m1]
        mode = ops.SMC_W_CATEGORICAL if self.kind == 'categorical' else ops.SMC_W_LOGISTIC_NORMAL
        ops.smc_init_w(m1 - m0, P, self.C, mode, seed, m0, sl(self.probs), sl(self.mean), sl(self.log_var), wr)


def smc_label_args(w, w_prior, N, C, device):
    """generate_smc takes exactly one of w [N, C] and w_prior (a WPrior over N melodies and C classes); returns
    (w as a float32 device tensor or None, the prior on the device or None)"""
    if (w is None) == (w_prior is None):
        raise ValueError("give exactly one of w and w_prior")
    if w_prior is None:
        return w.to(dtype=torch.float32, device=device), None
    if not isinstance(w_prior, WPrior):
        raise ValueError("w_prior must be a WPrior, got %r" % type(w_prior).__name__)
    if (w_prior.N, w_prior.C) != (int(N), int(C)):
        raise ValueError("w_prior is over %d melodies x %d classes, the call over %d x %d" % (w_prior.N, w_prior.C, N, C))
    return None, w_prior.to(device)


def smc_args(clamp, particles, resample_threshold, n_out, N, nsteps, D, device):
    """Validate generate_smc's arguments; returns the constraints on the device (clamp_roll: a roll, or a Constraints with
    voice counts)."""
    if clamp is None or (isinstance(clamp, Constraints) and clamp.roll is None and clamp.voices is None):
        raise ValueError("particle sampling needs a constraint roll (clamp=...)")
    if isinstance(particles, bool) or int(particles) != particles or not 1 <= particles <= SMC_MAX_PARTICLES:
        raise ValueError("particles must be an integer in [1, %d], got %r" % (SMC_MAX_PARTICLES, particles))
    tau = float(resample_threshold)
    if not 0.0 <= tau <= 1.0:
        raise ValueError("resample_threshold must lie in [0, 1], got %r" % (resample_threshold,))
    if isinstance(n_out, bool) or int(n_out) != n_out or n_out < 1:
        raise ValueError("n_out must be an integer >= 1, got %r" % (n_out,))
    if int(nsteps) < 1:
        raise ValueError("particle sampling needs nsteps >= 1, got %r" % (nsteps,))
    return clamp_roll(clamp, N, nsteps, D, device)


def temper_args(temperature, z_temperature):
    """Validate the two sampling temperatures and return the tempered model's factors (inv_T, Tz) as float32
    values, or None where both are 1 (the caller then runs exactly the untempered path).  temperature T > 0 divides a
    note's logit: inv_T = float32(1 / T), formed in double and rounded once.  z_temperature Tz >= 0 scales the latent noise;
    0 means z = its mean (z = 0 under the prior).  ValueError for a bool, a value that is not finite, T <= 0, a 1 / T that is
    zero or not finite in float32, Tz < 0."""
    vals = []
    for name, v in (('temperature', temperature), ('z_temperature', z_temperature)):
        if isinstance(v, (bool, np.bool_)):
            raise ValueError("%s must be a number, got %r" % (name, v))
        try:
            v = float(v)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number, got %r" % (name, v))
        if not np.isfinite(v):
            raise ValueError("%s must be finite, got %r" % (name, v))
        vals.append(v)
    T, Tz = vals
    if T <= 0.0:
        raise ValueError("temperature must be > 0, got %r" % (temperature,))
    if Tz < 0.0:
        raise ValueError("z_temperature must be >= 0, got %r" % (z_temperature,))
    with np.errstate(over='ignore', under='ignore'):
        inv_T, Tz32 = np.float32(1.0 / T), np.float32(Tz)
    if not np.isfinite(inv_T) or inv_T == 0:
        raise ValueError("1 / temperature must be a finite non-zero float32, got temperature %r" % (temperature,))
    if not np.isfinite(Tz32):
        raise ValueError("z_temperature must be a finite float32, got %r" % (z_temperature,))
    if inv_T == 1 and Tz32 == 1:
        return None
    return float(inv_T), float(Tz32)


VARY_HISTORY = ('own', 'source')


def vary_args(sources, w_enc, w_dec, x0, history, clamp, D, C, device):
    """Validate the arguments of a re-decoding and return them as contiguous device tensors: (sources
    [N, T, D] fp32, w_enc [N, C], w_dec [N, C] (w_enc where None), x0 [N, D] or None, the roll or None, history == 'source').
    numpy or torch in; ValueError for a wrong shape, an unknown history, and a w_dec given without a w_enc."""
    if history not in VARY_HISTORY:
        raise ValueError("history must be one of %s, got %r" % (VARY_HISTORY, history))
    if w_enc is None:
        raise ValueError("re-decoding needs w_enc, the label the encoder conditions on%s"
                         % ("" if w_dec is None else " (w_dec was given without it)"))
    t = lambda a: device_f32(a, device)
    sources = t(sources)
    if sources.dim() != 3 or sources.shape[0] < 1 or sources.shape[1] < 1 or sources.shape[2] != D:
        raise ValueError("sources must be [N, T, %d] with N, T >= 1, got shape %s" % (D, tuple(sources.shape)))
    N = int(sources.shape[0])
    w_enc = t(w_enc)
    w_dec = w_enc if w_dec is None else t(w_dec)
    for name, w in (('w_enc', w_enc), ('w_dec', w_dec)):
        if tuple(w.shape) != (N, C):
            raise ValueError("%s must have shape %s, got %s" % (name, (N, C), tuple(w.shape)))
    if x0 is not None:
        x0 = t(x0)
        if tuple(x0.shape) != (N, D):
            raise ValueError("x0 must have shape %s, got %s" % ((N, D), tuple(x0.shape)))
    return sources, w_enc, w_dec, x0, clamp_roll(clamp, N, int(sources.shape[1]), D, device), history == 'source'


STATE_FIELDS = {'cl_vrnn': ('h_enc', 'c_enc', 'h_dec', 'c_dec', 'x'), 'cl_vae': ('x_in', 'hist')}
# what else the host drivers know of a family.  Its seed: cl_vrnn steps through S >= 0 teacher-forced frames [N, S, D] from
# zero LSTM states; cl_vae's one frame [N, D] IS its state (x_in = hist = the frame) and takes no step, S = 0.  Its state
# fields that are H wide (the LSTM states); every other field is a frame, D wide.
SEED_RANK = {'cl_vrnn': 3, 'cl_vae': 2}
LSTM_FIELDS = {'cl_vrnn': ('h_enc', 'c_enc', 'h_dec', 'c_dec'), 'cl_vae': ()}
STEP_MAX = 2 ** 32 - 1                  # the Philox step is a uint32


def seed_steps(kind, x_seed):
    """S, the steps a sampler spends on its seed frames"""
    return int(x_seed.shape[1]) if SEED_RANK[kind] == 3 else 0


class GenState:
    """What a device sampler carries from one call to the next: float32 device tensors [N, width] and the
    Philox step t of the next frame (binary: the frame rows are known to hold only 0 and 1, which the states that the
    samplers return do by construction; cl_vae checks the others, binary_frames.  The mark describes the rows as the sampler
    left them: writing into a marked state's tensors voids it, and is the writer's to keep binary).  cl_vrnn: h_enc, c_enc, h_dec, c_dec
    [N, H] after the last frame's cells and x [N, D],
    the input of the next step (the last clamped sample; the bridge sample after priming with nsteps = 0).  cl_vae: x_in
    [N, D], the last frame, and hist [N, D], the frame before it.  Fields of equal width are views of one tensor `rows`
    [N, fields, width], the layout the persistent kernels read and write.  A state is never written by a call that takes
    it, so one state may be continued many times.  Access: state.h_enc, state['x'], state.tensors()."""

    def __init__(self, kind, tensors, t, rows=None):
        if kind not in STATE_FIELDS:
            raise ValueError("kind must be one of %s, got %r" % (tuple(STATE_FIELDS), kind))
        names = STATE_FIELDS[kind]
        if isinstance(t, (bool, np.bool_)) or int(t) != t or not 0 <= int(t) <= STEP_MAX:
            raise ValueError("t must be an integer in [0, 2^32), got %r" % (t,))
        if rows is None:
            if set(tensors) != set(names):
                raise ValueError("a %s state holds %s, got %s" % (kind, names, tuple(sorted(tensors))))
            ts = [tensors[k] for k in names]
            for k, v in zip(names, ts):
                if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.dim() != 2 or v.shape[0] != ts[0].shape[0] \
                        or v.shape[0] < 1 or v.device != ts[0].device:
                    raise ValueError("%s must be a float32 tensor [N, width] on the state's device, N >= 1" % k)
            if len({int(v.shape[1]) for v in ts}) == 1:
                rows = torch.stack(ts, 1).contiguous()
        elif rows.dim() != 3 or rows.shape[1] != len(names) or rows.dtype != torch.float32 or not rows.is_contiguous():
            raise ValueError("rows must be a contiguous float32 tensor [N, %d, width]" % len(names))
        self.kind, self.t, self.rows, self.binary = kind, int(t), rows, False
        self._d = {k: rows[:, i] for i, k in enumerate(names)} if rows is not None else \
            {k: tensors[k].contiguous() for k in names}

    @classmethod
    def fresh(cls, kind, cfg, device, N=None, seed_frame=None):
        """the state a sampler starts from: cl_vrnn zero LSTM states and the zero frame for N sequences; cl_vae x_in = hist =
        seed_frame [N, D]; t = 0"""
        f = dict(dtype=torch.float32, device=device)
        if SEED_RANK[kind] == 2:
            x = device_f32(seed_frame, device)
            if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] != cfg['D']:
                raise ValueError("seed_frame must be [N, %d] with N >= 1, got shape %s" % (cfg['D'], tuple(x.shape)))
            return cls(kind, None, 0, rows=torch.stack([x, x], 1).contiguous())
        return cls(kind, {k: torch.zeros(int(N), n, **f) for k, n in state_widths(kind, cfg).items()}, 0)

    @property
    def N(self):
        return int(self._d[STATE_FIELDS[self.kind][0]].shape[0])

    @property
    def device(self):
        return self._d[STATE_FIELDS[self.kind][0]].device

    def widths(self):
        return {k: int(v.shape[1]) for k, v in self._d.items()}

    def tensors(self):
        """name -> tensor, in the family's order"""
        return dict(self._d)

    def __getitem__(self, name):
        return self._d[name]

    def __getattr__(self, name):
        d = self.__dict__.get('_d')
        if d is not None and name in d:
            return d[name]
        raise AttributeError(name)

    def _like(self, f):
        if self.rows is not None:
            out = GenState(self.kind, None, self.t, rows=f(self.rows).contiguous())
        else:
            out = GenState(self.kind, {k: f(v) for k, v in self._d.items()}, self.t)
        out.binary = self.binary              # copies and selections of rows hold what the rows held
        return out

    def _sampled(self):
        """mark a state that a sampler built from its own frames"""
        self.binary = True
        return self

    def clone(self):
        return self._like(lambda v: v.clone())

    def select(self, index):
        """rows by an integer index, repeats allowed: branching.  Row n of a call draws the noise of index n, so two copies
        of one prefix at different rows continue differently."""
        idx = np.asarray(index.cpu() if isinstance(index, torch.Tensor) else index)
        if idx.ndim != 1 or idx.size < 1 or idx.dtype == np.bool_ or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("index must be a non-empty 1-D sequence of integers, got %r" % (index,))
        if idx.min() < 0 or idx.max() >= self.N:
            raise ValueError("index must lie in [0, %d), got [%d, %d]" % (self.N, idx.min(), idx.max()))
        ix = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(self.device)
        return self._like(lambda v: v.index_select(0, ix))

    def to_numpy(self):
        """a dict of float32 arrays and t (an int64 scalar array) that np.savez can hold"""
        out = {k: v.detach().cpu().numpy().astype(np.float32, copy=True) for k, v in self._d.items()}
        out['t'] = np.asarray(self.t, np.int64)
        return out

    @classmethod
    def from_numpy(cls, d, device):
        """the state of to_numpy() (or of np.load of its np.savez) on `device`; the family follows from the names"""
        names = set(d.keys() if hasattr(d, 'keys') else d) - {'t'}
        kinds = [k for k, f in STATE_FIELDS.items() if set(f) == names]
        if not kinds or 't' not in (d.keys() if hasattr(d, 'keys') else d):
            raise ValueError("not a sampler state: fields %s" % (tuple(sorted(names)),))
        t = np.asarray(d['t'])
        if t.size != 1:
            raise ValueError("t must be one integer, got shape %s" % (t.shape,))
        return cls(kinds[0], {k: device_f32(np.asarray(d[k]), device) for k in STATE_FIELDS[kinds[0]]}, int(t.reshape(())))


def resume_args(state, kind, N, widths, nframes):
    """Validate a sampler's state argument (None: a fresh start) against the call: a GenState of this family, N rows, the
    model's widths (dict name -> width), and a last Philox step t + nframes that fits a uint32.  Returns t, the step of the
    call's frame 0.  ValueError otherwise."""
    if state is None:
        t0 = 0
    else:
        if not isinstance(state, GenState):
            raise ValueError("state must be a GenState, got %r" % type(state).__name__)
        if state.kind != kind:
            raise ValueError("a %s state cannot continue a %s model" % (state.kind, kind))
        if N is not None and state.N != int(N):
            raise ValueError("the state holds %d sequences, the call %d" % (state.N, N))
        if state.widths() != dict(widths):
            raise ValueError("the state's widths %s are not the model's %s" % (state.widths(), dict(widths)))
        t0 = state.t
    if t0 + int(nframes) > STEP_MAX:
        raise ValueError("t = %d + %d frames passes the last Philox step 2^32 - 1" % (t0, nframes))
    return t0


def state_widths(kind, cfg):
    return {k: cfg['H'] if k in LSTM_FIELDS[kind] else cfg['D'] for k in STATE_FIELDS[kind]}


class FilterState:
    """What a filter stream carries from one advance to the next, for N melodies x P particles (global row
    m * P + p, R = N * P rows): gen, the rows' sampler state as a GenState over R rows (what a particle hands to its
    descendants; gen.t is the Philox step of the next frame); logW [R] and logZ [N] fp64, nres [N] and collapses [N] int32;
    and the pending store, the steps whose frames are not emitted yet -- per melody a ring of cap slots, pending step j
    (oldest first) in slot (head[m] + j) % cap of pend_anc [cap, R] int32 (every row's ancestor) and pend_hist [cap, R, D]
    uint8 (every row's frame), len[m] of them live; head, len [N] int32.  Unlike a GenState, a FilterState is CONSUMED by the
    call that takes it (the store is too large to copy per call): clone() first to keep one."""
    ARRAYS = ('logW', 'logZ', 'nres', 'collapses', 'pend_anc', 'pend_hist', 'head', 'len')
    DTYPES = dict(logW=torch.float64, logZ=torch.float64, nres=torch.int32, collapses=torch.int32, pend_anc=torch.int32,
                  pend_hist=torch.uint8, head=torch.int32, len=torch.int32)

    def __init__(self, gen, P, **arrays):
        if not isinstance(gen, GenState):
            raise ValueError("gen must be a GenState, got %r" % type(gen).__name__)
        if isinstance(P, (bool, np.bool_)) or int(P) != P or not 1 <= P <= SMC_MAX_PARTICLES or gen.N % int(P):
            raise ValueError("particles must be an integer in [1, %d] that divides the state's %d rows, got %r"
                             % (SMC_MAX_PARTICLES, gen.N, P))
        if set(arrays) != set(self.ARRAYS):
            raise ValueError("a filter state holds %s, got %s" % (self.ARRAYS, tuple(sorted(arrays))))
        self.gen, self.P = gen, int(P)
        R, N = gen.N, gen.N // int(P)
        cap = int(arrays['pend_anc'].shape[0]) if arrays['pend_anc'].dim() == 2 else 0
        D = int(arrays['pend_hist'].shape[2]) if arrays['pend_hist'].dim() == 3 else 0
        shapes = dict(logW=(R,), logZ=(N,), nres=(N,), collapses=(N,), pend_anc=(cap, R), pend_hist=(cap, R, D), head=(N,),
                      len=(N,))
        for k in self.ARRAYS:
            v = arrays[k]
            if not isinstance(v, torch.Tensor) or v.dtype != self.DTYPES[k] or tuple(v.shape) != shapes[k] or cap < 1 \
                    or D < 1 or v.device != gen.device:
                raise ValueError("%s must be a %s tensor of shape %s on the state's device" % (k, self.DTYPES[k], shapes[k]))
            setattr(self, k, v.contiguous())

    @classmethod
    def fresh(cls, gen, P, D, cap, logW, logZ, nres):
        """the state after a stream's first chunk, before its commit: nothing pending, no collapse"""
        N, d = gen.N // P, gen.device
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=d)
        return cls(gen, P, logW=logW, logZ=logZ, nres=nres, collapses=i32(N), pend_anc=i32(cap, gen.N),
                   pend_hist=torch.zeros(cap, gen.N, D, dtype=torch.uint8, device=d), head=i32(N), len=i32(N))

    kind = property(lambda self: self.gen.kind)
    t = property(lambda self: self.gen.t)
    R = property(lambda self: self.gen.N)
    N = property(lambda self: self.gen.N // self.P)
    D = property(lambda self: int(self.pend_hist.shape[2]))
    cap = property(lambda self: int(self.pend_anc.shape[0]))
    device = property(lambda self: self.gen.device)

    def pending(self):
        """the pending frames per melody, [N] int64 on the host (one small copy, which waits for the device)"""
        return self.len.cpu().numpy().astype(np.int64)

    def buffers(self):
        """the rows' state as contiguous fp32 [R, width] buffers (what clv_smc_gather permutes)"""
        g = self.gen
        return [g.rows.view(g.N, -1)] if g.rows is not None else [g[k] for k in STATE_FIELDS[g.kind]]

    def reserve(self, need):
        """make the ring hold `need` steps per melody: a larger store, every melody's live steps from slot 0 on"""
        cap, N, P, D = self.cap, self.N, self.P, self.D
        if need <= cap:
            return
        new = max(int(need), 2 * cap)
        slot = ((self.head.to(torch.int64)[None, :] + torch.arange(new, device=self.device)[:, None]) % cap)   # [new, N]
        m = torch.arange(N, device=self.device)[None, :]
        self.pend_anc = self.pend_anc.view(cap, N, P)[slot, m].reshape(new, N * P).contiguous()
        self.pend_hist = self.pend_hist.view(cap, N, P * D)[slot, m].reshape(new, N * P, D).contiguous()
        self.head = torch.zeros_like(self.head)

    def clone(self):
        return FilterState(self.gen.clone(), self.P, **{k: getattr(self, k).clone() for k in self.ARRAYS})

    def to_numpy(self):
        """a dict of arrays that np.savez can hold: the GenState's (to_numpy), particles, and the arrays above"""
        out = self.gen.to_numpy()
        out['particles'] = np.asarray(self.P, np.int64)
        out.update({k: getattr(self, k).detach().cpu().numpy().copy() for k in self.ARRAYS})
        return out

    @classmethod
    def from_numpy(cls, d, device):
        """the state of to_numpy() (or of np.load of its np.savez) on `device`"""
        keys = set(d.keys() if hasattr(d, 'keys') else d)
        if not set(cls.ARRAYS) | {'particles', 't'} <= keys:
            raise ValueError("not a filter state: fields %s" % (tuple(sorted(keys)),))
        gen = GenState.from_numpy({k: d[k] for k in keys - set(cls.ARRAYS) - {'particles'}}, device)
        arrays = {k: torch.as_tensor(np.ascontiguousarray(np.asarray(d[k])), device=device).to(cls.DTYPES[k])
                  for k in cls.ARRAYS}
        return cls(gen, int(np.asarray(d['particles']).reshape(())), **arrays)


def chunk_frames(clamp):
    """the number of frames a chunk's constraints cover: row count of its roll, else of its voice-count array"""
    parts = (clamp.roll, clamp.voices) if isinstance(clamp, Constraints) else (clamp,)
    for a in parts:
        if a is not None and not isinstance(a, tuple):
            shape = tuple(a.shape) if isinstance(a, torch.Tensor) else np.asarray(a).shape
            if len(shape) != 3 or shape[1] < 1:
                raise ValueError("a chunk's constraints are [N, n, ...] with n >= 1 frames, got shape %s" % (shape,))
            return int(shape[1])
    raise ValueError("a filter stream's chunk needs a constraint roll, or voice counts given as an array [N, n, 2]")


def generate_samples_numpy(engine, x_seeds, nsteps, w_vals=None, seed=0, z_prior=False, clamp=None, particles=None,
                           resample_threshold=0.5, return_evidence=False, w_prior=None, return_key=False, temperature=1.0,
                           z_temperature=1.0, state=None, return_state=False, kind=None, sweeps=None, return_renewed=False):
    """generate_samples_device of both families: engine.generate, or with particles engine.generate_smc, on host arrays ->
    [N, nsteps, D] float64 (and what smc_samples_numpy adds; with return_state (Xs, GenState)).  kind: the family
    ('cl_vrnn' | 'cl_vae'; default: the engine's).  sweeps=K (with particles): engine.generate_gibbs, the last sweep's
    path (gibbs_samples_numpy)."""
    temper = dict(temperature=temperature, z_temperature=z_temperature)
    temper_args(**temper)
    if sweeps is None and return_renewed:
        raise ValueError("return_renewed needs sweeps")
    if sweeps is not None:
        gibbs_args(sweeps, w_prior)
        if particles is None:
            raise ValueError("sweeps needs particles")
        if return_key:
            raise ValueError("sweeps do not combine with return_key: no key per particle under particle Gibbs")
        if state is not None or return_state:
            raise ValueError("a state does not combine with sweeps")
    d = engine.device
    if state is not None or return_state:
        return _resume_samples_numpy(engine, kind or engine.STATE_KIND, x_seeds, nsteps, w_vals, seed, z_prior, clamp,
                                     particles is not None or w_prior is not None or return_evidence or return_key, temper,
                                     state, return_state)
    if x_seeds is None:
        raise ValueError("give x_seeds (or a state to resume from)")
    xs = device_f32(x_seeds, d)
    if (w_vals is None) == (w_prior is None):
        raise ValueError("give exactly one of w_vals and w_prior")
    if particles is None and (w_prior is not None or return_key):
        raise ValueError("w_prior and return_key need particles")
    w = None if w_vals is None else device_f32(w_vals, d)
    if particles is not None:
        smc_args(clamp, particles, resample_threshold, 1, xs.shape[0], nsteps, engine.cfg['D'], d)
        if sweeps is not None:
            return gibbs_samples_numpy(engine, xs, w, nsteps, seed, z_prior, clamp, particles, sweeps, resample_threshold,
                                       return_evidence, return_renewed, **temper)
        return smc_samples_numpy(engine, xs, w, nsteps, seed, z_prior, clamp, particles, resample_threshold, return_evidence,
                                 w_prior=w_prior, return_key=return_key, **temper)
    if return_evidence:
        raise ValueError("return_evidence needs particles")
    clamp = clamp_roll(clamp, xs.shape[0], int(nsteps), engine.cfg['D'], d)
    return engine.generate(xs, w, int(nsteps), seed=int(seed), z_prior=z_prior, clamp=clamp,
                           **temper).cpu().numpy().astype(np.float64)


def _resume_samples_numpy(engine, kind, x_seeds, nsteps, w_vals, seed, z_prior, clamp, smc, temper, state, return_state):
    """generate_samples_numpy from and / or to a state: every refusal, then engine.generate"""
    cfg, d = engine.cfg, engine.device
    if smc:
        raise ValueError("a state does not combine with particles (the filter's per-particle state is not carried)")
    if w_vals is None:
        raise ValueError("give w_vals")
    if state is not None and not isinstance(state, GenState):
        raise ValueError("state must be a GenState, got %r" % type(state).__name__)
    rank = SEED_RANK[kind]
    if rank == 2 and state is not None and x_seeds is not None:
        raise ValueError("a cl_vae state holds its last two frames: give no x_seeds with it")
    if x_seeds is None:
        if state is None:
            raise ValueError("give x_seeds or a state")
        N = state.N
        xs = torch.zeros(N, 0, cfg['D'], dtype=torch.float32, device=d) if rank == 3 else None
    else:
        xs = device_f32(x_seeds, d)
        if xs.dim() != rank or xs.shape[0] < 1 or xs.shape[-1] != cfg['D']:
            raise ValueError("x_seeds must be %s, got shape %s" % (("[N, S, %d]" if rank == 3 else "[N, %d]") % cfg['D'],
                                                                    tuple(xs.shape)))
        N = int(xs.shape[0])
    resume_args(state, kind, N, state_widths(kind, cfg), seed_steps(kind, xs) + int(nsteps))
    w = device_f32(w_vals, d)
    if tuple(w.shape) != (N, cfg['C']):
        raise ValueError("w_vals must have shape %s, got %s" % ((N, cfg['C']), tuple(w.shape)))
    clamp = clamp_roll(clamp, N, int(nsteps), cfg['D'], d)
    out = engine.generate(xs, w, int(nsteps), seed=int(seed), z_prior=z_prior, clamp=clamp, state=state,
                          return_state=return_state, **temper)
    if return_state:
        return out[0].cpu().numpy().astype(np.float64), out[1]
    return out.cpu().numpy().astype(np.float64)


def vary_samples_numpy(engine, sources, w_enc, w_dec=None, x0=None, history='own', seed=0, clamp=None, temperature=1.0,
                       z_temperature=1.0, return_xhat=False, return_latents=False):
    """vary_samples_device of both families: engine.vary on host arrays -> [N, T, D] float64 (and x_hat, float64; with
    return_latents also (z, z_mean, z_log_var), each [N, T, L] float64, last)"""
    temper_args(temperature, z_temperature)
    cfg, d = engine.cfg, engine.device
    sources, w_enc, w_dec, x0, clamp, _ = vary_args(sources, w_enc, w_dec, x0, history, clamp, cfg['D'], cfg['C'], d)
    xhat = torch.zeros_like(sources) if return_xhat else None
    kw = {}
    if return_latents:
        kw['zout'] = torch.zeros(3, sources.shape[0], sources.shape[1], cfg['L'], dtype=torch.float32, device=d)
    Xs = engine.vary(sources, w_enc, w_dec, x0=x0, history=history, seed=int(seed), clamp=clamp, temperature=temperature,
                     z_temperature=z_temperature, xhat_out=xhat, **kw)
    out = [Xs.cpu().numpy().astype(np.float64)]
    if return_xhat:
        out.append(xhat.cpu().numpy().astype(np.float64))
    if return_latents:
        zo = kw['zout'].cpu().numpy().astype(np.float64)
        out.append((zo[2], zo[0], zo[1]))
    return out[0] if len(out) == 1 else tuple(out)


def encode_latents_numpy(engine, sources, w_enc, seed=0, z_temperature=1.0):
    """encode_latents_device of both families: the latents of engine.vary's loop on host arrays ->
    (z, z_mean, z_log_var), each [N, T, L] float64.  The encoder sees only the sources and w_enc, so the decoder half of
    the launch (run under w_enc, free) does not reach them."""
    return vary_samples_numpy(engine, sources, w_enc, seed=seed, z_temperature=z_temperature, return_latents=True)[1]


def decode_args(z, w_dec, x0, history, clamp, noise_rows, D, L, C, device):
    """Validate the arguments of a decoding and return them as contiguous device tensors: (z [N, T, L] fp32,
    w_dec [N, C], x0 [N, D] or None, history [N, T, D] or None ('own'), the roll or None, noise_rows [N] int32 or None).
    numpy or torch in; ValueError for a wrong shape, a z whose last dimension is not L, a history that is neither 'own' nor
    an [N, T, D] array, and noise_rows that are not N integers >= 0."""
    t = lambda a: device_f32(a, device)
    if z is None or w_dec is None:
        raise ValueError("decoding needs a latent path z and the decoder's label w_dec")
    z = t(z)
    if z.dim() != 3 or z.shape[0] < 1 or z.shape[1] < 1 or z.shape[2] != L:
        raise ValueError("z must be [N, T, %d] with N, T >= 1, got shape %s" % (L, tuple(z.shape)))
    N, T = int(z.shape[0]), int(z.shape[1])
    w_dec = t(w_dec)
    if tuple(w_dec.shape) != (N, C):
        raise ValueError("w_dec must have shape %s, got %s" % ((N, C), tuple(w_dec.shape)))
    if x0 is not None:
        x0 = t(x0)
        if tuple(x0.shape) != (N, D):
            raise ValueError("x0 must have shape %s, got %s" % ((N, D), tuple(x0.shape)))
    if isinstance(history, str):
        if history != 'own':
            raise ValueError("history must be 'own' or an [N, T, %d] array, got %r" % (D, history))
        history = None
    else:
        if history is None:
            raise ValueError("history must be 'own' or an [N, T, %d] array, got None" % D)
        history = t(history)
        if tuple(history.shape) != (N, T, D):
            raise ValueError("history must have shape %s, got %s" % ((N, T, D), tuple(history.shape)))
    if noise_rows is not None:
        nr = noise_rows.cpu().numpy() if isinstance(noise_rows, torch.Tensor) else np.asarray(noise_rows)
        if nr.dtype == np.bool_ or not np.issubdtype(nr.dtype, np.integer) or nr.shape != (N,):
            raise ValueError("noise_rows must be %d integers, got dtype %s shape %s" % (N, nr.dtype, nr.shape))
        if nr.min() < 0 or nr.max() >= 2 ** 31:
            raise ValueError("noise_rows must lie in [0, 2^31), got [%d, %d]" % (nr.min(), nr.max()))
        noise_rows = torch.from_numpy(np.ascontiguousarray(nr, dtype=np.int32)).to(device)
    return z, w_dec, x0, history, clamp_roll(clamp, N, T, D, device), noise_rows


def decode_temper(temperature):
    """the note temperature of a decoding: temper_args without a latent temperature (the path is given) -> inv_T"""
    t = temper_args(temperature, 1.0)
    return 1.0 if t is None else t[0]


def decode_latents_numpy(engine, z, w_dec, x0=None, history='own', seed=0, clamp=None, temperature=1.0, noise_rows=None,
                         return_xhat=False):
    """decode_latents_device of both families: engine.decode_latents on host arrays -> [N, T, D] float64 (and x_hat, float64)"""
    decode_temper(temperature)
    cfg, d = engine.cfg, engine.device
    z, w_dec, x0, hist, clamp, noise_rows = decode_args(z, w_dec, x0, history, clamp, noise_rows, cfg['D'], cfg['L'],
                                                        cfg['C'], d)
    xhat = torch.zeros(z.shape[0], z.shape[1], cfg['D'], dtype=torch.float32, device=d) if return_xhat else None
    Xs = engine.decode_latents(z, w_dec, x0=x0, history='own' if hist is None else hist, seed=int(seed), clamp=clamp,
                       temperature=temperature, noise_rows=noise_rows, xhat_out=xhat)
    Xs = Xs.cpu().numpy().astype(np.float64)
    return (Xs, xhat.cpu().numpy().astype(np.float64)) if return_xhat else Xs


def lerp_rows(a, ia, b, ib, alpha):
    """out [R, n] = (1 - alpha[r]) a[ia[r]] + alpha[r] b[ib[r]] on the device (clv_lerp_rows: two fmas, exact at both ends);
    a [Ra, n], b [Rb, n] float32 device tensors, ia, ib, alpha sequences of R entries"""
    d = a.device
    a, b = a.contiguous(), b.contiguous()
    ia, ib = np.asarray(ia, np.int64), np.asarray(ib, np.int64)
    R, n = len(ia), int(a.shape[1])
    if a.dim() != 2 or b.dim() != 2 or int(b.shape[1]) != n or len(ib) != R or len(alpha) != R or R < 1 or n < 1:
        raise ValueError("lerp_rows: a [Ra, n], b [Rb, n] and R >= 1 entries each of ia, ib, alpha")
    if ia.min() < 0 or ia.max() >= a.shape[0] or ib.min() < 0 or ib.max() >= b.shape[0]:
        raise ValueError("lerp_rows: a row index is out of range")
    i32 = lambda v: torch.from_numpy(np.ascontiguousarray(v, dtype=np.int32)).to(d)
    out = torch.zeros(R, n, dtype=torch.float32, device=d)
    ops.lerp_rows(R, n, a, i32(ia), b, i32(ib), torch.as_tensor(np.asarray(alpha, np.float32), device=d), out)
    return out


class _NoiseRows:
    """a frame chain's uniforms: those of its own N rows, or under noise_rows drawn for max(noise_rows) + 1 rows and gathered
    per row (clv_gather_rows)"""

    def __init__(self, noise_rows, N, D, device, first=0):
        self.N, self.D, self.nr, self.first = N, D, noise_rows, first       # first: the Philox index of own row 0's note 0
        if noise_rows is not None:
            self.R = int(noise_rows.max().item()) + 1
            self.idx = noise_rows.to(torch.int64).contiguous()
            self.u_all = torch.zeros(self.R, D, dtype=torch.float32, device=device)

    def draw(self, u, seed, counter, step=0):
        """the uniforms of Philox step `step` + the device counter (clv_philox_uniform adds the two)"""
        if self.nr is None:
            ops.philox_uniform(u, self.N * self.D, seed, step, 1, self.first, step_dev=counter)
        else:
            ops.philox_uniform(self.u_all, self.R * self.D, seed, step, 1, 0, step_dev=counter)
            ops.gather_rows(self.N, self.D, self.u_all, self.idx, u)


def smc_samples_numpy(engine, x_seed, w, nsteps, seed, z_prior, clamp, particles, resample_threshold, return_evidence,
                      w_prior=None, return_key=False, temperature=1.0, z_temperature=1.0):
    """generate_samples_device(particles=P): one draw per melody, [N, nsteps, D] float64 (and log_evidence [N] float64;
    with return_key, under a w_prior, also w_posterior [N, nsteps, C] and the path's label w_out [N, C], float64)"""
    if return_key and w_prior is None:
        raise ValueError("return_key needs a w_prior")
    kw = {} if w_prior is None else dict(w_prior=w_prior)
    if temper_args(temperature, z_temperature) is not None:
        kw.update(temperature=temperature, z_temperature=z_temperature)
    r = engine.generate_smc(x_seed, w, int(nsteps), clamp, particles, resample_threshold, n_out=1, seed=int(seed),
                            z_prior=z_prior, **kw)
    out = [r.Xs[:, 0].cpu().numpy().astype(np.float64)]
    if return_evidence:
        out.append(r.log_evidence.cpu().numpy())
    if return_key:
        out += [r.w_posterior.cpu().numpy(), r.w_out[:, 0].cpu().numpy().astype(np.float64)]
    return out[0] if len(out) == 1 else tuple(out)


def gibbs_samples_numpy(engine, x_seed, w, nsteps, seed, z_prior, clamp, particles, sweeps, resample_threshold,
                        return_evidence, return_renewed=False, temperature=1.0, z_temperature=1.0):
    """generate_samples_device(particles=P, sweeps=K): the last sweep's path per melody, [N, nsteps, D] float64 (then, with
    return_evidence, sweep 0's log_evidence [N] float64 -- the only unbiased one -- and, with return_renewed, renewed
    [N, K, nsteps] bool)"""
    r = engine.generate_gibbs(x_seed, w, int(nsteps), clamp, particles, sweeps, resample_threshold, seed=int(seed),
                              z_prior=z_prior, temperature=temperature, z_temperature=z_temperature)
    out = [r.Xs[:, -1].cpu().numpy().astype(np.float64)]
    if return_evidence:
        out.append(r.log_evidence[:, 0].cpu().numpy())
    if return_renewed:
        out.append(r.renewed.cpu().numpy())
    return out[0] if len(out) == 1 else tuple(out)


class _Smc:
    """Device state of one chunk of G melodies x P particles: the weight increments, normalized log weights,
    log Z, ESS, resample counts, ancestors A_t [nsteps, R] and the uint8 frame history [nsteps, R, D].  step() is the SMC
    part of one frame (sample, resample, gather); finish() draws the returned paths."""

    def __init__(self, G, P, nsteps, S, D, tau, seed, m0, clamp, device, wr=None):
        self.G, self.P, self.R, self.nsteps, self.S, self.D = G, P, G * P, nsteps, S, D
        self.wr = wr                # the particles' own label rows [R, C] under a key prior, else None
        if wr is not None:
            self.w_post = torch.zeros(G, nsteps, wr.shape[1], dtype=torch.float64, device=device)
        self.tau, self.seed, self.m0 = tau, seed, m0
        self.clamp, self.voices = clamp_parts(clamp)        # the roll (None under voice counts alone) and the counts
        f64 = dict(dtype=torch.float64, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        self.ell, self.logW = torch.zeros(self.R, **f64), torch.zeros(self.R, **f64)
        self.logZ, self.ess = torch.zeros(G, **f64), torch.zeros(G, nsteps, **f64)
        self.nres, self.flag = torch.zeros(G, **i32), torch.zeros(G, **i32)
        self.anc = torch.zeros(nsteps, self.R, **i32)
        self.hist = torch.zeros(nsteps, self.R, D, dtype=torch.uint8, device=device)

    ref = None                      # the path a conditional sweep pins (_GibbsSmc); the plain filter pins nothing

    def step(self, xhat, u, counter, x_next, gather):
        self.sample(xhat, u, counter, x_next)
        ops.smc_resample(self.G, self.P, self.nsteps, self.S, self.seed, self.m0, self.tau, self.ell, self.logW, self.logZ,
                         self.ess, self.nres, self.flag, self.anc, counter)
        gather(self.anc, self.flag, counter)
        if self.wr is not None:
            ops.smc_w_posterior(self.G, self.P, self.wr.shape[1], self.nsteps, self.S, self.logW, self.wr, counter,
                                self.w_post)

    def sample(self, xhat, u, counter, x_next):
        if self.voices is None:
            ops.smc_sample(self.R, self.D, self.P, self.nsteps, self.S, xhat, u, self.clamp, counter, x_next, self.ell,
                           self.hist)
        else:
            ops.smc_sample_voices(self.R, self.D, self.P, self.nsteps, self.S, xhat, u, self.clamp, self.voices, counter,
                                  x_next, self.ell, self.hist)

    def finish(self, n_out, Xs, w_out=None):
        picks = None if self.wr is None else torch.zeros(self.G, n_out, dtype=torch.int32, device=Xs.device)
        ops.smc_backtrack(self.G, self.P, self.nsteps, self.D, n_out, self.seed, self.m0, self.S + self.nsteps, self.logW,
                          self.anc, self.hist, Xs, picks)
        if self.wr is not None:     # the gather moved the rows with the state: the final particle holds its path's key
            ops.smc_take_w(self.G, self.P, self.wr.shape[1], n_out, picks, self.wr, w_out)


class _Path:
    """The path particle Gibbs retains for G melodies: frames x [G, nsteps, D] uint8, the latents of every
    chain step z [G, S + nsteps, L], the bridge sample b [G, D] (None without seed steps)"""

    def __init__(self, G, nsteps, S, D, L, device):
        self.x = torch.zeros(G, nsteps, D, dtype=torch.uint8, device=device)
        self.z = torch.zeros(G, S + nsteps, L, dtype=torch.float32, device=device)
        self.b = torch.zeros(G, D, dtype=torch.float32, device=device) if S > 0 else None


class _GibbsSmc(_Smc):
    """One sweep of particle Gibbs over a chunk: the filter, which also keeps every row's latents of every chain step
    (zhist [T, R, L]) and its sample of step S - 1 (bridge_rows [R, D]) so that the path it ends on can be retained; with
    ref (a _Path) a conditional sweep: row m * P is pinned to ref and the resampling is the conditional one."""

    def __init__(self, G, P, nsteps, S, D, L, tau, seed, m0, clamp, device, ref=None):
        super().__init__(G, P, nsteps, S, D, tau, seed, m0, clamp, device)
        self.L, self.ref = L, ref
        self.zhist = torch.zeros(S + nsteps, self.R, L, dtype=torch.float32, device=device)
        self.bridge_rows = torch.zeros(self.R, D, dtype=torch.float32, device=device) if S > 0 else None

    def pin_z(self, z, counter):
        ops.smc_pin_z(self.G, self.P, self.L, self.S + self.nsteps, self.ref.z, counter, z)

    def step(self, xhat, u, counter, x_next, gather):
        if self.ref is None:
            return super().step(xhat, u, counter, x_next, gather)
        self.sample(xhat, u, counter, x_next)
        ops.smc_pin_frame(self.G, self.P, self.D, self.nsteps, self.S, self.ref.x, self.ref.b, counter, x_next, self.hist)
        ops.smc_resample_conditional(self.G, self.P, self.nsteps, self.S, self.seed, self.m0, self.tau, self.ell, self.logW,
                                     self.logZ, self.ess, self.nres, self.flag, self.anc, counter)
        gather(self.anc, self.flag, counter)

    def record(self, t, z, x_next):
        """after chain step t (eagerly): every row's latents, and at step S - 1 its bridge sample"""
        self.zhist[t].copy_(z[:self.R])
        if t == self.S - 1:
            self.bridge_rows.copy_(x_next)

    def retain(self, path, Xs, renewed):
        """draw the sweep's path (Xs [G, 1, nsteps, D]) and write it to path; renewed [G, nsteps] uint8"""
        picks = torch.zeros(self.G, 1, dtype=torch.int32, device=Xs.device)
        ops.smc_backtrack(self.G, self.P, self.nsteps, self.D, 1, self.seed, self.m0, self.S + self.nsteps, self.logW,
                          self.anc, self.hist, Xs, picks)
        ops.smc_backtrack_path(self.G, self.P, self.nsteps, self.S, self.D, self.L, picks, self.anc, self.hist, self.zhist,
                               self.bridge_rows, path.x, path.z, path.b, renewed)


class _StreamSmc(_Smc):
    """One chunk of a filter stream: the filter whose resampling uniforms count their Philox step on from
    t0 and which, given the FilterState of the chunks before, continues its logW, logZ and nres (in place)."""

    def __init__(self, G, P, nsteps, S, D, tau, seed, clamp, device, t0=0, state=None):
        super().__init__(G, P, nsteps, S, D, tau, seed, 0, clamp, device)
        self.t0, self.carry = int(t0), state is not None
        if state is not None:
            self.logW, self.logZ, self.nres = state.logW, state.logZ, state.nres

    def step(self, xhat, u, counter, x_next, gather):
        self.sample(xhat, u, counter, x_next)
        ops.smc_resample_carry(self.G, self.P, self.nsteps, self.S, self.seed, self.m0, self.tau, self.ell, self.logW,
                               self.logZ, self.ess, self.nres, self.flag, self.anc, counter, self.t0, self.carry)
        gather(self.anc, self.flag, counter)


FilterEmit = namedtuple('FilterEmit', 'state frames counts ess picks')
FilterEmit.__doc__ = """What a filter stream's call hands out (DESIGN.md 23): the FilterState to go on from; frames [N, max count, D]
uint8 (device), of which row j < counts[m] of melody m is valid, oldest first; counts [N] int64 (host); ess [N, n] fp64 of
an advance's frames (else None); picks [N] int64 (host) the particle a collapse or the finish drew, -1 where none."""


def _smc_chunks(N, P, cap, chunk):
    """melody ranges [m0, m1): at most `chunk` melodies (default: all) and at most cap rows (None: no cap) per chunk"""
    g = N if chunk is None else int(chunk)
    if g < 1:
        raise ValueError("chunk must be >= 1, got %r" % (chunk,))
    if cap is not None:
        if P > cap:
            raise ValueError("%d particles exceed the engine's batch size %d" % (P, cap))
        g = min(g, cap // P)
    return [(m0, min(N, m0 + g)) for m0 in range(0, N, g)]


def _smc_drive(chunks, run_chunk, N, nsteps, D, n_out, device, C=None):
    """C: the number of classes when the filter carries a key per particle (SmcKeyResult), else None (SmcResult)"""
    f = dict(device=device)
    out = SmcResult(torch.zeros(N, n_out, nsteps, D, dtype=torch.float32, **f), torch.zeros(N, dtype=torch.float64, **f),
                    torch.zeros(N, nsteps, dtype=torch.float64, **f), torch.zeros(N, dtype=torch.int32, **f))
    if C is not None:
        out = SmcKeyResult(*out, torch.zeros(N, nsteps, C, dtype=torch.float64, **f),
                           torch.zeros(N, n_out, C, dtype=torch.float32, **f))
    for m0, m1 in chunks:
        smc = run_chunk(m0, m1)
        if C is None:
            smc.finish(n_out, out.Xs[m0:m1])
        else:
            smc.finish(n_out, out.Xs[m0:m1], out.w_out[m0:m1])
            out.w_posterior[m0:m1].copy_(smc.w_post)
        out.log_evidence[m0:m1].copy_(smc.logZ)
        out.ess[m0:m1].copy_(smc.ess)
        out.resamples[m0:m1].copy_(smc.nres)
    return out


def _zout_ok(zout, N, T, L):
    """the latents' output of vary: a contiguous float32 device tensor [3, N, T, L]"""
    if tuple(zout.shape) != (3, N, T, L) or zout.dtype != torch.float32 or not zout.is_contiguous():
        raise ValueError("zout must be a contiguous float32 tensor of shape %s, got %s %s" % ((3, N, T, L), zout.dtype,
                                                                                            tuple(zout.shape)))
    return zout


def _replay(frame, nsteps, use_graph, before=None, after=None):
    """run frame() nsteps times: step 0 eagerly (it sizes every workspace), then one captured graph replayed per step;
    before(t) runs eagerly ahead of step t, after(t) behind it"""
    graph = None
    for t in range(nsteps):
        if before is not None:
            before(t)
        if use_graph and t == 1:
            with ops.Graph() as graph:
                frame()
        if graph is not None:
            graph.launch()
        else:
            frame()
        if after is not None:
            after(t)


class _VaeRows:
    """cl_vae's part of a frame chain over R rows, at most the batch size: the engine's own buffers and layer chains"""

    def __init__(self, eng, R):
        if R > eng.B:
            raise ValueError("%d sequences exceed the engine's batch size %d" % (R, eng.B))
        self.eng, self.R = eng, R
        self.zargs, self.z, self.xhat = eng.zargs, eng.z, eng.logits

    def encode(self, x, w):
        self.eng.encode_z(x, w, self.R)

    def decode(self, w, z, xp, act):
        self.eng.decode(w, z, xp, self.R, act=act)

    def carried(self, x_enc, x_next):
        """what a particle hands to its descendants: x_enc too, the decoder's previous frame of the next step"""
        return [x_next, x_enc]


class _VrnnRows:
    """cl_vrnn's part of a frame chain over R rows (any number): a state of its own, the probabilities in st['xhat']"""

    def __init__(self, eng, R):
        self.eng, self.R = eng, R
        self.st = eng.new_state(R)
        self.zargs, self.xhat = self.st['zargs'], self.st['xhat']
        self.z = torch.zeros(R, eng.cfg['L'], dtype=torch.float32, device=eng.device)

    def encode(self, x, w):
        self.eng.enc_step(x, w, self.st)

    def decode(self, w, z, xp, act):
        self.eng.dec_step(z, xp, w, self.st, act=act)

    def carried(self, x_enc, x_next):
        """what a particle hands to its descendants: both LSTM states and its sample"""
        return [self.st[k] for k in LSTM_FIELDS['cl_vrnn']] + [x_next]


class _Chain:
    """The launches of one frame of every device sampling loop (generate, vary, decode_latents and generate_smc of both
    families) over the rows of a _VaeRows / _VrnnRows, and its replay.  Three frame slots: x_enc, the
    encoder's input; x_dec, the decoder's previous frame; x_next, the sample.  The call's choices:
    * x_enc: sources[:, t] of sources [R, nsteps, D] (clv_take_frame through the device step counter), else the sample fed
      back -- from step S = seed_frames.shape[1] on; before that seed_frames[:, t].
    * z: z_path[:, t] of z_path [R, nsteps, L] and no encoder, else the encoder on [x_enc, w_enc] with eps of Philox stream 0
      from index r0 * L; under z_prior its zargs are zeroed.
    * the uniforms: the rows' own of stream 1 from index r0 * D, or those of rows noise_rows (_NoiseRows).
    * the draw: free, under row t - S of the roll clamp [R, nsteps, D] -- or of a Constraints with voice counts, whose
      frames clv_bernoulli_sample_voices draws given their count --, or a particle filter's step (smc, an _Smc, which
      brings its own roll and S) followed by the ancestor gather of the rows' carried buffers.
    * dec_prev, what x_dec holds at the next step: 'sample'; 'enc_input', this step's x_enc (the decoder then lags the
      encoder by one frame: cl_vae's generator, and a re-decoding on its source's history); 'shared', x_dec IS x_enc
      (cl_vrnn's generator); or a history [R, nsteps, D] (history[:, t], clv_take_frame).
    temper None or (inv_T, Tz) (temper_args): a factor other than 1 takes one more launch each, the head's sigmoid then
    being sigmoid_temper's.
    t0: the Philox step of the chain's frame 0, a host value the noise kernels add to the device counter;
    the roll's row, the source frame and the seed hook keep counting from the chain's own frame 0."""

    def __init__(self, rows, w_enc, w_dec, nsteps, seed, temper, dec_prev, x_enc=None, x_dec=None, sources=None, z_path=None,
                 z_prior=False, seed_frames=None, noise_rows=None, r0=0, clamp=None, S=0, smc=None, t0=0):
        eng, R = rows.eng, rows.R
        D, L, d = eng.cfg['D'], eng.cfg['L'], eng.device
        new = lambda n: torch.zeros(R, n, dtype=torch.float32, device=d)
        self.rows, self.w_enc, self.w_dec, self.nsteps, self.seed, self.r0 = rows, w_enc, w_dec, nsteps, seed, r0
        self.inv_T, self.Tz = (1.0, 1.0) if temper is None else temper
        self.sources, self.z_path, self.z_prior, self.seed_frames = sources, z_path, z_prior, seed_frames
        self.history, self.dec_prev = (None, dec_prev) if isinstance(dec_prev, str) else (dec_prev, 'history')
        (self.clamp, self.voices), self.S, self.smc, self.t0 = clamp_parts(clamp), S, smc, int(t0)
        if z_path is None:
            self.x_enc, self.eps = new(D) if x_enc is None else x_enc, new(L)
        self.x_dec = self.x_enc if self.dec_prev == 'shared' else new(D) if x_dec is None else x_dec
        self.x_next, self.u = new(D), new(D)
        self.counter = torch.zeros(1, dtype=torch.int32, device=d)
        self.noise = _NoiseRows(noise_rows, R, D, d, first=r0 * D)
        if smc is not None:
            self.gather = ops.SmcGather(R, smc.P, smc.nsteps, smc.S, rows.carried(self.x_enc, self.x_next)
                                        + ([] if smc.wr is None else [smc.wr]))     # a particle's own key travels with it

    def frame(self):
        rows, R, T, c = self.rows, self.rows.R, self.nsteps, self.counter
        D, L = rows.eng.cfg['D'], rows.eng.cfg['L']
        if self.sources is not None:
            ops.take_frame(R, T, D, self.sources, c, self.x_enc)
        if self.z_path is None:
            rows.encode(self.x_enc, self.w_enc)
            ops.philox_normal(self.eps, R * L, self.seed, self.t0, 0, self.r0 * L, step_dev=c)
            if self.z_prior:
                rows.zargs[:R].zero_()
            if self.Tz != 1.0:
                ops.scale_temper(R * L, self.eps, self.Tz)
            ops.gauss_fwd(R, L, rows.zargs, self.eps, rows.z, L, None)
            if self.smc is not None and self.smc.ref is not None:      # a conditional sweep: the retained path's latents
                self.smc.pin_z(rows.z, c)
        else:
            ops.take_frame(R, T, L, self.z_path, c, rows.z)
        rows.decode(self.w_dec, rows.z, self.x_dec if rows.eng.cfg['use_x_prev'] else None,
                    ACT_SIGMOID if self.inv_T == 1.0 else ACT_NONE)
        if self.inv_T != 1.0:
            ops.sigmoid_temper(R * D, rows.xhat, self.inv_T)
        self.noise.draw(self.u, self.seed, c, self.t0)
        if self.smc is not None:
            self.smc.step(rows.xhat, self.u, c, self.x_next, self.gather)
        elif self.voices is not None:
            ops.bernoulli_sample_voices(R * D, D, T, self.S, rows.xhat, self.u, self.clamp, self.voices, c, self.x_next)
        elif self.clamp is None:
            ops.bernoulli_sample(R * D, rows.xhat, self.u, self.x_next)
        else:                   # the row of step counter - S: none for the seed steps and the bridge
            ops.bernoulli_sample_clamped(R * D, D, T, self.S, rows.xhat, self.u, self.clamp, c, self.x_next)
        if self.dec_prev == 'history':
            ops.take_frame(R, T, D, self.history, c, self.x_dec)        # history[:, t]: the previous frame of step t+1
        elif self.dec_prev != 'shared':
            self.x_dec.copy_(self.x_enc if self.dec_prev == 'enc_input' else self.x_next)
        if self.sources is None and self.z_path is None:
            self.x_enc.copy_(self.x_next)
        ops.i32_add(c, 1)

    def _seed(self, t):
        if t < self.seed_frames.shape[1]:
            self.x_enc.copy_(self.seed_frames[:, t])

    def run(self, nframes, use_graph, after=None):
        _replay(self.frame, nframes, use_graph, None if self.seed_frames is None else self._seed, after)

    def store(self, j, Xs, xhat_out=None, zout=None):
        """after a frame: its sample to Xs[:, j], its (tempered) probabilities to xhat_out[:, j], its latents (z_mean,
        z_log_var, z) to zout[:, :, j]"""
        rows, R, L = self.rows, self.rows.R, self.rows.eng.cfg['L']
        Xs[:, j].copy_(self.x_next)
        if xhat_out is not None:
            xhat_out[:, j].copy_(rows.xhat[:R])
        if zout is not None:
            zout[0, :, j].copy_(rows.zargs[:R, :L])
            zout[1, :, j].copy_(rows.zargs[:R, L:])
            zout[2, :, j].copy_(rows.z[:R])


class _Generate:
    """vary, decode_latents, generate_smc, generate_gibbs and the filter stream (filter_advance, filter_collapse) of both
    families, each written once.  What differs a family states itself
    (VaeGenerate, VrnnGenerate below) and the bodies here only ask for it:
    STATE_KIND                  its key in STATE_FIELDS, SEED_RANK, LSTM_FIELDS
    ROWS                        the rows of a frame chain: _VaeRows (at most the batch size) / _VrnnRows (any number)
    _persistent_ok()            do the model's shapes have a persistent kernel (reads cfg only)
    _family_flag()              the int after C in every persistent entry: use_x_prev / the gate activation
    _check_frames(**frames)     cl_vae reads frames as on / off: binary_frames; cl_vrnn takes any float: nothing
    _vary_fits(clamp, T, zout)  does a re-decoding fit the persistent kernel's 32-bit addressing
    _smc_seed(xs), _smc_cap()   how the filter's chain holds its seed rows xs; the most rows of a chunk (None: any)
    _filter_start(rows, xs, gen), _filter_read(rows, chain, t)   a filter stream's chain from seed rows or a carried
                                GenState, and the GenState its rows end on
    _vary_op, _decode_op        ops.vae_* / ops.vrnn_*: vary (with or without a zout) and decode
    _weights(encoder=True)      the weight arguments of those, in their order
    Every refusal (ValueError) comes before the first launch and before anything of the engine but cfg and device is read."""

    def vary(self, sources, w_enc, w_dec=None, x0=None, history='own', seed=0, clamp=None, temperature=1.0,
             z_temperature=1.0, persistent=True, use_graph=True, xhat_out=None, zout=None):
        """Re-decode sources [N, T, D]: per frame t the encoder on [sources[t], w_enc] (cl_vae: the z-encoder;
        cl_vrnn: the encoder step, from zero LSTM states), z = mean + exp(lv / 2) * Tz * eps, the decoder on [w_dec, xp, z]
        with xp the frame directly before t as in training: x0 (None: zeros) at t = 0, then the sample of frame t-1
        (history='own') or sources[t-1] ('source': the training forward pass; no effect without use_x_prev);
        x ~ Bernoulli(x_hat), then the roll clamp [N, T, D] (row t constrains frame t; no bridge).  w_dec=None: w_enc (a
        variation); another label: key transfer.  Noise as generate's (step = frame; cl_vrnn: with S = 0).  persistent=True
        (default where the shapes allow): ONE kernel, a workgroup per sequence (the VR instances of csrc/vae_generate.hip /
        csrc/generate.hip; any N); else the frame chain, captured once and replayed per frame (cl_vae: N <= batch size),
        reading its source frame through the device step counter.  cl_vrnn's kernel addresses in 32 bits: a roll of 2^32
        bytes or more, T * D * 4 >= 2^32 or a zout of 3 * 2^32 entries or more takes the chain.  Returns Xs [N, T, D];
        xhat_out [N, T, D] receives the unclamped (tempered) probabilities; zout [3, N, T, L] the latents
        (z_mean, z_log_var, z) of every frame.
        clamp may be a Constraints: without voices it is its roll; with voice counts every returned frame is
        drawn given its count on the frame chain -- persistent=True then takes the chain too: the persistent kernels do not
        carry the count.
        cl_vae reads frames as on / off: ValueError (binary_frames) for sources or an x0 with an entry other than 0 and 1,
        on both routes and before anything is launched.  cl_vrnn takes any float."""
        cfg, d = self.cfg, self.device
        D, L = cfg['D'], cfg['L']
        temper = temper_args(temperature, z_temperature)
        sources, w_enc, w_dec, x0, clamp, hist_source = vary_args(sources, w_enc, w_dec, x0, history, clamp, D, cfg['C'], d)
        self._check_frames(sources=sources, x0=x0)
        N, T = int(sources.shape[0]), int(sources.shape[1])
        if zout is not None:
            _zout_ok(zout, N, T, L)
        Xs = torch.zeros(N, T, D, dtype=torch.float32, device=d)
        if persistent and not isinstance(clamp, Constraints) and self._vary_fits(clamp, T, zout) and self._persistent_ok():
            self._vary_op(N, T, D, cfg['H'], L, cfg['C'], self._family_flag(), hist_source, seed, sources, x0, w_enc, w_dec,
                          *self._weights(), Xs, xhat_out, clamp=clamp, temper=temper, zout=zout)
            return Xs
        chain = _Chain(self.ROWS(self, N), w_enc, w_dec, T, seed, temper, 'enc_input' if hist_source else 'sample',
                       x_dec=None if x0 is None else x0.clone(), sources=sources, clamp=clamp)
        chain.run(T, use_graph, lambda t: chain.store(t, Xs, xhat_out, zout))
        return Xs

    def decode_latents(self, z, w_dec, x0=None, history='own', seed=0, clamp=None, temperature=1.0, noise_rows=None,
               persistent=True, use_graph=True, xhat_out=None):
        """Decode the latent path z [N, T, L]: vary's loop without its encoder.  Per frame t (cl_vrnn: from
        zero LSTM state) the decoder on [w_dec, xp, z[:, t]] with xp = x0 (None: zeros) at t = 0, then the sample of frame
        t-1 (history='own') or history[:, t-1] (an [N, T, D] array: teacher forcing; no effect without use_x_prev);
        x ~ Bernoulli(x_hat) with the uniforms of row noise_rows[n] (None: n), then the roll clamp [N, T, D].  No eps is
        drawn.  persistent=True (default where the shapes allow): ONE kernel, a workgroup per sequence (the ZG instances of
        csrc/vae_generate.hip / csrc/generate.hip); else the frame chain, captured once and replayed per frame (cl_vae:
        N <= batch size), reading z[:, t] and history[:, t-1] through the device step counter.  N*T*L or N*T*D of 2^32 or
        more takes the chain.  Returns Xs [N, T, D]; xhat_out [N, T, D] receives the unclamped (tempered) probabilities.
        clamp may be a Constraints: without voices it is its roll; with voice counts every returned frame is
        drawn given its count on the frame chain -- persistent=True then takes the chain too: the persistent kernels do not
        carry the count.
        cl_vae reads frames as on / off: ValueError (binary_frames) for an x0 or a given history with an entry other than
        0 and 1, on both routes and before anything is launched.  cl_vrnn takes any float."""
        cfg, d = self.cfg, self.device
        D, L = cfg['D'], cfg['L']
        inv_T = decode_temper(temperature)
        z, w_dec, x0, hist, clamp, noise_rows = decode_args(z, w_dec, x0, history, clamp, noise_rows, D, L, cfg['C'], d)
        self._check_frames(x0=x0, history=hist)
        N, T = int(z.shape[0]), int(z.shape[1])
        Xs = torch.zeros(N, T, D, dtype=torch.float32, device=d)
        if persistent and not isinstance(clamp, Constraints) and max(N * T * L, N * T * D) < 2 ** 32 \
                and self._persistent_ok():
            self._decode_op(N, T, D, cfg['H'], L, cfg['C'], self._family_flag(), seed, z, x0, hist, w_dec, noise_rows,
                            *self._weights(encoder=False), Xs, xhat_out, clamp=clamp, inv_T=inv_T)
            return Xs
        chain = _Chain(self.ROWS(self, N), None, w_dec, T, seed, None if inv_T == 1.0 else (inv_T, 1.0),
                       'sample' if hist is None else hist, x_dec=None if x0 is None else x0.clone(), z_path=z,
                       noise_rows=noise_rows, clamp=clamp)
        chain.run(T, use_graph, lambda t: chain.store(t, Xs, xhat_out))
        return Xs

    def generate_smc(self, x_seed, w, nsteps, clamp, particles, resample_threshold=0.5, n_out=1, seed=0, use_graph=True,
                     z_prior=False, chunk=None, w_prior=None, temperature=1.0, z_temperature=1.0):
        """Particle-filter sampling under the constraint roll clamp [N, nsteps, D]: melody m runs P =
        `particles` copies of the frame chain of generate(persistent=False) as global rows m*P + p, weighted by the
        probability of each returned frame's clamped notes and resampled (systematic, below an ESS of
        resample_threshold * P).  x_seed, w [N, C] device tensors.  cl_vae: x_seed [N, D], row t of the roll constrains
        frame t, and a chunk holds at most batch-size rows.  cl_vrnn: x_seed [N, S, D], row j of the roll constrains the
        sample of step S+j; the seed steps and the bridge carry no constraint and no weight; a chunk holds any number of
        rows.  `chunk`: at most that many melodies per pass; the Philox keys follow the global row, so the result does not
        depend on the chunking.  Returns SmcResult (Xs [N, n_out, nsteps, D]).
        clamp may be a Constraints with voice counts, with or without a roll: a counted frame's weight
        increment gains log P(count in range | forced notes), and log_evidence estimates log p(forced notes and every
        frame's count in its range | seed, w).
        w=None, w_prior=WPrior: every particle draws its own w from the prior and carries it with its state (cl_vrnn's seed
        steps run under it too, unweighted), so the filter targets p(w, free notes | seed, constraints);
        returns SmcKeyResult.
        temperature, z_temperature (temper_args): the filter runs on the TEMPERED model; its weights are the
        tempered probabilities of the clamped notes, so log_evidence estimates log p_T(constraints | seed, w), the evidence
        under the tempered model -- the trained model's only where both are 1."""
        cfg, d = self.cfg, self.device
        temper = temper_args(temperature, z_temperature)
        N, D = int(x_seed.shape[0]), cfg['D']
        clamp = smc_args(clamp, particles, resample_threshold, n_out, N, nsteps, D, d)
        P, tau, nsteps = int(particles), float(resample_threshold), int(nsteps)
        x_seed = x_seed.to(dtype=torch.float32, device=d)
        w, prior = smc_label_args(w, w_prior, N, cfg['C'], d)
        S = seed_steps(self.STATE_KIND, x_seed)

        def run_chunk(m0, m1):
            if prior is None:
                wr = w[m0:m1].repeat_interleave(P, 0).contiguous()
            else:
                wr = torch.zeros((m1 - m0) * P, cfg['C'], dtype=torch.float32, device=d)
                prior.init_rows(m0, m1, P, seed, wr)
            smc = _Smc(m1 - m0, P, nsteps, S, D, tau, seed, m0, clamp[m0:m1], d, wr=None if prior is None else wr)
            xs = x_seed[m0:m1].repeat_interleave(P, 0)          # seeds and labels per particle row, m0 * P the first global row
            _Chain(self.ROWS(self, smc.R), wr, wr, nsteps, seed, temper, z_prior=z_prior, r0=m0 * P, smc=smc,
                   **self._smc_seed(xs)).run(S + nsteps, use_graph)
            return smc

        return _smc_drive(_smc_chunks(N, P, self._smc_cap(), chunk), run_chunk, N, nsteps, D, int(n_out), d,
                          C=None if prior is None else cfg['C'])


    def generate_gibbs(self, x_seed, w, nsteps, clamp, particles, sweeps, resample_threshold=0.5, seed=0, use_graph=True,
                       z_prior=False, chunk=None, temperature=1.0, z_temperature=1.0):
        """Particle Gibbs under the constraints clamp: K = `sweeps` sweeps of generate_smc's filter with P =
        `particles` particles, x_seed, w [N, C], clamp (a roll or a Constraints), resample_threshold, chunk and the
        temperatures as there.  Sweep 0 IS that filter with n_out = 1 under `seed`, bit for bit.  Sweep s >= 1 runs the
        whole chain under the key gibbs_seed(seed, s) with particle 0 of every melody (row m * P) pinned to the path the
        sweep before retained -- its latents at every chain step, its frames, and cl_vrnn's bridge sample -- and with
        conditional multinomial resampling (the pinned particle always survives; every other particle draws its own
        uniform of the stream trainer.GIBBS_STREAM); the sweep's path is then drawn from its final weights and retained.
        A conditional sweep leaves p(free notes, z | seed, w, all constraints) invariant for any P >= 2, so the path after
        K sweeps approaches the posterior as K grows, at a fixed small P; with P = 1 every sweep returns sweep 0's path.
        There is no ancestor sampling: the early frames of a long piece renew slowly, and `renewed` shows it.
        Returns GibbsResult: Xs [N, K, nsteps, D], the path after every sweep; log_evidence [N, K] -- ONLY column 0 is an
        unbiased estimate of the evidence, the log Z of a conditional sweep is conditioned on the retained path --;
        renewed [N, K, nsteps] bool; z [N, S + nsteps, L], the last path's latents.  The Philox streams follow the global
        row and melody, so the result does not depend on `chunk`."""
        cfg, d = self.cfg, self.device
        temper = temper_args(temperature, z_temperature)
        K = gibbs_args(sweeps)
        N, D, L = int(x_seed.shape[0]), cfg['D'], cfg['L']
        clamp = smc_args(clamp, particles, resample_threshold, 1, N, nsteps, D, d)
        P, tau, nsteps = int(particles), float(resample_threshold), int(nsteps)
        x_seed = x_seed.to(dtype=torch.float32, device=d)
        w = w.to(dtype=torch.float32, device=d)
        S = seed_steps(self.STATE_KIND, x_seed)
        f = dict(device=d)
        out = GibbsResult(torch.zeros(N, K, nsteps, D, dtype=torch.float32, **f), torch.zeros(N, K, dtype=torch.float64, **f),
                          torch.ones(N, K, nsteps, dtype=torch.bool, **f), torch.zeros(N, S + nsteps, L, dtype=torch.float32, **f))
        for m0, m1 in _smc_chunks(N, P, self._smc_cap(), chunk):
            G = m1 - m0
            wr = w[m0:m1].repeat_interleave(P, 0).contiguous()
            path = _Path(G, nsteps, S, D, L, d)
            Xs = torch.zeros(G, 1, nsteps, D, dtype=torch.float32, **f)
            renewed = torch.zeros(G, nsteps, dtype=torch.uint8, **f)
            for s in range(K):
                key = gibbs_seed(seed, s)
                smc = _GibbsSmc(G, P, nsteps, S, D, L, tau, key, m0, clamp[m0:m1], d, ref=path if s else None)
                xs = x_seed[m0:m1].repeat_interleave(P, 0)      # anew per sweep: cl_vae's chain writes into its seed rows
                rows = self.ROWS(self, smc.R)
                chain = _Chain(rows, wr, wr, nsteps, key, temper, z_prior=z_prior, r0=m0 * P, smc=smc, **self._smc_seed(xs))
                chain.run(S + nsteps, use_graph, lambda t: smc.record(t, rows.z, chain.x_next))
                smc.retain(path, Xs, renewed)
                out.Xs[m0:m1, s].copy_(Xs[:, 0])
                out.log_evidence[m0:m1, s].copy_(smc.logZ)
                if s:
                    out.renewed[m0:m1, s].copy_(renewed != 0)
            out.z[m0:m1].copy_(path.z)
        return out

    def filter_advance(self, state, x_seed, w, clamp_chunk, particles, resample_threshold=0.5, seed=0, z_prior=False,
                       temperature=1.0, z_temperature=1.0, use_graph=True):
        """The next n frames of a filter stream: generate_smc's filter stopped after any frame and continued.
        state None starts the stream on x_seed (cl_vrnn [N, S, D]: the S seed frames and the bridge are teacher-forced,
        unweighted, as in generate_smc; cl_vae [N, D]); a FilterState continues it (x_seed None; the state is consumed).
        w [N, C]; clamp_chunk: the roll uint8 [N, n, D] of these frames, or a Constraints with voice counts for them; n is
        its length.  Runs n filter steps with the launches of generate_smc -- the Philox step of local frame c is t + c for
        the eps and u of the chain and for the resampling uniform; logW, logZ and nres continue -- and then commits: per
        melody the frames of the longest prefix of its pending steps through which every surviving lineage passes by one
        row are final, are returned and leave the pending store.  However a piece is cut into chunks, the rows' states,
        logW, logZ, ess, the ancestors and the frames are those of one generate_smc call, bit for bit.  Every melody's
        N * P rows run together: cl_vae needs N * P <= the batch size (ValueError).  Returns FilterEmit."""
        cfg, d, kind = self.cfg, self.device, self.STATE_KIND
        D = cfg['D']
        temper = temper_args(temperature, z_temperature)
        if (state is None) == (x_seed is None):
            raise ValueError("give x_seed to start a filter stream or a FilterState to continue one, not both")
        w = device_f32(w, d)
        if w.dim() != 2 or w.shape[0] < 1 or w.shape[1] != cfg['C']:
            raise ValueError("w must be [N, %d] with N >= 1, got shape %s" % (cfg['C'], tuple(w.shape)))
        N, n = int(w.shape[0]), chunk_frames(clamp_chunk)
        clamp = smc_args(clamp_chunk, particles, resample_threshold, 1, N, n, D, d)
        P, tau = int(particles), float(resample_threshold)
        R = N * P
        if self._smc_cap() is not None and R > self._smc_cap():
            raise ValueError("%d melodies x %d particles exceed the engine's batch size %d: a filter stream runs all of "
                             "its rows together" % (N, P, self._smc_cap()))
        if state is None:
            xs = device_f32(x_seed, d)
            if xs.dim() != SEED_RANK[kind] or xs.shape[0] != N or xs.shape[-1] != D:
                raise ValueError("x_seed must be %s, got shape %s" % ("[%d, S, %d]" % (N, D) if SEED_RANK[kind] == 3 else
                                                                     "[%d, %d]" % (N, D), tuple(xs.shape)))
            S, t0 = seed_steps(kind, xs), resume_args(None, kind, None, None, seed_steps(kind, xs) + n)
            xs = xs.repeat_interleave(P, 0)
        else:
            if not isinstance(state, FilterState):
                raise ValueError("state must be a FilterState, got %r" % type(state).__name__)
            if state.P != P or state.D != D:
                raise ValueError("the state holds %d particles of %d notes, the call %d of %d" % (state.P, state.D, P, D))
            S, xs, t0 = 0, None, resume_args(state.gen, kind, R, state_widths(kind, cfg), n)
        wr = w.repeat_interleave(P, 0).contiguous()
        smc = _StreamSmc(N, P, n, S, D, tau, seed, clamp, d, t0=t0, state=state)
        rows = self.ROWS(self, R)
        chain = _Chain(rows, wr, wr, n, seed, temper, z_prior=z_prior, smc=smc, t0=t0,
                       **self._filter_start(rows, xs, None if state is None else state.gen))
        chain.run(S + n, use_graph)
        gen = self._filter_read(rows, chain, t0 + S + n)
        if state is None:
            state, longest = FilterState.fresh(gen, P, D, n, smc.logW, smc.logZ, smc.nres), 0
        else:
            state.gen, longest = gen, int(state.pending().max())
        room = longest + n
        state.reserve(room)
        frames = torch.zeros(N, room, D, dtype=torch.uint8, device=d)
        ncommit = torch.zeros(N, dtype=torch.int32, device=d)
        ops.smc_commit(N, P, D, n, smc.anc, smc.hist, state.cap, state.pend_anc, state.pend_hist, state.head, state.len, room,
                       ncommit, frames)
        counts = ncommit.cpu().numpy().astype(np.int64)
        if counts.min() < 0:
            raise RuntimeError("clv_smc_commit: the pending store of melody %d is inconsistent" % int(counts.argmin()))
        return FilterEmit(state, frames[:, :int(counts.max())], counts, smc.ess, np.full(N, -1, np.int64))

    def filter_collapse(self, state, index=None, seed=0, final=False):
        """Force the issue for the melodies `index` (None: all) of a filter stream: draw one particle per
        melody from the current weights -- by systematic_pick with n = 1 and a Philox uniform of stream
        trainer.COLLAPSE_STREAM at step state.t, index m --, return its whole pending lineage, make all P rows of the melody
        copies of that particle (clv_smc_gather fed the pick as every row's ancestor), set logW = -log P and empty the
        melody's pending store; logZ stays (after a collapse it is no longer the unbiased estimate), collapses[m] counts.
        final=True is the stream's end instead: the draw of clv_smc_backtrack with n_out = 1 (SMC_STREAM, step state.t), for
        every melody, and nothing of the state changes.  The state is consumed.  Returns FilterEmit (ess None)."""
        if not isinstance(state, FilterState):
            raise ValueError("state must be a FilterState, got %r" % type(state).__name__)
        N, P, D, d = state.N, state.P, state.D, state.device
        which = np.ones(N, bool)
        if index is not None:
            if final:
                raise ValueError("the final draw takes every melody")
            idx = np.asarray(index)
            if idx.dtype == np.bool_ and idx.shape == (N,):
                which = idx.copy()
            elif idx.ndim == 1 and np.issubdtype(idx.dtype, np.integer) and (not idx.size or (idx.min() >= 0 and idx.max() < N)):
                which = np.zeros(N, bool)
                which[idx] = True
            else:
                raise ValueError("index must be melodies in [0, %d) or a boolean mask [%d], got %r" % (N, N, index))
        lens = state.pending()
        room = max(int(lens.max()), 1)
        i32 = dict(dtype=torch.int32, device=d)
        pick_of = torch.as_tensor(which.astype(np.int32), device=d)
        picks, flag = torch.full((N,), -1, **i32), torch.zeros(N, **i32)
        anc_row = torch.arange(N * P, **i32)
        frames = torch.zeros(N, room, D, dtype=torch.uint8, device=d)
        ops.smc_collapse(N, P, D, seed, 0, state.t, final, pick_of, state.logW, state.cap, state.pend_anc, state.pend_hist,
                         state.head, state.len, room, picks, frames, anc_row, flag)
        if not final:
            ops.SmcGather(N * P, P, 1, 0, state.buffers())(anc_row.view(1, -1), flag, torch.zeros(1, **i32))
            state.collapses += flag
        picks = picks.cpu().numpy().astype(np.int64)
        if (picks[which] < 0).any():
            raise RuntimeError("clv_smc_collapse: the pending store of melody %d is inconsistent"
                               % int(np.nonzero(which & (picks < 0))[0][0]))
        counts = np.where(which, lens, 0)
        return FilterEmit(state, frames[:, :int(counts.max())], counts, None, picks)


class VaeGenerate(_Generate):
    STATE_KIND = 'cl_vae'
    ROWS = _VaeRows
    _check_frames = staticmethod(binary_frames)
    _vary_op, _decode_op = staticmethod(ops.vae_vary), staticmethod(ops.vae_decode)

    def _persistent_ok(self):
        cfg = self.cfg
        return cfg['H'] > 0 and ops.vae_generate_supported(cfg['D'], cfg['H'], cfg['L'], cfg['C'])

    def _family_flag(self):
        return self.cfg['use_x_prev']

    def _vary_fits(self, clamp, T, zout):
        return True

    def _smc_seed(self, xs):
        """the seed frame is both the encoder's input and the decoder's previous frame of step 0"""
        return dict(dec_prev='enc_input', x_enc=xs, x_dec=xs.clone())

    def _smc_cap(self):
        return self.B

    def _filter_start(self, rows, xs, gen):
        """a filter stream's chain arguments: from the seed rows xs as generate_smc's, or from a state's last two frames"""
        return self._smc_seed(xs) if gen is None else dict(dec_prev='enc_input', x_enc=gen.x_in.clone(), x_dec=gen.hist.clone())

    def _filter_read(self, rows, chain, t):
        return GenState('cl_vae', None, t, rows=torch.stack([chain.x_enc, chain.x_dec], 1).contiguous())._sampled()

    def _weights(self, encoder=True):
        """the persistent kernels' weight arguments in the order ops.vae_* take them: the encoder half (vae_decode takes
        none), the decoder half, the head"""
        p = self.P.p
        enc = (p('h/kernel'), p('h/bias'), p('zargs/kernel'), p('zargs/bias')) if encoder else ()
        return enc + (p('decoder_h/kernel'), p('decoder_h/bias'), p('x_decoded_mean/kernel'), p('x_decoded_mean/bias'))

    def generate(self, x_seed, w, nsteps, seed=0, use_graph=True, z_prior=False, persistent=True, xhat_out=None, clamp=None,
                 temperature=1.0, z_temperature=1.0, state=None, return_state=False):
        """N independent sequences of `nsteps` frames on the device: the frame loop of cl_vae/model.py:28-41
        (z-encoder on the last frame, z ~ N(mean, exp(lv)) or N(0, 1), decoder on (w, z, frame before last),
        x ~ Bernoulli); eps and u come from the Philox streams 0 / 1 at step = frame index.  x_seed [N,D], w [N,C] device
        tensors.  persistent=True (default where the shapes allow): the whole loop is ONE kernel, a workgroup per
        sequence (csrc/vae_generate.hip; any N); otherwise the layer chain captured once as a hipGraph and replayed per
        frame (N <= batch size).  Same noise, same samples either way.  clamp: constraint roll [N,nsteps,D] (clamp_roll;
        row t constrains frame t, which is then fed back like a sampled one: clamped ancestral sampling).
        clamp may be a Constraints: without voices it is its roll; with voice counts every returned frame is
        drawn given its count on the frame chain -- persistent=True then takes the chain too: the persistent kernels do not
        carry the count.
        temperature, z_temperature (temper_args): sample from the tempered model, x_hat = sigmoid(logit /
        temperature) and z = mean + exp(lv / 2) * z_temperature * eps, with the same Philox draws; xhat_out then holds the
        tempered probabilities.  Both 1.0 (default): exactly the untempered launches.
        state, return_state: continue from a GenState (x_seed is then None: the state holds the last two
        frames) with the Philox steps counted on from state.t, and / or return (Xs, GenState after the last frame).  A
        piece generated in several such calls is bit for bit the piece of one call; the state is the same on both routes
        and is not written.  Neither given (default): exactly the launches above -- the plain, clamped or tempered instance;
        with either, the ST instance (ops.vae_generate from / to a state).
        Frames are read as on / off: ValueError (binary_frames) for an x_seed, or a state not returned by a sampler, with
        an entry other than 0 and 1, on both routes and before anything is launched."""
        cfg, d = self.cfg, self.device
        D, f = cfg['D'], dict(dtype=torch.float32, device=d)
        resume = state is not None or return_state
        if resume:
            temper, nsteps = temper_args(temperature, z_temperature), int(nsteps)
            if state is None:
                state = GenState.fresh('cl_vae', cfg, d, seed_frame=x_seed)
            elif x_seed is not None:
                raise ValueError("a cl_vae state holds its last two frames: give no x_seed with it")
            N = int(w.shape[0])
            t0 = resume_args(state, 'cl_vae', N, state_widths('cl_vae', cfg), nsteps)
            if nsteps < 1:
                raise ValueError("nsteps must be >= 1, got %r" % (nsteps,))
            clamp = clamp_roll(clamp, N, nsteps, D, d)
            if not state.binary:                   # a seed frame, from_numpy, built by hand: one reduction over both rows
                binary_frames(**{'x_seed' if x_seed is not None else 'the state (x_in, hist)': state.rows})
            x_in, hist = state.x_in, state.hist
        else:
            N, t0 = int(x_seed.shape[0]), 0
            clamp = clamp_roll(clamp, N, nsteps, D, d)
            temper = temper_args(temperature, z_temperature)
            binary_frames(x_seed=x_seed)
            x_in = hist = x_seed.to(**f).contiguous()
        w = w.to(**f).contiguous()
        if not (persistent and not isinstance(clamp, Constraints) and self._persistent_ok()):
            return self._generate_frames(x_in, hist, w, nsteps, seed, use_graph, z_prior, clamp, temper, t0, return_state)
        Xs = torch.zeros(N, nsteps, D, **f)
        head = (N, nsteps, D, cfg['H'], cfg['L'], cfg['C'], cfg['use_x_prev'], z_prior, seed)
        out = torch.empty(N, 2, D, **f) if return_state else None
        from_state = dict(t0=t0, state_in=state.rows, state_out=out) if resume else {}     # the state stands for the seed frame
        ops.vae_generate(*head, None if resume else x_in, w, *self._weights(), Xs, xhat_out, clamp=clamp, temper=temper,
                         **from_state)
        return (Xs, GenState('cl_vae', None, t0 + nsteps, rows=out)._sampled()) if return_state else Xs

    def _generate_frames(self, x_in, hist, w, nsteps, seed, use_graph, z_prior, clamp, temper, t0=0, return_state=False):
        """generate on the frame chain, started from the last frame x_in and the one before it, hist (a fresh start: the seed
        frame twice, t0 = 0); with return_state the two frames it ends on go back as a state"""
        Xs = torch.zeros(w.shape[0], nsteps, self.cfg['D'], dtype=torch.float32, device=self.device)
        chain = _Chain(_VaeRows(self, int(w.shape[0])), w, w, nsteps, seed, temper, 'enc_input', x_enc=x_in.clone(),
                       x_dec=hist.clone(), z_prior=z_prior, clamp=clamp, t0=t0)
        chain.run(nsteps, use_graph, lambda t: chain.store(t, Xs))
        if not return_state:
            return Xs
        rows = torch.stack([chain.x_enc, chain.x_dec], 1).contiguous()
        return Xs, GenState('cl_vae', None, t0 + nsteps, rows=rows)._sampled()


class VrnnGenerate(_Generate):
    STATE_KIND = 'cl_vrnn'
    ROWS = _VrnnRows
    _check_frames = staticmethod(lambda **frames: None)
    _vary_op, _decode_op = staticmethod(ops.vrnn_vary), staticmethod(ops.vrnn_decode)

    def _persistent_ok(self):
        cfg = self.cfg
        return ops.vrnn_generate_supported(cfg['D'], cfg['H'], cfg['L'], cfg['C'])

    def _family_flag(self):
        return self.gate_act

    def _vary_fits(self, clamp, T, zout):
        """the persistent kernel addresses the roll, a sequence's frames and the latents in 32 bits"""
        return not ((clamp is not None and clamp.numel() >= 2 ** 32) or T * self.cfg['D'] * 4 >= 2 ** 32
                    or (zout is not None and zout.numel() >= 3 * 2 ** 32))

    def _smc_seed(self, xs):
        """S teacher-forced steps on one frame slot that the encoder and the decoder share"""
        return dict(dec_prev='shared', seed_frames=xs)

    def _smc_cap(self):
        return None

    def _filter_start(self, rows, xs, gen):
        """a filter stream's chain arguments: from the seed rows xs as generate_smc's, or the rows' LSTM states and the
        shared frame slot from a state (no seed step then)"""
        if gen is None:
            return self._smc_seed(xs)
        for k in LSTM_FIELDS['cl_vrnn']:
            rows.st[k].copy_(gen[k])
        return dict(dec_prev='shared', x_enc=gen.x.clone())

    def _filter_read(self, rows, chain, t):
        tensors = {k: rows.st[k].clone() for k in LSTM_FIELDS['cl_vrnn']}
        tensors['x'] = chain.x_enc.clone()
        return GenState('cl_vrnn', tensors, t)

    # -- stateful single-step inference (the reference's stateful batch-1 sub-models,
    #    cl_vrnn/model.py:116-162; here for any batch of independent sequences) -------------
    def new_state(self, B):
        d, H = self.device, self.cfg['H']
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=d)
        return dict(B=B, h_enc=z(B, H), c_enc=z(B, H), h_dec=z(B, H), c_dec=z(B, H), gates=z(B, 4 * H),
                    hs=z(B, H), zargs=z(B, 2 * self.cfg['L']), xhat=z(B, self.cfg['D']))

    def encode_w(self, X, B):
        """hW -> Wargs for B windows [B, T*D] (:174-181) -> self.wargs[:B]"""
        cfg, P = self.cfg, self.P
        D, T, C1 = cfg['D'], cfg['T'], cfg['C'] - 1
        ops.gemm(X, P.p('hW/kernel'), self.hW, B, D, T * D, bias=P.p('hW/bias'), act=ACT_RELU, ws=self.ws)
        ops.gemm(self.hW, P.p('Wargs/kernel'), self.wargs, B, 2 * C1, D, bias=P.p('Wargs/bias'), ws=self.ws)

    def _lstm_step(self, name, st, hkey, ckey):
        ops.lstm_seq_fwd(st['B'], 1, st['gates'], None, self.P.p(name + '/recurrent_kernel'), st['hs'], None, None,
                         h0=st[hkey], c0=st[ckey], hT=st[hkey], cT=st[ckey], gate_act=self.gate_act, H=self.cfg['H'])

    def enc_step(self, x, w, st, rec_name='encoder_h'):
        """one encoder-LSTM step on [x_t, w] + the Z heads -> st['zargs'] = [z_mean | z_log_var]"""
        cfg, P, B = self.cfg, self.P, st['B']
        D, H, L, Cn = cfg['D'], cfg['H'], cfg['L'], cfg['C']
        g, ws = ops.gemm, self.ws
        g(x, P.p(rec_name + '/kernel'), st['gates'], B, 4 * H, D, ws=ws)
        g(w, P.rows(P.params, rec_name + '/kernel', D), st['gates'], B, 4 * H, Cn, beta=1.0, bias=P.p(rec_name + '/bias'),
          ws=ws)
        self._lstm_step(rec_name, st, 'h_enc', 'c_enc')
        g(st['hs'], P.p('Zargs/kernel'), st['zargs'], B, 2 * L, H, bias=P.p('Zargs/bias'), ws=ws)

    def dec_step(self, z, xp, w, st, act=ACT_SIGMOID):
        """one decoder-LSTM step on [x_{t-1}, z_t, w] + sigmoid head -> st['xhat'] (act=ACT_NONE: the head's pre-activations)"""
        cfg, P, B = self.cfg, self.P, st['B']
        D, H, L, Cn = cfg['D'], cfg['H'], cfg['L'], cfg['C']
        g, ws, off = ops.gemm, self.ws, self.off
        if cfg['use_x_prev']:
            g(xp, P.p('decoder_h/kernel'), st['gates'], B, 4 * H, D, ws=ws)
        g(z, P.rows(P.params, 'decoder_h/kernel', off), st['gates'], B, 4 * H, L,
          beta=1.0 if cfg['use_x_prev'] else 0.0, ws=ws)
        g(w, P.rows(P.params, 'decoder_h/kernel', off + L), st['gates'], B, 4 * H, Cn, beta=1.0,
          bias=P.p('decoder_h/bias'), ws=ws)     # three tiny GEMMs: batch-1 sampling is launch-bound, not flop-bound
        self._lstm_step('decoder_h', st, 'h_dec', 'c_dec')
        g(st['hs'], P.p('X_decoded_mean/kernel'), st['xhat'], B, D, H, bias=P.p('X_decoded_mean/bias'),
          act=act, ws=ws)

    def _weights(self, encoder=True):
        """the persistent kernels' weight arguments in the order ops.vrnn_* take them: the encoder half (vrnn_decode takes
        none), the decoder half, the head"""
        p, L, off = self.P.p, self.cfg['L'], self.off
        rows = lambda name, r: self.P.rows(self.P.params, name, r)
        enc = (p('encoder_h/kernel'), rows('encoder_h/kernel', self.cfg['D']), p('encoder_h/bias'),
               p('encoder_h/recurrent_kernel'), p('Zargs/kernel'), p('Zargs/bias')) if encoder else ()
        return enc + (p('decoder_h/kernel') if self.cfg['use_x_prev'] else None, rows('decoder_h/kernel', off),
                      rows('decoder_h/kernel', off + L), p('decoder_h/bias'), p('decoder_h/recurrent_kernel'),
                      p('X_decoded_mean/kernel'), p('X_decoded_mean/bias'))

    def generate(self, x_seed, w, nsteps, seed=0, use_graph=True, z_prior=False, persistent=True, xhat_out=None, clamp=None,
                 temperature=1.0, z_temperature=1.0, state=None, return_state=False):
        """Autoregressive generation of N independent sequences on the device (the hot loop of cl_vrnn/model.py:47-59,
        noise from Philox instead of np.random): x_seed [N,S,D] device tensor (teacher-forced frames, S may be 0), w [N,C];
        returns Xs [N,nsteps,D].  One frame = encoder step -> z ~ N(mean, exp(lv)) -> decoder step -> x ~ Bernoulli(x_hat).
        persistent=True (default where the shapes allow): the whole frame loop is ONE kernel, a workgroup per sequence
        (csrc/generate.hip); otherwise the frame chain, captured once and replayed per frame with no host synchronisation.
        Same Philox noise either way.
        xhat_out [N,S+nsteps,D] (persistent path only) receives every frame's note probabilities.
        clamp: constraint roll [N,nsteps,D] (engine_generate.clamp_roll): row j constrains the returned frame Xs[:, j],
        drawn at step S+j; the bridge sample of step S-1 stays free (clamped ancestral sampling).  The
        persistent kernel addresses the roll in 32 bits: a roll of 2^32 bytes or more takes the frame chain.
        clamp may be a Constraints: without voices it is its roll; with voice counts every returned frame is
        drawn given its count on the frame chain -- persistent=True then takes the chain too: the persistent kernels do not
        carry the count.
        temperature, z_temperature (temper_args): sample from the tempered model, x_hat = sigmoid(logit /
        temperature) and z = mean + exp(lv / 2) * z_temperature * eps, with the same Philox draws (runs that differ only in
        the temperature share their uniforms); xhat_out then holds the tempered probabilities.  Both 1.0 (default):
        exactly the untempered launches.
        state, return_state: start both LSTMs and the first input from a GenState instead of zero, with the
        Philox steps counted on from state.t, and / or return (Xs, GenState after the last frame).  With a state x_seed
        may be None or [N,0,D] (the free run goes on from the state's x) or hold more teacher-forced frames.  nsteps = 0
        with seed frames primes a state: its x is then the bridge sample.  A piece generated in several such calls is bit
        for bit the piece of one call; the state is the same on both routes and is not written.  Neither given (default):
        exactly the launches above -- the plain, clamped or tempered instance; with either, the ST instances
        (ops.vrnn_generate from / to a state; they need D = H: one row width)."""
        cfg = self.cfg
        temper = temper_args(temperature, z_temperature)
        resume = state is not None or return_state
        if x_seed is None:
            if state is None:
                raise ValueError("give x_seed or a state")
            x_seed = torch.zeros(state.N, 0, cfg['D'], dtype=torch.float32, device=self.device)
        N, S, nsteps = int(x_seed.shape[0]), int(x_seed.shape[1]), int(nsteps)
        t0 = resume_args(state, 'cl_vrnn', N, state_widths('cl_vrnn', cfg), S + nsteps) if resume else 0
        if resume and S + nsteps < 1:
            raise ValueError("nothing to run: no seed frame and nsteps = 0")
        clamp = clamp_roll(clamp, N, nsteps, cfg['D'], self.device)
        if clamp is not None and nsteps == 0:
            clamp = None                # nothing is returned, so nothing is constrained
        if clamp is not None and (isinstance(clamp, Constraints) or clamp.numel() >= 2 ** 32):
            persistent = False          # voice counts run on the frame chain; so does a roll past 32-bit addressing
        if resume:
            x_seed = x_seed.to(dtype=torch.float32, device=self.device)
            w = w.to(dtype=torch.float32, device=self.device)
        x_seed, w = x_seed.contiguous(), w.contiguous()
        if not (persistent and self._persistent_ok()):
            return self._generate_frames(x_seed, w, nsteps, seed, use_graph, z_prior, clamp, temper, t0, state, return_state)
        Xs = torch.zeros(N, nsteps, cfg['D'], dtype=torch.float32, device=self.device)
        head = (N, S, nsteps, cfg['D'], cfg['H'], cfg['L'], cfg['C'], self.gate_act, z_prior, seed, x_seed if S else None, w,
                *self._weights())
        out = torch.empty(N, 5, cfg['D'], dtype=torch.float32, device=self.device) if return_state else None
        from_state = dict(t0=t0, state_in=None if state is None else state.rows, state_out=out) if resume else {}
        ops.vrnn_generate(*head, Xs if nsteps else None, xhat_out, clamp=clamp, temper=temper, **from_state)
        return (Xs, GenState('cl_vrnn', None, t0 + S + nsteps, rows=out)) if return_state else Xs

    def _generate_frames(self, x_seed, w, nsteps, seed=0, use_graph=True, z_prior=False, clamp=None, temper=None, t0=0,
                         state=None, return_state=False):
        """generate on the frame chain: S seed steps, then nsteps returned frames.  With a state the rows' LSTM states and
        the first input are taken from it (else zero, t0 = 0); with return_state they are read back after the last frame."""
        N, S = int(x_seed.shape[0]), int(x_seed.shape[1])
        Xs = torch.zeros(N, nsteps, self.cfg['D'], dtype=torch.float32, device=self.device)
        rows = _VrnnRows(self, N)
        chain = _Chain(rows, w, w, nsteps, seed, temper, 'shared', z_prior=z_prior, seed_frames=x_seed, clamp=clamp, S=S,
                       t0=t0)
        if state is not None:
            for k in LSTM_FIELDS['cl_vrnn']:
                rows.st[k].copy_(state[k])
            chain.x_enc.copy_(state.x)

        def after(t):
            if t >= S:
                chain.store(t - S, Xs)

        chain.run(S + nsteps, use_graph, after)
        if not return_state:
            return Xs
        tensors = {k: rows.st[k].clone() for k in LSTM_FIELDS['cl_vrnn']}
        tensors['x'] = chain.x_enc.clone()
        return Xs, GenState('cl_vrnn', tensors, t0 + S + nsteps)
