"""Resumable generation: a piece generated a chunk at a time on the device.

generate_samples_device(state=..., return_state=True) of both families carries the samplers' state from call to call; this
module is the convenient face of it.  A Stream holds the state of N pieces and advances them by any number of frames per
call -- endless generation, a live accompaniment a bar at a time, a roll that arrives chunk by chunk.  The label, the roll
and the temperatures may change between calls: modulate() changes the key on the way.  fork() branches: one prefix, several
continuations.  However a piece is cut into chunks, its frames are bit for bit those of one call.

A FilterStream does the same for the particle filter of generate_samples_device(particles=P): it carries the
particles' state, weights and ancestry, and hands out a frame as soon as every surviving lineage agrees on it."""
import numpy as np

from .engine_generate import GenState, temper_args


def _family(model):
    kind = getattr(model.engine, 'STATE_KIND', None)
    if kind == 'cl_vrnn':
        from .cl_vrnn.model import generate_samples_device
        return kind, generate_samples_device, 'z_prior'
    if kind == 'cl_vae':
        from .cl_vae.model import generate_samples_device
        return kind, generate_samples_device, 'use_z_prior'
    raise ValueError("model must be a cl_vrnn or cl_vae model, got %r" % type(model).__name__)


class Stream:
    """N pieces that go on where they stopped.  Stream(model, x_seeds, w, seed=0, z_prior=False) primes on the seed: cl_vrnn
    teacher-forces x_seeds [N, S, 88] (S = 0: a cold start) and keeps the bridge sample as the next input, cl_vae starts
    with x_seeds [N, 88] as the last frame and the one before it.  w [N, C] is the label until advance() replaces it.
    temperature, z_temperature: those of the priming (cl_vrnn with seed frames: the latents of the seed steps and the bridge
    sample are drawn under them, as one call draws them under its own).  A first advance() under other temperatures primes
    again under its own, so that seed + first call is the one call whatever the constructor was given; a fork() taken before
    it keeps the priming it was taken from.
    .t: the Philox step of the next frame; .state: the GenState (a call never writes it); .w: the current label."""

    def __init__(self, model, x_seeds, w, seed=0, z_prior=False, temperature=1.0, z_temperature=1.0):
        self.kind, self._gen, zname = _family(model)
        self.model, self.seed, self._zkw = model, int(seed), {zname: bool(z_prior)}
        self._pending = None            # cl_vrnn seed frames, their label and the priming's temperatures, until the first advance
        cfg, d = model.engine.cfg, model.engine.device
        self.w = np.asarray(w, np.float64)
        x = np.asarray(x_seeds)
        if self.kind == 'cl_vae':
            self.state = GenState.fresh('cl_vae', cfg, d, seed_frame=x)
        elif x.ndim != 3 or x.shape[0] < 1 or x.shape[2] != cfg['D']:
            raise ValueError("x_seeds must be [N, S, %d] with N >= 1, got shape %s" % (cfg['D'], x.shape))
        elif x.shape[1] == 0:
            self.state = GenState.fresh('cl_vrnn', cfg, d, N=x.shape[0])
        else:
            self._pending = (x, self.w, (float(temperature), float(z_temperature)))
            self._prime(temperature, z_temperature)
        if self.w.shape != (self.state.N, cfg['C']):
            raise ValueError("w must have shape %s, got %s" % ((self.state.N, cfg['C']), self.w.shape))

    def _prime(self, temperature, z_temperature):
        x, w0, _ = self._pending
        _, self.state = self._gen(self.model, x, 0, w0, seed=self.seed, return_state=True, temperature=temperature,
                                  z_temperature=z_temperature, **self._zkw)

    @property
    def t(self):
        return self.state.t

    @property
    def N(self):
        return self.state.N

    def advance(self, nsteps, w=None, clamp=None, temperature=1.0, z_temperature=1.0):
        """the next nsteps frames [N, nsteps, 88] (float64).  w [N, C] replaces the label from this call on; clamp: a roll
        uint8 [N, nsteps, 88] for these frames (row j constrains frame j of this call), or a Constraints with voice counts for
        them; temperature, z_temperature as in
        generate_samples_device, for this call."""
        if isinstance(nsteps, (bool, np.bool_)) or int(nsteps) != nsteps or nsteps < 1:
            raise ValueError("nsteps must be an integer >= 1, got %r" % (nsteps,))
        if w is not None:
            w = np.asarray(w, np.float64)
            if w.shape != self.w.shape:
                raise ValueError("w must have shape %s, got %s" % (self.w.shape, w.shape))
            self.w = w
        if self._pending is not None:
            if self._pending[2] != (float(temperature), float(z_temperature)):
                self._prime(temperature, z_temperature)
            self._pending = None
        Xs, self.state = self._gen(self.model, None, int(nsteps), self.w, seed=self.seed, clamp=clamp,
                                   temperature=temperature, z_temperature=z_temperature, state=self.state,
                                   return_state=True, **self._zkw)
        return Xs

    def fork(self, index=None):
        """a Stream that continues from here on its own: all rows (index=None), or the rows `index` (repeats allowed).  Row
        n of a call draws the noise of index n, so a copy at another row continues differently; a copy at the same row of
        an unchanged fork continues like the original."""
        other = object.__new__(Stream)
        other.__dict__.update(self.__dict__)
        other._pending = None
        if index is None:
            other.state, other.w = self.state.clone(), self.w.copy()
        else:
            other.state = self.state.select(index)
            other.w = self.w[np.asarray(index, np.int64)].copy()
        return other


class FilterStream:
    """Particle-filter harmonization of N melodies as their frames arrive: generate_smc's filter, stopped
    after any frame and continued, handing out every frame as soon as it is final.
    FilterStream(model, x_seeds, w, particles, seed=0, resample_threshold=0.5, z_prior=False, max_lag=None); x_seeds as
    Stream's (cl_vrnn [N, S, 88], teacher-forced by the first advance; cl_vae [N, 88]), w [N, C] for the whole stream.
    advance(clamp) runs the chunk's frames and returns those that became final: a frame is final once every surviving
    lineage passes through one ancestor at it, so whatever particle the end of the piece picks, that frame is the one it
    gets.  All emitted frames followed by those of finish() are generate_samples_device(particles=P)'s over the whole roll,
    bit for bit, and log_evidence is its evidence -- in the exact mode, max_lag=None, where the pending frames grow as
    they must.  max_lag=L: after an advance every melody with more than L pending frames is collapsed (collapse()): one
    particle is drawn from the current weights, its pending frames go out and the melody goes on from that particle
    alone.  That is an approximation, the caller's choice: after a collapse log_evidence is no longer the unbiased
    estimate of the evidence.  collapses [N] counts them.
    Not covered, ValueError: a key per particle (w_prior, infer_key), particle Gibbs sweeps, n_out > 1, fork(), and a
    label change between advances."""

    def __init__(self, model, x_seeds, w, particles, seed=0, resample_threshold=0.5, z_prior=False, max_lag=None, **refused):
        for name, why in (('w_prior', 'a filter stream carries no key per particle'),
                          ('infer_key', 'a filter stream carries no key per particle'),
                          ('sweeps', 'a conditional sweep needs the whole piece'), ('n_out', 'a filter stream returns one path')):
            if refused.get(name) is not None and not (name == 'n_out' and refused[name] == 1
                                                      and not isinstance(refused[name], bool)):
                raise ValueError("%s does not combine with a filter stream: %s" % (name, why))
        if set(refused) - {'w_prior', 'infer_key', 'sweeps', 'n_out'}:
            raise ValueError("unknown arguments %s" % sorted(set(refused) - {'w_prior', 'infer_key', 'sweeps', 'n_out'}))
        if isinstance(particles, (bool, np.bool_)) or not isinstance(particles, (int, np.integer)) or particles < 1:
            raise ValueError("particles must be an integer >= 1, got %r" % (particles,))
        if max_lag is not None and (isinstance(max_lag, (bool, np.bool_)) or not isinstance(max_lag, (int, np.integer))
                                    or max_lag < 0):
            raise ValueError("max_lag must be None or an integer >= 0, got %r" % (max_lag,))
        tau = float(resample_threshold)
        if not 0.0 <= tau <= 1.0:
            raise ValueError("resample_threshold must lie in [0, 1], got %r" % (resample_threshold,))
        self.kind, _, _ = _family(model)            # every refusal above comes before the model is touched
        cfg = model.engine.cfg
        x, self.w = np.asarray(x_seeds), np.asarray(w, np.float64)
        rank = 3 if self.kind == 'cl_vrnn' else 2
        if x.ndim != rank or x.shape[0] < 1 or x.shape[-1] != cfg['D']:
            raise ValueError("x_seeds must be %s with N >= 1, got shape %s" % ("[N, S, %d]" % cfg['D'] if rank == 3 else
                                                                               "[N, %d]" % cfg['D'], x.shape))
        if self.w.shape != (x.shape[0], cfg['C']):
            raise ValueError("w must have shape %s, got %s" % ((x.shape[0], cfg['C']), self.w.shape))
        self.model, self.particles, self.seed, self.tau = model, int(particles), int(seed), tau
        self.z_prior, self.max_lag = bool(z_prior), None if max_lag is None else int(max_lag)
        self._x, self.state, self.finished = x, None, False
        self.N = int(x.shape[0])
        self._out = [[] for _ in range(self.N)]
        self.ess, self.picks = None, np.full(self.N, -1, np.int64)

    @property
    def pending(self):
        """[N]: the frames fed and not emitted yet"""
        return np.zeros(self.N, np.int64) if self.state is None or self.finished else self.state.pending()

    @property
    def emitted(self):
        """per melody the frames emitted so far, [count, 88] float64"""
        D = self.model.engine.cfg['D']
        return [np.concatenate(o, axis=0) if o else np.zeros((0, D)) for o in self._out]

    @property
    def log_evidence(self):
        """[N] float64: log Z of the frames fed so far (unbiased only while collapses is all zero)"""
        return np.zeros(self.N) if self.state is None else self.state.logZ.cpu().numpy().copy()

    @property
    def collapses(self):
        return np.zeros(self.N, np.int64) if self.state is None else self.state.collapses.cpu().numpy().astype(np.int64)

    @property
    def t(self):
        return 0 if self.state is None else self.state.t

    def _take(self, emit):
        self.state = emit.state
        frames = emit.frames.cpu().numpy().astype(np.float64)
        for m, c in enumerate(emit.counts):
            if c:
                self._out[m].append(frames[m, :c])
        return frames, emit.counts.copy()

    @staticmethod
    def _join(a, b):
        """two emissions of one call: per melody a's frames, then b's"""
        counts = a[1] + b[1]
        out = np.zeros((len(counts), int(counts.max()) if len(counts) else 0, a[0].shape[2]))
        for m in range(len(counts)):
            out[m, :a[1][m]] = a[0][m, :a[1][m]]
            out[m, a[1][m]:counts[m]] = b[0][m, :b[1][m]]
        return out, counts

    def advance(self, clamp, temperature=1.0, z_temperature=1.0, **refused):
        """feed the next n >= 1 frames' constraints -- a roll uint8 [N, n, 88], or a Constraints with voice counts for them
        -- and return (frames [N, max count, 88] float64, counts [N]): melody m's newly final frames are frames[m,
        :counts[m]], oldest first.  The label is the stream's: advance takes no w."""
        if refused:
            raise ValueError("a filter stream's advance takes the chunk's constraints and the temperatures, not %s (the label "
                             "is the stream's: every particle's history was drawn under it)" % sorted(refused))
        if self.finished:
            raise ValueError("the stream is finished")
        temper_args(temperature, z_temperature)
        emit = self.model.engine.filter_advance(self.state, self._x if self.state is None else None, self.w, clamp,
                                                self.particles, self.tau, seed=self.seed, z_prior=self.z_prior,
                                                temperature=temperature, z_temperature=z_temperature)
        self._x = None
        self.ess = emit.ess.cpu().numpy()
        out = self._take(emit)
        if self.max_lag is not None:
            late = self.state.pending() > self.max_lag
            if late.any():
                out = self._join(out, self.collapse(np.nonzero(late)[0]))
        return out

    def collapse(self, index=None):
        """force the melodies `index` (None: all) onto one particle each, drawn from the current weights; returns their
        pending frames as advance does.  .picks [N] holds the drawn particles (-1: not collapsed by the last call)."""
        if self.finished:
            raise ValueError("the stream is finished")
        if self.state is None:
            raise ValueError("nothing to collapse before the first advance")
        emit = self.model.engine.filter_collapse(self.state, index, seed=self.seed)
        self.picks = emit.picks
        return self._take(emit)

    def finish(self):
        """end the stream: one particle per melody drawn from the final weights as generate_smc draws its path; returns
        its pending frames as advance does.  Afterwards advance and collapse raise."""
        if self.finished:
            raise ValueError("the stream is finished")
        if self.state is None:
            raise ValueError("nothing to finish before the first advance")
        emit = self.model.engine.filter_collapse(self.state, None, seed=self.seed, final=True)
        self.picks = emit.picks
        out = self._take(emit)
        self.finished = True
        return out

    def fork(self, index=None):
        raise ValueError("a filter stream does not fork: its particles' lineages are one filter's")


def check_plan(plan, N, C):
    """a modulation plan [(w0, n0), (w1, n1), ...]: at least one stage, every w [N, C], every n an integer >= 1 -> the
    plan with float64 labels; ValueError otherwise"""
    try:
        stages = [tuple(p) for p in plan]
    except TypeError:
        raise ValueError("plan must be a sequence of (w, nsteps) pairs")
    if not stages or any(len(p) != 2 for p in stages):
        raise ValueError("plan must be a non-empty sequence of (w, nsteps) pairs")
    out = []
    for w, n in stages:
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError("every stage of a plan runs an integer number of frames >= 1, got %r" % (n,))
        w = np.asarray(w, np.float64)
        if w.shape != (int(N), int(C)):
            raise ValueError("every label of a plan must have shape %s, got %s" % ((int(N), int(C)), w.shape))
        out.append((w, int(n)))
    return out


def modulate(model, x_seeds, plan, seed=0, **temper):
    """One piece per seed that changes its label on the way: plan = [(w0, n0), (w1, n1), ...] runs n0 frames under w0 (the
    seed is primed under w0 too), then n1 under w1, ...  Returns [N, sum n, 88] float64.  The frames before the first change
    are those of generate_samples_device(model, x_seeds, n0, w0, seed), bit for bit.  temper: temperature, z_temperature."""
    if set(temper) - {'temperature', 'z_temperature'}:
        raise ValueError("unknown arguments %s" % sorted(set(temper) - {'temperature', 'z_temperature'}))
    temper_args(temper.get('temperature', 1.0), temper.get('z_temperature', 1.0))
    N = np.asarray(x_seeds).shape[0]
    plan = check_plan(plan, N, model.engine.cfg['C'])
    s = Stream(model, x_seeds, plan[0][0], seed=seed, **temper)
    return np.concatenate([s.advance(n, w=w, **temper) for w, n in plan], axis=1)


def chunk_bounds(nsteps, chunk=None, changes=()):
    """the frame ranges [a, b) of a piece of nsteps frames cut every `chunk` frames (None: not at all) and at every frame
    of `changes`"""
    cuts = {0, int(nsteps)} | {int(f) for f in changes}
    if chunk is not None:
        cuts |= set(range(0, int(nsteps), int(chunk)))
    cuts = sorted(c for c in cuts if 0 <= c <= nsteps)
    return list(zip(cuts[:-1], cuts[1:]))


def generate_chunked(model, x_seeds, nsteps, w, chunk=None, changes=(), seed=0, z_prior=False, clamp=None, **temper):
    """generate_samples_device through a Stream: the nsteps frames in chunks of `chunk`, the roll sliced per chunk; changes:
    [(frame, w), ...], from returned frame `frame` on the label is that w.  Without changes the frames are those of the one
    call, bit for bit.  Returns [N, nsteps, 88] float64."""
    if chunk is not None and (isinstance(chunk, bool) or int(chunk) != chunk or chunk < 1):
        raise ValueError("chunk must be an integer >= 1, got %r" % (chunk,))
    frames = [int(f) for f, _ in changes]
    if any(not 0 < f < nsteps for f in frames) or any(b <= a for a, b in zip(frames, frames[1:])):
        raise ValueError("the frames of the changes must be strictly increasing, > 0 and < %d, got %s" % (nsteps, frames))
    new_w = dict((int(f), wv) for f, wv in changes)
    s = Stream(model, x_seeds, w, seed=seed, z_prior=z_prior, **temper)
    out = []
    for a, b in chunk_bounds(nsteps, chunk, frames):
        out.append(s.advance(b - a, w=new_w.get(a), clamp=None if clamp is None else clamp[:, a:b], **temper))
    return np.concatenate(out, axis=1)
