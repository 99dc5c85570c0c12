"""Resumable generation: a piece generated a chunk at a time on the device.

generate_samples_device(state=..., return_state=True) of both families carries the samplers' state from call to call; this
module is the convenient face of it.  A Stream holds the state of N pieces and advances them by any number of frames per
call -- endless generation, a live accompaniment a bar at a time, a roll that arrives chunk by chunk.  The label, the roll
and the temperatures may change between calls: modulate() changes the key on the way.  fork() branches: one prefix, several
continuations.  However a piece is cut into chunks, its frames are bit for bit those of one call."""
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
