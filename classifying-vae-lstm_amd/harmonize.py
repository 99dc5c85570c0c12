"""Harmonizing a melody: keep one voice of a piano roll and let a model generate the rest.

A constraint roll (uint8 [N, nsteps, 88], one row per returned frame) fixes notes during device generation: 0 forces a
note off, 1 forces it on, FREE (any other value) leaves it to the model.  The output head factorizes over the notes given
the recurrent state, so inside a frame the free notes are drawn exactly from p(free notes | past, z_t, w); the clamped
frame is then fed back as the next input.  This is clamped ancestral sampling: it does not condition on constraints that
lie in the future.  harmonize(particles=P) samples given the whole voice instead, with a particle filter
(DESIGN.md 11), and can return the model's log p(voice | seed, w); with sweeps=K it runs K sweeps of particle Gibbs on
that filter.  harmonize(particles=P, infer_key=...) gives every
particle a key of its own, so that the key follows the voice: it also returns the posterior over the key."""
import numpy as np

FREE = 255
VOICES = ('top', 'bottom')


def voice_constraints(roll, voice='top', fence=True):
    """Constraint roll that keeps one voice of `roll` ([..., 88], nonzero = sounding): in every frame the highest
    (voice='top') or lowest ('bottom') sounding note is forced on and, with `fence`, every note above (below) it is forced
    off; all other notes are FREE.  A frame with no sounding note is entirely FREE.  Returns uint8 of roll's shape."""
    if voice not in VOICES:
        raise ValueError("voice must be one of %s, got %r" % (VOICES, voice))
    on = np.asarray(roll) != 0
    D = on.shape[-1]
    out = np.full(on.shape, FREE, dtype=np.uint8)
    flat, cons = on.reshape(-1, D), out.reshape(-1, D)
    sounding = flat.any(axis=1)
    idx = np.arange(D)
    if voice == 'top':
        pick = D - 1 - np.argmax(flat[:, ::-1], axis=1)
        outside = idx[None, :] > pick[:, None]
    else:
        pick = np.argmax(flat, axis=1)
        outside = idx[None, :] < pick[:, None]
    if fence:
        cons[sounding[:, None] & outside] = 0
    rows = np.nonzero(sounding)[0]
    cons[rows, pick[rows]] = 1
    return out


def voice_counts(voices, source_rolls, roll=None):
    """harmonize's voices argument as an engine_generate.Constraints over `roll`: an int k, a pair (lo, hi), or 'source'
    (every frame as many sounding notes as the frame of source_rolls)"""
    from .engine_generate import Constraints
    if isinstance(voices, str):
        if voices != 'source':
            raise ValueError("voices must be an int, a pair (lo, hi) or 'source', got %r" % (voices,))
        return Constraints.as_in(source_rolls, roll=roll)
    if isinstance(voices, (tuple, list)):
        if len(voices) != 2:
            raise ValueError("voices must be an int, a pair (lo, hi) or 'source', got %r" % (voices,))
        return Constraints.between(voices[0], voices[1], roll=roll)
    return Constraints.exactly(voices, roll=roll)


INFER_KEY = ('discrete', 'continuous')


def default_w_prior(model, N, infer_key):
    """the key prior of harmonize(infer_key=...): 'discrete' every key equally likely, 'continuous' the model's own
    logistic-normal prior (mean 0, log variance w_log_var_prior)"""
    from .engine_generate import WPrior
    cfg = model.engine.cfg
    if infer_key == 'discrete':
        return WPrior.uniform(N, cfg['C'])
    shape = (N, cfg['C'] - 1)
    return WPrior.logistic_normal(np.zeros(shape), np.full(shape, float(cfg.get('w_log_var_prior', 0.0))))


def harmonize(model, seeds, source_rolls, w_vals=None, voice='top', seed=0, fence=True, z_prior=False, particles=None,
              resample_threshold=0.5, return_evidence=False, infer_key=None, w_prior=None, temperature=1.0, z_temperature=1.0,
              voices=None, sweeps=None, return_renewed=False):
    """Generate len(seeds) sequences that keep the `voice` of source_rolls [N, nsteps, 88] and fill in the rest, with the
    frame loop on the device.  seeds: cl_vrnn [N, S, 88] teacher-forced frames (the first source frame follows them),
    cl_vae [N, 88] (frame 0 of the sequence; the first source frame is frame 1).  Returns [N, nsteps, 88] float64.
    particles=P: a particle filter of P particles per melody samples given the whole voice instead of
    clamped ancestral sampling; return_evidence (with particles) also returns log p(voice | seed, w) [N] float64.
    infer_key='discrete' | 'continuous' (with particles, instead of w_vals): every particle draws its own w from a prior
    over the key (default_w_prior, or the WPrior given as w_prior) and the filter weighs the keys by the voice
    (DESIGN.md 12).  The evidence is then log p(voice | seed), and the call also returns, after it, the key posterior
    w_posterior [N, nsteps, C] (after each frame) and the label w_out [N, C] of each returned sequence, float64.
    temperature, z_temperature: harmonize with the tempered model (note logits divided by temperature, latent
    noise scaled by z_temperature); evidence and key posterior are then that tempered model's, not the trained model's
    unless both are 1.
    voices: how many notes sound in every returned frame, the kept voice included -- an int k (exactly k), a
    pair (lo, hi), or 'source' (as many as the source frame has).  Each frame is then drawn exactly from p(frame | the kept
    voice, count in range); with particles the evidence becomes log p(voice and texture | seed, w).  The call runs on the
    frame chain or in the filter.  ValueError for a frame that cannot be had: the kept voice needs lo - 1 free notes on its
    open side (with `fence`), and counts go up to 15.
    sweeps=K (with particles): K sweeps of particle Gibbs instead of one pass of the filter; the last sweep's
    sequences are returned, the evidence is sweep 0's, and return_renewed adds renewed [N, K, nsteps] bool (which frames
    each sweep took from a particle other than the pinned one).  ValueError for sweeps without particles or with
    infer_key."""
    from .engine import VaeEngine
    source_rolls = np.asarray(source_rolls)
    if source_rolls.ndim != 3:
        raise ValueError("source_rolls must be [N, nsteps, 88], got shape %s" % (source_rolls.shape,))
    extra = {}
    if sweeps is not None or return_renewed:
        if sweeps is not None and particles is None:
            raise ValueError("sweeps needs particles")
        if sweeps is not None and (infer_key is not None or w_prior is not None):
            raise ValueError("sweeps do not combine with infer_key: a conditional sweep pins no key")
        extra = dict(sweeps=sweeps, return_renewed=return_renewed)
    if infer_key is not None:
        if infer_key not in INFER_KEY:
            raise ValueError("infer_key must be one of %s, got %r" % (INFER_KEY, infer_key))
        if w_vals is not None:
            raise ValueError("give either w_vals or infer_key, not both")
        if particles is None:
            raise ValueError("infer_key needs particles: a single path cannot weigh keys")
        extra.update(w_prior=w_prior if w_prior is not None else default_w_prior(model, source_rolls.shape[0], infer_key),
                     return_key=True)
    elif w_prior is not None:
        raise ValueError("w_prior needs infer_key")
    elif w_vals is None:
        raise ValueError("harmonize needs w_vals (or infer_key with particles)")
    clamp = voice_constraints(source_rolls, voice, fence)
    if voices is not None:
        clamp = voice_counts(voices, source_rolls, clamp)
    nsteps = source_rolls.shape[1]
    extra.update(temperature=temperature, z_temperature=z_temperature)
    if isinstance(model.engine, VaeEngine):
        from .cl_vae.model import generate_samples_device
        return generate_samples_device(model, seeds, nsteps, w_vals, seed=seed, use_z_prior=z_prior, clamp=clamp,
                                       particles=particles, resample_threshold=resample_threshold,
                                       return_evidence=return_evidence, **extra)
    from .cl_vrnn.model import generate_samples_device
    return generate_samples_device(model, seeds, nsteps, w_vals, seed=seed, z_prior=z_prior, clamp=clamp, particles=particles,
                                   resample_threshold=resample_threshold, return_evidence=return_evidence, **extra)


class Accompaniment:
    """accompany()'s object: feed(source_chunk) harmonizes the next frames of the melodies, finish() ends the piece; .stream
    is the stream.FilterStream underneath (emitted, pending, log_evidence, ess, collapses, collapse())."""

    def __init__(self, stream, voice, fence, voices):
        self.stream, self.voice, self.fence, self.voices = stream, voice, fence, voices

    def feed(self, source_chunk, temperature=1.0, z_temperature=1.0):
        """source_chunk [N, n, 88]: the next n >= 1 frames of the pieces whose voice is kept.  Returns (frames, counts) as
        FilterStream.advance: the harmonized frames that became final."""
        src = np.asarray(source_chunk)
        if src.ndim != 3 or src.shape[0] != self.stream.N or src.shape[1] < 1:
            raise ValueError("source_chunk must be [%d, n, 88] with n >= 1, got shape %s" % (self.stream.N, src.shape))
        clamp = voice_constraints(src, self.voice, self.fence)
        if self.voices is not None:
            clamp = voice_counts(self.voices, src, clamp)
        return self.stream.advance(clamp, temperature=temperature, z_temperature=z_temperature)

    def finish(self):
        return self.stream.finish()

    emitted = property(lambda self: self.stream.emitted)
    pending = property(lambda self: self.stream.pending)
    log_evidence = property(lambda self: self.stream.log_evidence)
    collapses = property(lambda self: self.stream.collapses)


def accompany(model, seeds, w_vals, voice='top', particles=64, fence=True, voices=None, **stream_kw):
    """harmonize(particles=P) for melodies that arrive a chunk at a time: returns an Accompaniment whose
    feed(source_chunk) builds the chunk's constraints as harmonize does (voice_constraints, and voice_counts under
    `voices`) and advances a stream.FilterStream by them, returning the frames that are final; finish() returns the rest.
    All of them together are harmonize(model, seeds, the whole source, w_vals, particles=P)'s frames, bit for bit, unless
    max_lag forces frames out early.  stream_kw: FilterStream's seed, resample_threshold, z_prior, max_lag."""
    from .stream import FilterStream
    if voice not in VOICES:
        raise ValueError("voice must be one of %s, got %r" % (VOICES, voice))
    if w_vals is None:
        raise ValueError("accompany needs w_vals: a filter stream carries no key per particle")
    return Accompaniment(FilterStream(model, seeds, w_vals, particles, **stream_kw), voice, fence, voices)


def live_harmonize(acc, source_rolls, chunk, **temper):
    """the sample CLIs' --live: source_rolls [N, nsteps, 88] fed to the Accompaniment `chunk` frames at a time, a line
    printed per chunk, then finish().  Returns (frames [N, nsteps, 88] float64, log_evidence [N]) like
    harmonize(particles=P, return_evidence=True)."""
    source_rolls = np.asarray(source_rolls)
    nsteps = source_rolls.shape[1]
    for i, a in enumerate(range(0, nsteps, int(chunk))):
        b = min(nsteps, a + int(chunk))
        _, counts = acc.feed(source_rolls[:, a:b], **temper)
        print_live(i, a, b, counts, acc.pending)
    _, counts = acc.finish()
    print('live finish: emitted %s' % ' '.join(str(int(c)) for c in counts))
    return np.stack(acc.emitted), acc.log_evidence


def print_live(chunk, first, last, counts, pending):
    """one line per fed chunk (the sample CLIs' --live): what went out and what is still held back, per sample"""
    print('live chunk %d (frames %d..%d): emitted %s pending %s' % (chunk, first, last - 1, ' '.join(str(int(c)) for c in counts),
                                                                   ' '.join(str(int(p)) for p in pending)))


def print_evidence(names, log_evidence, nsteps):
    """one line per harmonization: log p(voice | seed, w) per frame (the sample CLIs' --particles)"""
    for name, le in zip(names, np.asarray(log_evidence, dtype=np.float64)):
        print('%s: log p(voice) per frame %.4f (total %.4f over %d frames)' % (name, le / nsteps, le, nsteps))


def print_renewed(names, renewed):
    """one line per harmonization: the share of its frames that each sweep took from a particle other than the pinned one
    (the sample CLIs' --sweeps; sweep 0, the plain filter, renews everything)"""
    for name, r in zip(names, np.asarray(renewed, dtype=np.float64)):
        print('%s: renewed per sweep %s' % (name, ' '.join('%.2f' % v for v in r.mean(axis=-1))))


def print_key_posterior(names, w_posterior, key_map):
    """one line per harmonization: the posterior over the key after the last frame, most probable key first (the sample
    CLIs' --infer_key); key_map: PianoData.key_map (key name -> class index)"""
    name_of = {int(idx): str(name) for name, idx in key_map.items()}
    for name, post in zip(names, np.asarray(w_posterior, dtype=np.float64)[:, -1]):
        order = np.argsort(-post, kind='stable')
        print('%s: key posterior %s' % (name, ' '.join('%s=%.4f' % (name_of.get(int(c), str(int(c))), post[c])
                                                         for c in order)))
