"""Harmonizing a melody: keep one voice of a piano roll and let a model generate the rest.

A constraint roll (uint8 [N, nsteps, 88], one row per returned frame) fixes notes during device generation: 0 forces a
note off, 1 forces it on, FREE (any other value) leaves it to the model.  The output head factorizes over the notes given
the recurrent state, so inside a frame the free notes are drawn exactly from p(free notes | past, z_t, w); the clamped
frame is then fed back as the next input.  This is clamped ancestral sampling: it does not condition on constraints that
lie in the future.  harmonize(particles=P) samples given the whole voice instead, with a particle filter
(DESIGN.md 11), and can return the model's log p(voice | seed, w)."""
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


def harmonize(model, seeds, source_rolls, w_vals, voice='top', seed=0, fence=True, z_prior=False, particles=None,
              resample_threshold=0.5, return_evidence=False):
    """Generate len(seeds) sequences that keep the `voice` of source_rolls [N, nsteps, 88] and fill in the rest, with the
    frame loop on the device.  seeds: cl_vrnn [N, S, 88] teacher-forced frames (the first source frame follows them),
    cl_vae [N, 88] (frame 0 of the sequence; the first source frame is frame 1).  Returns [N, nsteps, 88] float64.
    particles=P: a particle filter of P particles per melody samples given the whole voice instead of
    clamped ancestral sampling; return_evidence (with particles) also returns log p(voice | seed, w) [N] float64."""
    from .engine import VaeEngine
    source_rolls = np.asarray(source_rolls)
    if source_rolls.ndim != 3:
        raise ValueError("source_rolls must be [N, nsteps, 88], got shape %s" % (source_rolls.shape,))
    clamp = voice_constraints(source_rolls, voice, fence)
    nsteps = source_rolls.shape[1]
    if isinstance(model.engine, VaeEngine):
        from .cl_vae.model import generate_samples_device
        return generate_samples_device(model, seeds, nsteps, w_vals, seed=seed, use_z_prior=z_prior, clamp=clamp,
                                       particles=particles, resample_threshold=resample_threshold,
                                       return_evidence=return_evidence)
    from .cl_vrnn.model import generate_samples_device
    return generate_samples_device(model, seeds, nsteps, w_vals, seed=seed, z_prior=z_prior, clamp=clamp, particles=particles,
                                   resample_threshold=resample_threshold, return_evidence=return_evidence)


def print_evidence(names, log_evidence, nsteps):
    """one line per harmonization: log p(voice | seed, w) per frame (the sample CLIs' --particles)"""
    for name, le in zip(names, np.asarray(log_evidence, dtype=np.float64)):
        print('%s: log p(voice) per frame %.4f (total %.4f over %d frames)' % (name, le / nsteps, le, nsteps))
