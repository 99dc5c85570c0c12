"""cl_vrnn sampling CLI (reference: code/cl_vrnn/sample.py; flags :49-72 verbatim in clvae_amd.cli.TABLES)."""
import os
import sys

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import clvae_amd  # noqa: E402,F401
from clvae_amd.cl_vrnn import model as M  # noqa: E402
from clvae_amd.cli import (DEVICE_LOOP_FLAGS, GIBBS_FLAGS, HARMONIZE_FLAGS, LIVE_FLAGS, MORPH_FLAGS, NOVELTY_FLAGS,  # noqa: E402
                           RESUME_FLAGS, STATS_FLAGS, TEMPERATURE_FLAGS, VARY_FLAGS, VOICES_FLAGS, gibbs_kwargs, live_kwargs, morph_kwargs,
                           novelty_check, parser_for, resume_kwargs, resuming, stats_check, temperature_kwargs, voices_kwargs)
from clvae_amd.harmonize import (accompany, harmonize, live_harmonize, print_evidence, print_key_posterior,  # noqa: E402
                                 print_renewed, voice_constraints, voice_counts)
from clvae_amd.stream import generate_chunked  # noqa: E402
from clvae_amd.utils.midi_utils import write_sample  # noqa: E402
from clvae_amd.utils.model_utils import to_categorical  # noqa: E402
from clvae_amd.utils.pianoroll import PianoData  # noqa: E402
from clvae_amd.morph import morph  # noqa: E402
from clvae_amd.novelty import audit_samples  # noqa: E402
from clvae_amd import stats  # noqa: E402
from clvae_amd.vary import vary  # noqa: E402


def seed_windows(P, key, n):
    """Up to n test windows in random order (one np.random.shuffle), all keys or only those in `key`."""
    name_of = {idx: name for name, idx in P.key_map.items()}
    picks = np.arange(len(P.test_song_keys))
    if key is not None:
        picks = picks[np.array([name_of[k] for k in P.test_song_keys]) == key]
    np.random.shuffle(picks)
    return picks[:n]


def one_label(args):
    """whether every sample is generated under the one label of its seed window: not with an inferred label, a label that
    changes on the way (--modulate, --to_key) or a mix of two (--morph)"""
    return not (args.infer_w or getattr(args, 'infer_key', None) or getattr(args, 'modulate', None) is not None
                or getattr(args, 'to_key', None) is not None or getattr(args, 'morph', None) is not None)


def gen_samples(P, dec_model, w_enc_model, z_enc_model, args, margs, model=None, keys_out=None):
    """Seed windows -> generated continuations; writes <run>_<j>.mid and the seed as <run><j>_seed_<i>.mid.
    With `model` the frame loops of all seeds run together on the device (Philox noise).  keys_out: a list that receives
    the class every sample is generated under, where one label holds (--stats)."""
    half_speed = 'jsb' in args.train_file.lower()
    picks = seed_windows(P, args.c, args.n)
    if keys_out is not None and one_label(args):
        keys_out.extend(int(P.test_song_keys[i]) for i in picks)
    label_of = lambda i: None if args.infer_w else to_categorical(P.test_song_keys[i], margs['n_classes'])
    voice = getattr(args, 'harmonize', None)
    if voice:
        return harmonize_samples(P, w_enc_model, args, margs, model, picks, label_of, voice, half_speed)
    if getattr(args, 'vary', False):
        return vary_samples(P, w_enc_model, args, margs, model, picks, label_of, half_speed)
    if getattr(args, 'morph', None) is not None:
        return morph_samples(P, w_enc_model, args, margs, model, picks, label_of, half_speed)
    if model is not None and len(picks):
        ws = [label_of(i) for i in picks]
        if args.infer_w:
            ws = [M.infer_label(w_enc_model, P.x_test[i], margs['seq_length'], discrete=args.discrete_w) for i in picks]
        resume = resume_kwargs(args, P.key_map, len(picks), margs['n_classes'])
        if resume:              # --chunk / --modulate: the same call a chunk at a time
            rolls = list(generate_chunked(model, np.stack([P.x_test[i] for i in picks]), args.t, np.vstack(ws),
                                          seed=getattr(args, 'seed', 0), **resume, **temperature_kwargs(args),
                                          **count_clamp(args)))
        else:
            rolls = list(M.generate_samples_device(model, np.stack([P.x_test[i] for i in picks]), args.t, np.vstack(ws),
                                                   seed=getattr(args, 'seed', 0), **temperature_kwargs(args),
                                                   **count_clamp(args)))
    else:
        rolls = [M.generate_sample(dec_model, w_enc_model, z_enc_model, P.x_test[i], args.t, margs['use_x_prev'],
                                   w_val=label_of(i), w_discrete=args.discrete_w, seq_length=margs['seq_length'])
                 for i in picks]
    for j, (i, roll) in enumerate(zip(picks, rolls)):
        write_sample(roll, args.sample_dir, '%s_%d' % (args.run_name, j), half_speed)
        write_sample(P.x_test[i], args.sample_dir, '%s%d_seed_%d' % (args.run_name, j, i), half_speed)
    return rolls


def harmonize_samples(P, w_enc_model, args, margs, model, picks, label_of, voice, half_speed):
    """--harmonize: windows of 2t frames; the first t are the teacher-forced seed, the chosen voice of the next t the
    constraint.  Writes <run>_<j>.mid (the harmonization), <run>_<j>_source.mid (the original frames) and the seed."""
    t = args.t
    if not len(picks):
        return []
    seeds = np.stack([np.asarray(P.x_test[i])[:t] for i in picks])
    sources = np.stack([np.asarray(P.x_test[i])[t:2 * t] for i in picks])
    particles = getattr(args, 'particles', None)
    infer_key = getattr(args, 'infer_key', None)
    if infer_key:               # --infer_key: the filter weighs the keys by the voice, a key per particle
        model.engine.cfg['w_log_var_prior'] = float(margs.get('w_log_var_prior', 0.0))      # load_model rebuilds layers only
        out = harmonize(model, seeds, sources, None, voice=voice, seed=getattr(args, 'seed', 0), particles=particles,
                        return_evidence=True, infer_key=infer_key, **temperature_kwargs(args), voices=voices_kwargs(args))
    else:
        ws = [label_of(i) for i in picks]
        if args.infer_w:
            ws = [M.infer_label(w_enc_model, s, margs['seq_length'], discrete=args.discrete_w) for s in seeds]
        resume = resume_kwargs(args, P.key_map, len(picks), margs['n_classes'])
        live, live_kw = live_kwargs(args)
        if resume:              # --chunk / --modulate: harmonize()'s call a chunk at a time, the roll sliced per chunk
            out = generate_chunked(model, seeds, t, np.vstack(ws), seed=getattr(args, 'seed', 0),
                                   clamp=kept_voice(args, sources), **resume, **temperature_kwargs(args))
        elif live:              # --live: the filter fed `live` frames at a time, final frames handed out on the way
            out = live_harmonize(accompany(model, seeds, np.vstack(ws), voice=voice, particles=particles,
                                           voices=voices_kwargs(args), seed=getattr(args, 'seed', 0), **live_kw),
                                 sources, live, **temperature_kwargs(args))
        else:
            out = harmonize(model, seeds, sources, np.vstack(ws), voice=voice, seed=getattr(args, 'seed', 0),
                            particles=particles, return_evidence=particles is not None, **temperature_kwargs(args),
                            voices=voices_kwargs(args), **gibbs_kwargs(args))
    rolls = list(out[0] if particles is not None else out)
    if particles is not None:
        names = ['%s_%d' % (args.run_name, j) for j in range(len(rolls))]
        print_evidence(names, out[1], t)
        if gibbs_kwargs(args):      # --sweeps: out = (the last sweep's rolls, sweep 0's evidence, renewed)
            print_renewed(names, out[2])
        if infer_key:
            print_key_posterior(names, out[2], P.key_map)
    for j, (i, roll) in enumerate(zip(picks, rolls)):
        write_sample(roll, args.sample_dir, '%s_%d' % (args.run_name, j), half_speed)
        write_sample(sources[j], args.sample_dir, '%s_%d_source' % (args.run_name, j), half_speed)
        write_sample(seeds[j], args.sample_dir, '%s%d_seed_%d' % (args.run_name, j, i), half_speed)
    return rolls


def vary_samples(P, w_enc_model, args, margs, model, picks, label_of, half_speed):
    """--vary: the t frames of each picked test window re-decoded under their own key, or under --to_key.
    Writes <run>_<j>.mid (the re-decoding) and <run>_<j>_source.mid (the window's frames)."""
    if not len(picks):
        return []
    sources = np.stack([np.asarray(P.x_test[i])[:args.t] for i in picks])
    ws = [label_of(i) for i in picks]
    if args.infer_w:
        ws = [M.infer_label(w_enc_model, s, margs['seq_length'], discrete=args.discrete_w) for s in sources]
    rolls = list(vary(model, sources, np.vstack(ws), to_key=getattr(args, 'to_key', None), key_map=P.key_map,
                      history=getattr(args, 'vary_history', 'own'), seed=getattr(args, 'seed', 0), **temperature_kwargs(args),
                      **count_clamp(args)))
    for j, roll in enumerate(rolls):
        write_sample(roll, args.sample_dir, '%s_%d' % (args.run_name, j), half_speed)
        write_sample(sources[j], args.sample_dir, '%s_%d_source' % (args.run_name, j), half_speed)
    return rolls


def morph_samples(P, w_enc_model, args, margs, model, picks, label_of, half_speed):
    """--morph K: consecutive picks are pairs (a, b); the t frames of both are encoded and K + 1 mixes of their latent paths
    and labels decoded.  Writes <run>_<j>_a.mid, <run>_<j>_b.mid and <run>_<j>_morph<k>.mid, k = 0..K."""
    picks = picks[:2 * (len(picks) // 2)]
    if not len(picks):
        return []
    sources = np.stack([np.asarray(P.x_test[i])[:args.t] for i in picks])
    ws = [label_of(i) for i in picks]
    if args.infer_w:
        ws = [M.infer_label(w_enc_model, s, margs['seq_length'], discrete=args.discrete_w) for s in sources]
    ws = np.vstack(ws)
    rolls = morph(model, sources[0::2], sources[1::2], steps=args.morph, w_a=ws[0::2], w_b=ws[1::2],
                  seed=getattr(args, 'seed', 0), **morph_kwargs(args), **count_clamp(args))
    for j, rows in enumerate(rolls):
        write_sample(sources[2 * j], args.sample_dir, '%s_%d_a' % (args.run_name, j), half_speed)
        write_sample(sources[2 * j + 1], args.sample_dir, '%s_%d_b' % (args.run_name, j), half_speed)
        for k, roll in enumerate(rows):
            write_sample(roll, args.sample_dir, '%s_%d_morph%d' % (args.run_name, j, k), half_speed)
    return list(rolls)


def count_clamp(args):
    """--voices as the clamp= of a call without a roll: {} without the flag (also for parsers without it)"""
    v = voices_kwargs(args)
    return {} if v is None else dict(clamp=voice_counts(v, None))


def kept_voice(args, sources):
    """--harmonize's roll over `sources`, under --voices with the frames' counts"""
    roll, v = voice_constraints(sources, getattr(args, 'harmonize', None)), voices_kwargs(args)
    return roll if v is None else voice_counts(v, sources, roll)


def sample(args):
    model, _, margs = M.load_model(args.model_file, optimizer='adam')
    dims = (margs['intermediate_dim'], margs['latent_dim'])
    w_enc = M.make_w_encoder(model, margs['original_dim'], margs['n_classes'], margs['seq_length'])
    z_enc = M.make_z_encoder(model, margs['original_dim'], margs['n_classes'], dims)
    dec = M.make_decoder(model, margs['original_dim'], margs['intermediate_dim'], margs['latent_dim'],
                         margs['n_classes'], margs['use_x_prev'])
    voice = getattr(args, 'harmonize', None)
    # --harmonize: windows of the seed's t frames and the t frames whose voice is kept
    P = PianoData(args.train_file, batch_size=1, seq_length=2 * args.t if voice else args.t, squeeze_x=False)
    # the reference's host loop (np.random) for every -n; --device_loop opts into the device-side loop (Philox noise), and
    # a sampling temperature, --vary, --morph, --chunk, --modulate and --voices imply it (the parser refuses them next to
    # --host_loop)
    on_device = bool(voice) or getattr(args, 'voices', None) is not None or bool(getattr(args, 'vary', False)) or getattr(args, 'morph', None) is not None or bool(
        temperature_kwargs(args)) or resuming(args) or (
        bool(getattr(args, 'device_loop', False)) and not getattr(args, 'host_loop', False))
    novelty_check(args, margs['original_dim'])
    stats_check(args, margs['original_dim'])
    keys = []
    rolls = gen_samples(P, dec, w_enc, z_enc, args, margs, model=model if on_device else None, keys_out=keys)
    audit_samples(rolls, args)          # --novelty: the rolls just written against the training songs
    stats.audit_samples(rolls, args, keys=keys or None)         # --stats: their texture against the songs' 
    return rolls


def build_parser():
    return parser_for('cl_vrnn.sample')


if __name__ == '__main__':
    sample(parser_for('cl_vrnn.sample',
                      DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS + TEMPERATURE_FLAGS + VARY_FLAGS + MORPH_FLAGS
                      + RESUME_FLAGS + VOICES_FLAGS + GIBBS_FLAGS + STATS_FLAGS + NOVELTY_FLAGS + LIVE_FLAGS).parse_args())
