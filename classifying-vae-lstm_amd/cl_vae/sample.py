"""cl_vae sampling CLI (reference: code/cl_vae/sample.py; flags :35-61 verbatim in clvae_amd.cli.TABLES)."""
import os
import sys

import numpy as np

if __package__ in (None, ''):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import clvae_amd  # noqa: E402,F401
from clvae_amd.cl_vae import model as M  # noqa: E402
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


class Sampler:
    """The trained model's three inference views plus the test split the seed frames come from."""

    def __init__(self, args):
        self.args = args
        self.model, _, self.margs = M.load_model(args.model_file, no_x_prev=args.no_x_prev,
                                                 batch_size=max(1, args.n * (getattr(args, 'particles', None) or 1)
                                                                if on_device(args) else 1))
        m, dims = self.margs, (self.margs['intermediate_dim'], self.margs['latent_dim'])
        self.w_enc = M.make_w_encoder(self.model, m['original_dim'])
        self.z_enc = M.make_z_encoder(self.model, m['original_dim'], m['n_classes'], dims)
        self.dec = M.make_decoder(self.model, dims, m['n_classes'], use_x_prev=m['use_x_prev'])
        # --harmonize: windows of the seed frame and the t frames whose voice is kept
        self.data = PianoData(args.train_file, batch_size=1, seq_length=args.t + 1 if voice_of(args) else args.t,
                              squeeze_x=True)
        self.keys = []          # --stats: the class every sample is generated under, None where no one label holds

    def pick_seed(self):
        """(first frame of a random test window, its key's one-hot or None with --infer_w); one np.random draw"""
        i = np.random.choice(range(len(self.data.x_test)))
        self.keys.append(None if self.args.infer_w else int(self.data.test_song_keys[i]))
        w = None if self.args.infer_w else to_categorical(self.data.test_song_keys[i], self.margs['n_classes'])
        return self.data.x_test[i][0], w

    def one(self, name):
        x_seed, w_val = self.pick_seed()
        roll = M.generate_sample(self.dec, self.w_enc, self.z_enc, x_seed, self.args.t, w_val=w_val,
                                 use_z_prior=self.args.use_z_prior, use_x_prev=self.margs['use_x_prev'])
        write_sample(roll, self.args.sample_dir, name, True)
        return roll

    def many_on_device(self, names):
        """All samples in one device-side frame loop (Philox noise; the seeds are drawn like one() draws them)."""
        seeds, ws = zip(*[self.pick_seed() for _ in names])
        if self.args.infer_w:
            ws = [M.sample_w(self.w_enc.predict(s[None, :]), add_noise=False) for s in seeds]
        resume = resume_kwargs(self.args, self.data.key_map, len(names), self.margs['n_classes'])
        if getattr(self.args, 'modulate', None) is not None:
            self.keys = None    # the label changes on the way
        if resume:              # --chunk / --modulate: the same call a chunk at a time
            rolls = generate_chunked(self.model, np.stack(seeds), self.args.t, np.vstack(ws), seed=getattr(self.args, 'seed', 0),
                                     z_prior=self.args.use_z_prior, **resume, **temperature_kwargs(self.args),
                                     **count_clamp(self.args))
        else:
            rolls = M.generate_samples_device(self.model, np.stack(seeds), self.args.t, np.vstack(ws),
                                              seed=getattr(self.args, 'seed', 0), use_z_prior=self.args.use_z_prior,
                                              **temperature_kwargs(self.args), **count_clamp(self.args))
        for roll, name in zip(rolls, names):
            write_sample(roll, self.args.sample_dir, name, True)
        return list(rolls)

    def harmonize_on_device(self, names):
        """--harmonize: frame 0 of a random test window is the seed, the chosen voice of its next t frames the
        constraint; writes <name>.mid (the harmonization) and <name>_source.mid (the original frames)."""
        picks = [np.random.choice(range(len(self.data.x_test))) for _ in names]
        wins = [np.asarray(self.data.x_test[i]).reshape(self.args.t + 1, -1) for i in picks]
        seeds, sources = np.stack([w[0] for w in wins]), np.stack([w[1:] for w in wins])
        particles = getattr(self.args, 'particles', None)
        infer_key = getattr(self.args, 'infer_key', None)
        self.keys = (None if infer_key or self.args.infer_w or getattr(self.args, 'modulate', None) is not None
                     else [int(self.data.test_song_keys[i]) for i in picks])
        if infer_key:           # --infer_key: the filter weighs the keys by the voice, a key per particle
            ws = None
            self.model.engine.cfg['w_log_var_prior'] = float(self.margs.get('w_log_var_prior', 0.0))
        elif self.args.infer_w:
            ws = [M.sample_w(self.w_enc.predict(s[None, :]), add_noise=False) for s in seeds]
        else:
            ws = [to_categorical(self.data.test_song_keys[i], self.margs['n_classes']) for i in picks]
        resume = resume_kwargs(self.args, self.data.key_map, len(names), self.margs['n_classes'])
        if resume:              # --chunk / --modulate: harmonize()'s call a chunk at a time, the roll sliced per chunk
            out = generate_chunked(self.model, seeds, self.args.t, np.vstack(ws), seed=getattr(self.args, 'seed', 0),
                                   z_prior=self.args.use_z_prior, clamp=kept_voice(self.args, sources),
                                   **resume, **temperature_kwargs(self.args))
        elif live_kwargs(self.args)[0]:     # --live: the filter fed a chunk at a time, final frames handed out on the way
            live, live_kw = live_kwargs(self.args)
            out = live_harmonize(accompany(self.model, seeds, np.vstack(ws), voice=voice_of(self.args), particles=particles,
                                           voices=voices_kwargs(self.args), seed=getattr(self.args, 'seed', 0),
                                           z_prior=self.args.use_z_prior, **live_kw),
                                 sources, live, **temperature_kwargs(self.args))
        else:
            out = harmonize(self.model, seeds, sources, None if ws is None else np.vstack(ws), voice=voice_of(self.args),
                            seed=getattr(self.args, 'seed', 0), z_prior=self.args.use_z_prior, particles=particles,
                            return_evidence=particles is not None, **(dict(infer_key=infer_key) if infer_key else {}),
                            **temperature_kwargs(self.args), voices=voices_kwargs(self.args), **gibbs_kwargs(self.args))
        rolls = out[0] if particles is not None else out
        if particles is not None:
            print_evidence(names, out[1], self.args.t)
            if gibbs_kwargs(self.args):     # --sweeps: out = (the last sweep's rolls, sweep 0's evidence, renewed)
                print_renewed(names, out[2])
            if infer_key:
                print_key_posterior(names, out[2], self.data.key_map)
        for roll, src, name in zip(rolls, sources, names):
            write_sample(roll, self.args.sample_dir, name, True)
            write_sample(src, self.args.sample_dir, name + '_source', True)
        return list(rolls)

    def vary_on_device(self, names):
        """--vary: the t frames of a random test window re-decoded under their own key (the data's, or the
        w-encoder's mean over the frames with --infer_w), or under --to_key; writes <name>.mid and <name>_source.mid."""
        picks = [np.random.choice(range(len(self.data.x_test))) for _ in names]
        sources = np.stack([np.asarray(self.data.x_test[i]).reshape(self.args.t, -1) for i in picks])
        ws = None if self.args.infer_w else np.vstack([to_categorical(self.data.test_song_keys[i], self.margs['n_classes'])
                                                       for i in picks])
        self.keys = (None if self.args.infer_w or getattr(self.args, 'to_key', None) is not None
                     else [int(self.data.test_song_keys[i]) for i in picks])
        rolls = vary(self.model, sources, ws, to_key=getattr(self.args, 'to_key', None), key_map=self.data.key_map,
                     history=getattr(self.args, 'vary_history', 'own'), seed=getattr(self.args, 'seed', 0),
                     **temperature_kwargs(self.args), **count_clamp(self.args))
        for roll, src, name in zip(rolls, sources, names):
            write_sample(roll, self.args.sample_dir, name, True)
            write_sample(src, self.args.sample_dir, name + '_source', True)
        return list(rolls)

    def morph_on_device(self, names):
        """--morph K: consecutive picks are pairs (a, b): the t frames of two random test windows (of the key -c where
        given) are encoded and K + 1 mixes of their latent paths and labels decoded; writes <run>_<j>_a.mid,
        <run>_<j>_b.mid and <run>_<j>_morph<k>.mid, k = 0..K."""
        pool = np.arange(len(self.data.x_test))
        key = getattr(self.args, 'c', None)
        if key is not None:
            name_of = {idx: name for name, idx in self.data.key_map.items()}
            pool = pool[np.array([name_of[k] for k in self.data.test_song_keys]) == key]
        n = 2 * (len(names) // 2)
        self.keys = None        # a mix of two labels
        if not n or not len(pool):
            return []
        picks = [np.random.choice(pool) for _ in range(n)]
        sources = np.stack([np.asarray(self.data.x_test[i]).reshape(self.args.t, -1) for i in picks])
        ws = None if self.args.infer_w else np.vstack([to_categorical(self.data.test_song_keys[i], self.margs['n_classes'])
                                                       for i in picks])
        rolls = morph(self.model, sources[0::2], sources[1::2], steps=self.args.morph,
                      w_a=None if ws is None else ws[0::2], w_b=None if ws is None else ws[1::2],
                      seed=getattr(self.args, 'seed', 0), **morph_kwargs(self.args), **count_clamp(self.args))
        for j, rows in enumerate(rolls):
            write_sample(sources[2 * j], self.args.sample_dir, '%s_%d_a' % (self.args.run_name, j), True)
            write_sample(sources[2 * j + 1], self.args.sample_dir, '%s_%d_b' % (self.args.run_name, j), True)
            for k, roll in enumerate(rows):
                write_sample(roll, self.args.sample_dir, '%s_%d_morph%d' % (self.args.run_name, j, k), True)
        return list(rolls)


def make_sample(P, dec_model, w_enc_model, z_enc_model, args, margs):
    """One sample from explicit sub-models (the reference's helper, :8-19)."""
    i = np.random.choice(range(len(P.x_test)))
    w_val = None if args.infer_w else to_categorical(P.test_song_keys[i], margs['n_classes'])
    roll = M.generate_sample(dec_model, w_enc_model, z_enc_model, P.x_test[i][0], args.t, w_val=w_val,
                             use_z_prior=args.use_z_prior, use_x_prev=margs['use_x_prev'])
    write_sample(roll, args.sample_dir, args.run_name, True)
    return roll


def count_clamp(args):
    """--voices as the clamp= of a call without a roll: {} without the flag (also for parsers without it)"""
    v = voices_kwargs(args)
    return {} if v is None else dict(clamp=voice_counts(v, None))


def kept_voice(args, sources):
    """--harmonize's roll over `sources`, under --voices with the frames' counts"""
    roll, v = voice_constraints(sources, getattr(args, 'harmonize', None)), voices_kwargs(args)
    return roll if v is None else voice_counts(v, sources, roll)


def voice_of(args):
    """--harmonize's voice, or None (also for parsers without the flag)"""
    return getattr(args, 'harmonize', None)


def on_device(args):
    """Where the frame loop runs: like the reference (host loop, np.random) for every -n unless --device_loop asks for
    the device-side loop (Philox noise: other samples for the same np.random.seed, so it is opt-in); --harmonize
    --vary, --morph, --chunk and --modulate always run there, and so does a sampling temperature (the parser refuses them
    next to --host_loop), and so does --voices."""
    return bool(voice_of(args)) or getattr(args, 'voices', None) is not None or bool(getattr(args, 'vary', False)) or getattr(args, 'morph', None) is not None or bool(
        temperature_kwargs(args)) or resuming(args) or (
        bool(getattr(args, 'device_loop', False)) and not getattr(args, 'host_loop', False))


def sample(args):
    s = Sampler(args)
    novelty_check(args, s.margs['original_dim'])
    stats_check(args, s.margs['original_dim'])
    names = ['%s_%d' % (args.run_name, i) for i in range(args.n)]
    if voice_of(args):
        rolls = s.harmonize_on_device(names)
    elif getattr(args, 'vary', False):
        rolls = s.vary_on_device(names)
    elif getattr(args, 'morph', None) is not None:
        rolls = s.morph_on_device(names)
    else:
        rolls = s.many_on_device(names) if on_device(args) else [s.one(nm) for nm in names]
    audit_samples(rolls, args)          # --novelty: the rolls just written against the training songs
    stats.audit_samples(rolls, args, keys=s.keys)       # --stats: their texture against the songs' 
    return rolls


def build_parser():
    return parser_for('cl_vae.sample')


if __name__ == '__main__':
    sample(parser_for('cl_vae.sample',
                      DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS + TEMPERATURE_FLAGS + VARY_FLAGS + MORPH_FLAGS
                      + RESUME_FLAGS + VOICES_FLAGS + GIBBS_FLAGS + STATS_FLAGS + NOVELTY_FLAGS + LIVE_FLAGS).parse_args())
