"""The four command-line tools' argument tables and the parts of a run that do not depend on the model family.

The reference spells the same flags out four times (cl_vae/train.py:76-121, cl_vrnn/train.py:76-118,
cl_vae/sample.py:35-61, cl_vrnn/sample.py:49-72).  Here each tool is a list of `Flag` rows (names, type, default, help;
verbatim, they are the interface) and the two training scripts share `TrainPlan`: process layout under
torch.distributed, loss-weight ramps, callbacks, the `[y, w, w, y]` target wiring, fit, and the pick of the best epoch.
"""
import argparse
from collections import namedtuple

import numpy as np

from .keras_like import OptimizerSpec, Variable
from .parallel import init_from_env
from .utils.model_utils import (AnnealLossWeight, best_epoch, get_callbacks, init_adam_wn, save_model_in_pieces,
                                to_categorical)

Flag = namedtuple('Flag', 'names kind default help')
ON = 'store_true'          # kind of a switch


def _train_flags(batch_size, seq_length, seq_help, extra=()):
    return [
        Flag(('run_name',), str, None, 'tag for current run'),
        Flag(('--batch_size',), int, batch_size, 'batch size'),
        Flag(('--optimizer',), str, 'adam-wn', 'optimizer name'),
        Flag(('--num_epochs',), int, 200, 'number of epochs'),
        Flag(('--original_dim',), int, 88, 'input dim'),
        Flag(('--intermediate_dim',), int, 88, 'intermediate dim'),
        Flag(('--latent_dim',), int, 2, 'latent dim'),
        Flag(('--seq_length',), int, seq_length, seq_help),
        Flag(('--class_weight',), float, 1.0, 'relative weight on classifying key'),
        Flag(('--w_log_var_prior',), float, 0.0, 'w log var prior'),
        *extra,
        Flag(('--do_log',), ON, False, 'save log files'),
        Flag(('--predict_next',), ON, False, "use x_t to 'autoencode' x_{t+1}"),
        Flag(('--use_x_prev',), ON, False, 'use x_{t-1} to help z_t decode x_t'),
        Flag(('--patience',), int, 5, '# of epochs, for early stopping'),
        Flag(('--kl_anneal',), int, 0, 'number of epochs before kl loss term is 1.0'),
        Flag(('--w_kl_anneal',), int, 0, "number of epochs before w's kl loss term is 1.0"),
        Flag(('--log_dir',), str, '../data/logs', 'basedir for saving log files'),
        Flag(('--model_dir',), str, '../data/models', 'basedir for saving model weights'),
        Flag(('--train_file',), str, '../data/input/JSB Chorales_Cs.pickle', 'file of training data (.pickle)'),
    ]


_SAMPLE_TAIL = [
    Flag(('--sample_dir',), str, '../data/samples', 'basedir for saving output midi files'),
]
_SAMPLE_FILES = [
    Flag(('-i', '--model_file'), str, '', 'preload model weights (no training)'),
    Flag(('--train_file',), str, '../data/input/JSB Chorales_Cs.pickle', 'file of training data (.pickle)'),
]

TABLES = {
    'cl_vae.train': _train_flags(100, 1, 'sequence length (concat)',
                                 extra=[Flag(('--intermediate_class_dim',), int, 88, 'intermediate dims for classes')]),
    'cl_vrnn.train': _train_flags(200, 16, 'sequence length'),
    'cl_vae.sample': [
        Flag(('run_name',), str, None, 'tag for current run'),
        Flag(('-n',), int, 1, 'number of samples'),
        Flag(('--use_z_prior',), ON, False, 'sample z from standard normal at each timestep'),
        Flag(('-t',), int, 32, 'number of timesteps per sample'),
        Flag(('--infer_w',), ON, False, 'infer w when generating'),
        Flag(('--no_x_prev',), ON, False, 'override use_x_prev'),
        *_SAMPLE_TAIL,
        Flag(('--model_dir',), str, '../data/models', 'basedir for saving model weights'),
        *_SAMPLE_FILES,
    ],
    'cl_vrnn.sample': [
        Flag(('run_name',), str, None, 'tag for current run'),
        Flag(('--infer_w',), ON, False, 'infer w when generating'),
        Flag(('--discrete_w',), ON, False, 'sample discrete w when generating'),
        Flag(('-t',), int, 32, 'number of timesteps per sample'),
        Flag(('-n',), int, 1, 'number of samples'),
        Flag(('-c',), str, None, 'set key of seed sample'),
        *_SAMPLE_TAIL,
        *_SAMPLE_FILES,
    ],
}

# the two scoring tools of THIS implementation (the reference has none: its cl_vrnn/train.py builds the test split and
# never uses it): importance-weighted log-likelihood and Keras evaluate() of a trained model on one split
_EVAL_FLAGS = [
    Flag(('run_name',), str, None, 'tag for current run'),
    Flag(('-i', '--model_file'), str, '', 'trained model weights (.h5, with its .json next to it)'),
    Flag(('--train_file',), str, '../data/input/JSB Chorales_Cs.pickle', 'file of training data (.pickle)'),
    Flag(('--split',), str, 'test', 'split to score: test, valid or train'),
    Flag(('-k',), int, 100, 'importance samples per window'),
    Flag(('--seed',), int, 0, 'noise key of the importance samples'),
    Flag(('--out',), str, '', 'write the results as JSON to this file'),
]
TABLES['cl_vae.evaluate'] = list(_EVAL_FLAGS)
TABLES['cl_vrnn.evaluate'] = list(_EVAL_FLAGS)
SPLIT_CHOICES = ('test', 'valid', 'train')

# switches of THIS implementation (not in the reference): where the frame loop of sample.py runs
# cl_vae/train.py only, next to the reference's flags
BF16_FLAGS = [
    Flag(('--bf16',), ON, False, 'Dense products of the fused training step on the bf16 matrix cores (fp32 accumulate)'),
]

# Keras' optimizer arguments that the reference's scripts leave at their defaults (both train.py, next to the reference's flags)
OPTIMIZER_FLAGS = [
    Flag(('--clipnorm',), float, 0.0, 'scale the gradient down to this global L2 norm when it is larger (0: off)'),
    Flag(('--clipvalue',), float, 0.0, 'then clamp every gradient element to +- this value (0: off)'),
    Flag(('--lr_decay',), float, 0.0, 'learning rate lr / (1 + lr_decay * iterations) (0: off)'),
]

# transposition augmentation of the training windows (not in the reference; both train.py)
AUGMENT_FLAGS = [
    Flag(('--transpose',), int, 0, 'transpose every training window by a random number of semitones in -K..K, drawn per step on '
                                   'the device among the shifts that keep its notes on the keyboard and its key among the '
                                   'classes (0: off; at most 12)'),
]

DEVICE_LOOP_FLAGS = [
    Flag(('--device_loop',), ON, False, 'generate all -n samples in one device-side frame loop (Philox noise; opt-in: the default is the reference host loop)'),
    Flag(('--host_loop',), ON, False, 'frame loop on the host with np.random, like the reference (the default; overrides --device_loop)'),
    Flag(('--seed',), int, 0, 'noise key of the device-side loop'),
]

# harmonization (not in the reference): keep one voice of test frames and generate the others (implies --device_loop)
HARMONIZE_CHOICES = ('top', 'bottom')
HARMONIZE_FLAGS = [
    Flag(('--harmonize',), str, None, 'keep the top or bottom voice of the -t test frames after the seed and generate '
                                      'the other voices (clamped sampling on the device; implies --device_loop)'),
    Flag(('--particles',), int, None, 'with --harmonize: sample given the whole voice with a particle filter of this many '
                                      'particles per sample (DESIGN.md 11) and print log p(voice) per frame'),
    Flag(('--infer_key',), str, None, 'with --particles: infer the key from the voice while harmonizing, a key per '
                                      'particle (DESIGN.md 12): discrete keys under a uniform prior, or continuous w under '
                                      "the model's logistic-normal prior; prints the key posterior"),
]
INFER_KEY_CHOICES = ('discrete', 'continuous')

# sampling temperatures (not in the reference): a value other than 1 implies --device_loop
TEMPERATURE_FLAGS = [
    Flag(('--temperature',), float, 1.0, "divide every note's logit by this before the sigmoid: below 1 more conservative, "
                                         'above 1 more adventurous (1e-3 is as good as greedy); on the device loop only'),
    Flag(('--z_temperature',), float, 1.0, 'scale the latent noise by this: 0 keeps z at its mean (at 0 under '
                                           '--use_z_prior); on the device loop only'),
]


# re-decoding (not in the reference): variations of test pieces and key transfer (implies --device_loop)
VARY_HISTORY_CHOICES = ('own', 'source')
VARY_FLAGS = [
    Flag(('--vary',), ON, False, 're-decode the -t test frames of each pick: the encoder reads the piece, the decoder runs on '
                                 'its own output (a variation of the piece; implies --device_loop)'),
    Flag(('--to_key',), str, None, 'with --vary: decode under this key (a name of the data set\'s key map) instead of the '
                                   "piece's own: key transfer"),
    Flag(('--vary_history',), str, 'own', "with --vary: the decoder's previous frame is its own sample (own) or the piece's "
                                          'frame (source: teacher-forced reconstruction)'),
]


# latent morphing (not in the reference): consecutive picks are pairs, K + 1 mixes of each (implies --device_loop)
MORPH_FLAGS = [
    Flag(('--morph',), int, None, 'interpolate between consecutive picks in latent space in this many steps: both pieces are '
                                  'encoded, their latent paths and labels mixed at k / K, k = 0..K, and every mix decoded '
                                  '(the posterior means are mixed unless --z_temperature is given; implies --device_loop)'),
]


# resumable generation (not in the reference): the -t frames a chunk at a time, and a change of key on the way
# (both imply --device_loop)
RESUME_FLAGS = [
    Flag(('--chunk',), int, None, 'generate the -t frames in chunks of this many through a Stream that carries the '
                                  "sampler's state (the same frames as one call; implies --device_loop)"),
    Flag(('--modulate',), str, None, 'NAME@FRAME[,NAME@FRAME...]: from returned frame FRAME on, the label is the one-hot of '
                                     "key NAME (a name of the data set's key map); frames strictly increasing, > 0 and "
                                     'below -t (implies --device_loop)'),
]


# voice counts (not in the reference): how many notes sound in every generated frame (implies --device_loop)
VOICES_FLAGS = [
    Flag(('--voices',), str, None, 'LO[:HI]: every generated frame holds LO (or LO to HI) sounding notes, 0 <= LO <= HI <= 15, '
                                   'drawn exactly given that count; with --harmonize the kept voice counts too (on the '
                                   'device loop only; implies --device_loop)'),
]


# particle Gibbs (not in the reference): sweeps of the particle filter on a retained path
GIBBS_FLAGS = [
    Flag(('--sweeps',), int, None, 'with --particles: this many sweeps of particle Gibbs; every sweep after the first reruns '
                                   'the filter with one particle pinned to the path of the sweep before, so a few particles '
                                   'and several sweeps reach what one pass of many particles would; prints how much of the '
                                   'path each sweep renewed (not with --infer_key)'),
]


# live harmonization (not in the reference): the particle filter fed a chunk of the melody at a time
LIVE_FLAGS = [
    Flag(('--live',), int, None, 'with --harmonize --particles: feed the -t frames to the filter in chunks of this many and '
                                 'print per chunk how many frames are final and how many are held back; the files are those '
                                 'of the run without --live'),
    Flag(('--max_lag',), int, None, 'with --live: hold back at most this many frames per sample; a sample that exceeds it is '
                                    'collapsed onto one particle (an approximation: the files may then differ)'),
]


def live_kwargs(args):
    """--live / --max_lag as (chunk, dict(max_lag=...)); (None, {}) without --live (also for parsers without the flags)"""
    k = getattr(args, 'live', None)
    return (None, {}) if k is None else (int(k), dict(max_lag=getattr(args, 'max_lag', None)))


# novelty audit (not in the reference): the rolls a sampling tool writes against the training split's songs
NOVELTY_FLAGS = [
    Flag(('--novelty',), int, None, 'audit the samples for copied passages: every window of this many frames of every sample '
                                    "against every window of the training split's songs (Hamming distance on the device), and "
                                    'the same for the test split as a baseline; prints per sample the nearest passage'),
    Flag(('--novelty_transpose',), int, 0, 'with --novelty: also look for the passage transposed by up to this many '
                                           'semitones (0..12)'),
]


def novelty_check(args, width):
    """--novelty compares 88-key rolls with the data set's songs: SystemExit for a model whose samples are not such rolls
    (cl_vae with --seq_length > 1 keeps only the notes that sound somewhere -- what --transpose is refused for)"""
    if getattr(args, 'novelty', None) is not None and int(width) != 88:
        raise SystemExit("--novelty compares 88-key rolls with the training songs: not for a model whose frames are %d wide"
                         % width)


# roll statistics audit (not in the reference): the texture of the rolls a sampling tool writes against the songs'
STATS_FLAGS = [
    Flag(('--stats',), ON, None, "audit the samples' texture: per sample the histograms of pitch, scale degree, voices, "
                                 'intervals, note lengths, change between frames, outer-voice steps and span (integer counts on '
                                 "the device), compared with the training split's songs and, as a baseline, the test split's"),
    Flag(('--stats_max_duration',), int, None, 'with --stats: note lengths are counted up to this many frames, longer notes '
                                               'in the last bin (1..64, default 32)'),
]
STATS_MAX_DURATION = 32


def stats_check(args, width):
    """--stats compares 88-key rolls with the data set's songs: SystemExit for a model whose samples are not such rolls (as
    novelty_check)"""
    if getattr(args, 'stats', False) and int(width) != 88:
        raise SystemExit("--stats compares 88-key rolls with the training songs: not for a model whose frames are %d wide"
                         % width)


def gibbs_kwargs(args):
    """--sweeps as keyword arguments of harmonize: empty without the flag (also for parsers without it)"""
    k = getattr(args, 'sweeps', None)
    return {} if k is None else dict(sweeps=k, return_renewed=True)


def parse_voices(text):
    """--voices' LO[:HI] -> (lo, hi); ValueError unless both are integers with 0 <= lo <= hi <= 15"""
    lo, sep, hi = str(text).partition(':')
    try:
        lo = int(lo)
        hi = int(hi) if sep else lo
    except ValueError:
        raise ValueError("--voices takes LO[:HI], got %r" % (text,))
    if not 0 <= lo <= hi <= 15:
        raise ValueError("--voices: 0 <= LO <= HI <= 15, got %r" % (text,))
    return lo, hi


def voices_kwargs(args):
    """--voices as a pair (lo, hi), None without the flag (also for parsers without it)"""
    v = getattr(args, 'voices', None)
    return None if v is None else parse_voices(v)


def parse_modulate(text, t):
    """--modulate's NAME@FRAME[,NAME@FRAME...] -> [(name, frame), ...]; ValueError unless every item has a name and an
    integer frame and the frames are strictly increasing, > 0 and < t"""
    out = []
    for item in str(text).split(','):
        name, at, frame = item.strip().rpartition('@')
        if not at or not name.strip():
            raise ValueError("--modulate takes NAME@FRAME[,NAME@FRAME...], got %r" % (item,))
        try:
            frame = int(frame)
        except ValueError:
            raise ValueError("--modulate: the frame of %r is not an integer" % (item,))
        out.append((name.strip(), frame))
    frames = [f for _, f in out]
    if any(not 0 < f < int(t) for f in frames) or any(b <= a for a, b in zip(frames, frames[1:])):
        raise ValueError("--modulate: frames must be strictly increasing, > 0 and < -t = %d, got %s" % (t, frames))
    return out


def resuming(args):
    """whether --chunk or --modulate was given (also for parsers without the flags)"""
    return getattr(args, 'chunk', None) is not None or getattr(args, 'modulate', None) is not None


def resume_kwargs(args, key_map, n, n_classes):
    """--chunk / --modulate as keyword arguments of stream.generate_chunked: empty without either flag.  The names of
    --modulate are looked up in key_map (PianoData.key_map) and become one-hot label rows [n, n_classes]."""
    if not resuming(args):
        return {}
    chunk, mod = getattr(args, 'chunk', None), getattr(args, 'modulate', None)
    kw = dict(chunk=chunk)
    if mod is not None:
        from .vary import key_rows
        kw['changes'] = [(frame, key_rows(name, n, n_classes, key_map)) for name, frame in parse_modulate(mod, args.t)]
    return kw


def temperature_kwargs(args):
    """the sampling tools' --temperature / --z_temperature as keyword arguments of generate_samples_device / harmonize:
    empty where both are 1 (also for parsers without the flags)"""
    T, Tz = getattr(args, 'temperature', 1.0), getattr(args, 'z_temperature', 1.0)
    return {} if T == 1.0 and Tz == 1.0 else dict(temperature=T, z_temperature=Tz)


def morph_kwargs(args):
    """--temperature / --z_temperature for morph(): the latent temperature stays at morph's default (0: the posterior means
    are mixed) unless the flag was given a value other than 1"""
    kw = dict(temperature=getattr(args, 'temperature', 1.0))
    if getattr(args, 'z_temperature', 1.0) != 1.0:
        kw['z_temperature'] = args.z_temperature
    return kw


class _Parser(argparse.ArgumentParser):
    """argparse with the rules between flags: --particles only with --harmonize, --infer_key only with --particles, --sweeps >= 1 only
    with --particles and not with --infer_key, a temperature other than 1 not with --host_loop (the host loop is the reference's and has none), --vary not with
    --harmonize or --host_loop, --to_key / --vary_history only with --vary, --morph >= 1 and not with --harmonize, --vary or
    --host_loop, --chunk >= 1 and a well-formed --modulate, neither with --particles, --vary, --morph or --host_loop, a
    well-formed --voices LO[:HI] and not with --host_loop, --live >= 1 only with --particles and not with --sweeps,
    --infer_key, --chunk, --modulate, --vary, --morph or --host_loop, --max_lag >= 0 only with --live, --novelty >= 1, --novelty_transpose in 0..12 and only with --novelty,
    --stats_max_duration in 1..64 and only with --stats (without the flag it is 32)"""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        chunk, mod = getattr(ns, 'chunk', None), getattr(ns, 'modulate', None)
        if chunk is not None or mod is not None:
            if chunk is not None and chunk < 1:
                self.error('--chunk must be >= 1')
            if mod is not None:
                try:
                    parse_modulate(mod, ns.t)
                except ValueError as e:
                    self.error(str(e))
            for flag, on in (('--particles', getattr(ns, 'particles', None) is not None), ('--vary', getattr(ns, 'vary', False)),
                             ('--morph', getattr(ns, 'morph', None) is not None), ('--host_loop', getattr(ns, 'host_loop', False))):
                if on:
                    self.error('--chunk / --modulate carry the state of plain or clamped generation on the device: not '
                               'with %s' % flag)
        particles = getattr(ns, 'particles', None)
        if particles is not None:
            if not getattr(ns, 'harmonize', None):
                self.error('--particles needs --harmonize')
            if particles < 1:
                self.error('--particles must be >= 1')
        elif getattr(ns, 'infer_key', None):
            self.error('--infer_key needs --particles')
        sweeps = getattr(ns, 'sweeps', None)
        if sweeps is not None:
            if particles is None:
                self.error('--sweeps needs --particles')
            if sweeps < 1:
                self.error('--sweeps must be >= 1')
            if getattr(ns, 'infer_key', None):
                self.error('--sweeps pins no key: not with --infer_key')
        live, lag = getattr(ns, 'live', None), getattr(ns, 'max_lag', None)
        if live is not None:
            if live < 1:
                self.error('--live must be >= 1')
            if particles is None:
                self.error('--live feeds the particle filter: it needs --harmonize and --particles')
            for flag, on in (('--sweeps', sweeps is not None), ('--infer_key', bool(getattr(ns, 'infer_key', None))),
                             ('--chunk', chunk is not None), ('--modulate', mod is not None),
                             ('--vary', getattr(ns, 'vary', False)), ('--morph', getattr(ns, 'morph', None) is not None),
                             ('--host_loop', getattr(ns, 'host_loop', False))):
                if on:
                    self.error('--live streams one pass of the filter under one label: not with %s' % flag)
            if lag is not None and lag < 0:
                self.error('--max_lag must be >= 0')
        elif lag is not None:
            self.error('--max_lag needs --live')
        if getattr(ns, 'vary', False):
            if getattr(ns, 'harmonize', None):
                self.error('--vary re-decodes whole pieces: not with --harmonize')
            if getattr(ns, 'host_loop', False):
                self.error('--vary runs on the device loop: not with --host_loop')
        elif getattr(ns, 'to_key', None) is not None or getattr(ns, 'vary_history', 'own') != 'own':
            self.error('--to_key / --vary_history need --vary')
        morph = getattr(ns, 'morph', None)
        if morph is not None:
            if morph < 1:
                self.error('--morph must be >= 1')
            if getattr(ns, 'harmonize', None):
                self.error('--morph mixes whole pieces: not with --harmonize')
            if getattr(ns, 'vary', False):
                self.error('--morph decodes mixed latent paths: not with --vary')
            if getattr(ns, 'host_loop', False):
                self.error('--morph runs on the device loop: not with --host_loop')
        voices = getattr(ns, 'voices', None)
        if voices is not None:
            try:
                parse_voices(voices)
            except ValueError as e:
                self.error(str(e))
            if getattr(ns, 'host_loop', False):
                self.error('--voices runs on the device loop: not with --host_loop')
        if not 0 <= getattr(ns, 'transpose', 0) <= 12:
            self.error('--transpose must be in 0..12')
        novelty = getattr(ns, 'novelty', None)
        if novelty is not None and novelty < 1:
            self.error('--novelty must be >= 1')
        if not 0 <= getattr(ns, 'novelty_transpose', 0) <= 12:
            self.error('--novelty_transpose must be in 0..12')
        if novelty is None and getattr(ns, 'novelty_transpose', 0):
            self.error('--novelty_transpose needs --novelty')
        if hasattr(ns, 'stats_max_duration'):
            lmax = ns.stats_max_duration
            if lmax is not None and not getattr(ns, 'stats', False):
                self.error('--stats_max_duration needs --stats')
            if lmax is not None and not 1 <= lmax <= 64:
                self.error('--stats_max_duration must be in 1..64')
            ns.stats_max_duration = STATS_MAX_DURATION if lmax is None else lmax
        temper = temperature_kwargs(ns)
        if temper:
            from .engine_generate import temper_args
            try:
                temper_args(**temper)
            except ValueError as e:
                self.error(str(e))
            if getattr(ns, 'host_loop', False):
                self.error('--temperature / --z_temperature run on the device loop: not with --host_loop')
        return ns, rest


def parser_for(tool, extra=()):
    p = _Parser()
    for f in list(TABLES[tool]) + list(extra):
        if f.kind == ON:
            p.add_argument(*f.names, action=ON, help=f.help)
        elif f.names == ('--split',):
            p.add_argument(*f.names, type=f.kind, default=f.default, choices=SPLIT_CHOICES, help=f.help)
        elif f.names == ('--harmonize',):
            p.add_argument(*f.names, type=f.kind, default=f.default, choices=HARMONIZE_CHOICES, help=f.help)
        elif f.names == ('--vary_history',):
            p.add_argument(*f.names, type=f.kind, default=f.default, choices=VARY_HISTORY_CHOICES, help=f.help)
        elif f.names == ('--infer_key',):
            p.add_argument(*f.names, type=f.kind, default=f.default, choices=INFER_KEY_CHOICES, help=f.help)
        elif f.names[0].startswith('-'):
            p.add_argument(*f.names, type=f.kind, default=f.default, help=f.help)
        else:
            p.add_argument(*f.names, type=f.kind, help=f.help)
    return p


class TrainPlan:
    """Everything of train() that is the same for cl_vae and cl_vrnn.

    Under torch.distributed.run (one process per GPU) `--batch_size` stays the GLOBAL batch: the model is built for
    batch_size / world rows and Model.fit shards every batch (keras_like.Model.fit); a plain `python train.py` is
    world 1."""

    def __init__(self, args):
        self.args = args
        self.rank, local, self.world = init_from_env()
        if args.batch_size % self.world:
            raise SystemExit("--batch_size %d is not divisible by the %d processes" % (args.batch_size, self.world))
        self.local_batch = args.batch_size // self.world
        self.device = 'cuda:%d' % local
        if args.predict_next and args.use_x_prev:
            raise AssertionError("Can't use --predict_next if using --use_x_prev")
        # epochs before this one are never checkpointed, never stop the run and never count as "best"
        self.first_epoch = max(args.kl_anneal, args.w_kl_anneal) + 1
        self.callbacks = get_callbacks(args, patience=args.patience, min_epoch=self.first_epoch, do_log=args.do_log)
        self.kl_weight = self._ramped('kl_weight', args.kl_anneal, start=0.1)
        self.w_kl_weight = self._ramped('w_kl_weight', args.w_kl_anneal, start=0.0)

    def _ramped(self, name, n_epochs, start):
        """1.0, or a variable that a callback raises from `start` to 1.0 over the first n_epochs epochs"""
        if n_epochs <= 0:
            return 1.0
        if n_epochs > self.args.num_epochs:
            raise AssertionError("invalid " + name.replace('_weight', '_anneal'))
        var = Variable(start)
        self.callbacks.append(AnnealLossWeight(var, name=name, final_value=1.0, n_epochs=n_epochs))
        return var

    def labels(self, P, n_classes):
        return to_categorical(P.train_song_keys, n_classes), to_categorical(P.valid_song_keys, n_classes)

    def optimizer(self):
        """The optimizer object for get_model; `args.optimizer` keeps the flag's string for the run's JSON."""
        a = self.args
        clip = dict(decay=getattr(a, 'lr_decay', 0.0), clipnorm=getattr(a, 'clipnorm', 0.0), clipvalue=getattr(a, 'clipvalue', 0.0))
        opt, _ = init_adam_wn(a.optimizer)
        if not any(clip.values()):
            return opt
        if isinstance(opt, OptimizerSpec):          # 'adam-wn': the reference's hyper-parameters, with OPTIMIZER_FLAGS on top
            return type(opt)(lr=opt.lr, beta_1=opt.beta_1, beta_2=opt.beta_2, epsilon=opt.epsilon, **clip)
        return OptimizerSpec.resolve(opt, **clip)   # 'adam', 'rmsprop'

    def augment(self, P, w_train):
        """--transpose K: the augment.TransposePlan of the training windows (None when the flag is 0 or absent)"""
        K = getattr(self.args, 'transpose', 0)
        if not K:
            return None
        if np.ndim(P.x_train) == 2 and self.args.seq_length > 1:
            # cl_vae's flattened windows keep only the notes that sound somewhere: a column is no semitone any more
            raise SystemExit("--transpose shifts frames of all 88 notes: not with cl_vae's --seq_length > 1")
        from .augment import TransposePlan
        plan = TransposePlan.build([P.y_train, P.x_train], P.train_song_keys, P.key_map, semitones=K,
                                   n_classes=w_train.shape[1])
        if self.rank == 0:
            n = plan.counts()
            print("Transposing by up to %d semitones: %d to %d of %d shifts allowed per window."
                  % (K, n.min(), n.max(), 2 * K + 1))
        return plan

    def describe(self, model):
        if self.rank == 0:
            save_model_in_pieces(model, self.args)

    def fit(self, model, P, w_train, w_valid, best_from=None):
        """inputs [y, x] (current frames, history) with --use_x_prev, else x; targets [recon, w, w, recon].
        Returns the history entries of the best epoch (lowest val_loss from epoch `best_from` on; default: the first
        epoch after the ramps)."""
        a = self.args
        if a.use_x_prev:
            x_tr, x_va = [P.y_train, P.x_train], [P.y_valid, P.x_valid]
        else:
            x_tr, x_va = P.x_train, P.x_valid
        hist = model.fit(x_tr, [P.y_train, w_train, w_train, P.y_train], shuffle=True, epochs=a.num_epochs,
                         batch_size=a.batch_size, callbacks=self.callbacks, augment=self.augment(P, w_train),
                         validation_data=(x_va, [P.y_valid, w_valid, w_valid, P.y_valid]))
        at = best_epoch(hist.history['val_loss'], self.first_epoch if best_from is None else best_from)
        return {k: v[at] for k, v in hist.history.items()}


def score_split(model, x, y, args, margs):
    """The common tail of cl_vae/evaluate.py and cl_vrnn/evaluate.py: the importance-weighted log-likelihood and Keras
    evaluate() of `model` on one split's windows (x, y as fit() takes them), printed and, with --out, written as JSON.
    The model's noise key is --seed (evaluate() draws from it), so two runs with the same flags write the same file."""
    import json
    model.seed = int(args.seed)
    # load_model rebuilds the layers only; the label prior is part of p(x) and of the w_kl loss
    model.engine.cfg['w_log_var_prior'] = float(margs.get('w_log_var_prior', 0.0))
    res = model.log_likelihood(x, y, k=args.k, seed=args.seed)
    res['evaluate'] = dict(zip(model.metrics_names, model.evaluate(x, y)))
    res.update(split=args.split, model_file=args.model_file, seed=int(args.seed))
    print("%s split: %d windows, K = %d: log-likelihood %.4f nats per window (%.4f per frame), ELBO %.4f, ESS %.2f"
          % (args.split, res['n_windows'], res['k'], res['log_likelihood'], res['log_likelihood_per_frame'], res['elbo'],
             res['ess']))
    print(" - ".join("%s: %.4f" % kv for kv in res['evaluate'].items()))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
    return res
