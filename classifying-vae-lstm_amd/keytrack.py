"""Key tracking: the model's label head at every offset of a piece, smoothed by an HMM over the keys.

The model is a CLASSIFYING VAE: its label head names the key of a window (cl_vrnn: seq_length frames, cl_vae: one frame).
track() slides that head over whole pieces -- every window of every piece in one launch, straight from the byte roll
(clv_key_track_windows) -- and lets a sticky HMM (clv_key_track_smooth) turn the per-window posteriors into the key of the
piece, the smoothed key at every window and the Viterbi segmentation: where the piece changes key.  The result feeds what
takes a label: vary(w=), morph.encode(w=), harmonize(w=) and, as segments, stream.modulate's plan."""
import numpy as np

from .trainer import KEY_STREAM  # noqa: F401  (the Philox stream of the label samples, reserved in trainer.py)

MAX_SAMPLES = 1024
MAX_PIECE = 1 << 24          # frames of a piece: the window's start frame is 24 bits of its Philox index


class KeyTrack:
    """What track() returns.  Per piece n (lists of N arrays): starts[n] [J_n] the first frame of every window, wargs[n]
    [J_n, 2(C-1)] = [mean | log_var], logp[n] [J_n, C] the label head's log posterior per window, post[n] [J_n, C] the
    smoothed marginals, path[n] [J_n] the Viterbi path; piece_post [N, C] the posterior over ONE key for the whole piece,
    log_evidence [N] the HMM's log normaliser; lengths [N] the pieces' frames."""

    def __init__(self, T, hop, C, lengths, starts, wargs, logp, post, path, piece_post, log_evidence):
        self.T, self.hop, self.C = int(T), int(hop), int(C)
        self.lengths = [int(p) for p in lengths]
        self.starts, self.wargs, self.logp, self.post, self.path = starts, wargs, logp, post, path
        self.piece_post = np.asarray(piece_post, np.float64)
        self.log_evidence = np.asarray(log_evidence, np.float64)

    def __len__(self):
        return len(self.lengths)

    def key(self, n):
        """the key of piece n: the argmax of piece_post[n] (first index on a tie)"""
        return int(np.argmax(self.piece_post[n]))

    def labels(self, soft=False):
        """label rows [N, C] float64 for vary(w=), morph.encode(w=), harmonize(w=): the one-hot of key(n), or with soft the
        mean over the piece's windows of exp(logp) -- the label head's own average, before any smoothing, which is what
        vary.infer_labels computes at hop = T without samples (a piece without a window: piece_post, i.e. the prior)"""
        if not soft:
            return np.eye(self.C)[[self.key(n) for n in range(len(self))]].reshape(len(self), self.C)
        return np.vstack([np.exp(lp).mean(axis=0) if len(lp) else self.piece_post[n] for n, lp in enumerate(self.logp)])

    def segments(self, n):
        """[(key, first_frame, n_frames), ...] of piece n from its Viterbi path, covering frames 0 .. lengths[n] exactly:
        window j speaks for the frames [j hop, (j+1) hop), the last window also for the tail; a piece without a window is
        one segment in key(n); a piece without frames has none"""
        P, path = self.lengths[n], np.asarray(self.path[n])
        if P == 0:
            return []
        if len(path) == 0:
            return [(self.key(n), 0, P)]
        cuts = [0] + [j for j in range(1, len(path)) if path[j] != path[j - 1]]
        first = [j * self.hop for j in cuts]
        return [(int(path[j]), f, e - f) for j, f, e in zip(cuts, first, first[1:] + [P])]

    def modulation(self, n):
        """segments(n) as stream.modulate's plan for one seed: [(one-hot label [1, C], n_frames), ...]"""
        return [(np.eye(self.C)[[k]], nf) for k, _, nf in self.segments(n)]


def sticky_transitions(C, hop, expected_segment):
    """[C, C]: stay with probability 1 - hop / expected_segment, the rest spread evenly over the other keys"""
    leave = float(hop) / float(expected_segment)
    if not 0.0 < leave < 1.0:
        raise ValueError("expected_segment = %r frames must exceed hop = %d" % (expected_segment, hop))
    A = np.full((C, C), leave / (C - 1))
    A[np.diag_indices(C)] = 1.0 - leave
    return A


def _distribution(a, shape, name):
    a = np.asarray(a, np.float64)
    if a.shape != shape:
        raise ValueError("%s must have shape %s, got %s" % (name, shape, a.shape))
    if not np.all(np.isfinite(a)) or np.any(a <= 0):
        raise ValueError("%s must have positive finite entries (a zero has no logarithm)" % name)
    if np.any(np.abs(a.sum(axis=-1) - 1.0) > 1e-9):
        raise ValueError("%s must sum to 1%s" % (name, " along every row" if a.ndim == 2 else ""))
    return a


def pack_pieces(pieces, D):
    """pieces (a list of binary [P_n, D] arrays, or one [N, P, D] array) -> (uint8 [F, D], lengths [N]); ValueError for a
    wrong frame width, a roll that is not 0 / 1, no piece at all or a piece of 2^24 frames or more"""
    if isinstance(pieces, np.ndarray) and pieces.ndim == 3:
        pieces = list(pieces)
    pieces = [np.asarray(p) for p in pieces]
    if not pieces:
        raise ValueError("no pieces")
    for p in pieces:
        if p.ndim != 2 or p.shape[1] != D:
            raise ValueError("every piece must be [frames, %d], got shape %s" % (D, p.shape))
        if p.shape[0] >= MAX_PIECE:
            raise ValueError("a piece has %d frames; the limit is %d" % (p.shape[0], MAX_PIECE - 1))
        if p.size and not np.all((p == 0) | (p == 1)):
            raise ValueError("pieces must be binary rolls (0 / 1)")
    lengths = [p.shape[0] for p in pieces]
    roll = np.concatenate([p.astype(np.uint8) for p in pieces], axis=0) if sum(lengths) else np.zeros((0, D), np.uint8)
    return np.ascontiguousarray(roll), lengths


def window_counts(lengths, T, hop):
    return [max(0, (p - T) // hop + 1) for p in lengths]


def head_of(model):
    """(is_vae, T, Hd, names of the label head's four tensors) of the model's family"""
    from .engine import VaeEngine
    cfg = model.engine.cfg
    if isinstance(model.engine, VaeEngine):
        return True, 1, cfg['Hc'], ('h_w/kernel', 'h_w/bias', 'wargs/kernel', 'wargs/bias')
    return False, cfg['T'], cfg['D'], ('hW/kernel', 'hW/bias', 'Wargs/kernel', 'Wargs/bias')


def track(model, pieces, hop=1, samples=0, seed=0, expected_segment=64, prior=None, trans=None, kappa=None, piece0=0):
    """Track the key of every piece.  pieces: a list of binary [P_n, 88] arrays of any lengths, or one [N, P, 88] array.
    hop: frames from one window to the next.  samples: 0 for the noise-free label (what every infer_* path uses), K >= 1 for
    the mean over K label samples (noise keyed by seed, the piece's global number piece0 + n and the window's first frame).
    The HMM: prior [C] over the first key (None: uniform), trans [C, C] (row = from; None: sticky_transitions(C, hop,
    expected_segment) -- expected_segment is the user's prior on how long a key lasts, in frames), kappa in (0, 1] the
    exponent on every window's posterior (None: min(1, hop / T): windows T frames long taken every hop frames see each
    frame T / hop times, so their evidence is discounted by the overlap).  Returns a KeyTrack.  ValueError for a wrong frame
    width, a non-binary roll, hop < 1, samples outside 0..1024, a prior / trans of the wrong shape, not normalised or with a
    zero entry, kappa outside (0, 1]."""
    cfg = model.engine.cfg
    D, C = cfg['D'], cfg['C']
    is_vae, T, Hd, names = head_of(model)
    for name, v, lo, hi in (('hop', hop, 1, None), ('samples', samples, 0, MAX_SAMPLES), ('piece0', piece0, 0, None)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
            raise ValueError("%s must be an integer %s, got %r" % (name, ">= %d" % lo if hi is None else "in %d..%d" % (lo, hi), v))
    roll, lengths = pack_pieces(pieces, D)
    log_prior = None if prior is None else np.log(_distribution(prior, (C,), 'prior'))
    A = sticky_transitions(C, hop, expected_segment) if trans is None else _distribution(trans, (C, C), 'trans')
    if kappa is None:
        kappa = min(1.0, float(hop) / T)
    if isinstance(kappa, (bool, np.bool_)) or not 0.0 < float(kappa) <= 1.0:
        raise ValueError("kappa must be in (0, 1], got %r" % (kappa,))

    import torch
    from . import ops
    dev, P = model.engine.device, model.engine.P
    N = len(lengths)
    counts = window_counts(lengths, T, hop)
    piece_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    win_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    Wtot, C1 = int(win_off[-1]), C - 1
    t = lambda a: torch.as_tensor(a, device=dev)
    frames = t(roll) if roll.size else torch.zeros(1, D, dtype=torch.uint8, device=dev)
    po, wo = t(piece_off), t(win_off)
    wargs = torch.empty(max(Wtot, 1), 2 * C1, dtype=torch.float32, device=dev)
    logp = torch.empty(max(Wtot, 1), C, dtype=torch.float32, device=dev)
    post = torch.empty(max(Wtot, 1), C, dtype=torch.float64, device=dev)
    path = torch.empty(max(Wtot, 1), dtype=torch.int32, device=dev)
    log_ev = torch.empty(N, dtype=torch.float64, device=dev)
    piece_post = torch.empty(N, C, dtype=torch.float64, device=dev)
    Kh, bh, Ka, ba = (P.p(n) for n in names)
    ops.key_track_windows(N, T, D, Hd, C, hop, samples, frames, po, wo, Kh, bh, Ka, ba, seed, piece0, wargs, logp)
    ops.key_track_smooth(N, C, wo, logp, None if log_prior is None else t(log_prior), t(np.log(A)), float(kappa), post, path,
                         log_ev, piece_post)
    cut = lambda x: [x[win_off[n]:win_off[n + 1]] for n in range(N)]
    host = lambda x: x[:Wtot].cpu().numpy()
    return KeyTrack(T, hop, C, lengths, [np.arange(c, dtype=np.int64) * hop for c in counts], cut(host(wargs)), cut(host(logp)),
                    cut(host(post)), cut(host(path)), piece_post.cpu().numpy(), log_ev.cpu().numpy())


# ---- the command-line tools cl_vae/keys.py and cl_vrnn/keys.py -------------------------------------------------------------
SPLIT_CHOICES = ('test', 'valid', 'train')


def build_keys_parser():
    import argparse
    p = argparse.ArgumentParser(description="track the key of every song of one split with a trained model's label head "
                                            "and score it against the songs' keys")
    p.add_argument('run_name', type=str, help='tag for current run')
    p.add_argument('-i', '--model_file', type=str, default='', help='trained model weights (.h5, with its .json next to it)')
    p.add_argument('--train_file', type=str, default='../data/input/JSB Chorales_Cs.pickle', help='file of training data (.pickle)')
    p.add_argument('--split', type=str, default='test', choices=SPLIT_CHOICES, help='split to track: test, valid or train')
    p.add_argument('--hop', type=int, default=1, help='frames from one window to the next')
    p.add_argument('--samples', type=int, default=0, help='label samples per window (0: the noise-free label)')
    p.add_argument('--seed', type=int, default=0, help='noise key of the label samples')
    p.add_argument('--expected_segment', type=float, default=64, help='prior on how long a key lasts, in frames')
    p.add_argument('--out', type=str, default='', help='write the results as JSON to this file')
    return p


def split_songs(train_file, split, use_rel_major=True):
    """(rolls, keys, key_map) of one split of a pickle of the reference's schema: every SONG as a uint8 roll [frames, 88],
    its key as an index of key_map -- PianoData's: the sorted union of the three splits' keys, minor keys folded onto
    their relative major"""
    from .utils.pianoroll import SPLITS, _load_pickle, relative_major, song_to_pianoroll
    pickled = _load_pickle(train_file)
    fold = relative_major if use_rel_major else (lambda k: k)
    names = np.unique(np.hstack([[fold(k) for k in pickled[s + '_key']] for s in SPLITS]))
    key_map = {str(k): i for i, k in enumerate(names)}
    rolls = [song_to_pianoroll(s, dtype=np.uint8) if len(s) else np.zeros((0, 88), np.uint8) for s in pickled[split]]
    return rolls, [key_map[str(fold(k))] for k in pickled[split + '_key']], key_map


def score_keys(model, args):
    """The common body of cl_vae/keys.py and cl_vrnn/keys.py: track every song of --split, print the piece-level accuracy of
    KeyTrack.key against the songs' keys, the confusion matrix by key name, the share of songs whose Viterbi path changes key
    and every song's segments; with --out the same as JSON.  Returns the result dictionary."""
    import json
    rolls, keys, key_map = split_songs(args.train_file, args.split)
    C = model.engine.cfg['C']
    if keys and max(keys) >= C:
        raise ValueError("the data set names %d keys, the model has %d classes" % (len(key_map), C))
    names = [str(c) for c in range(C)]
    for k, i in key_map.items():
        if i < C:
            names[i] = k
    kt = track(model, rolls, hop=args.hop, samples=args.samples, seed=args.seed, expected_segment=args.expected_segment)
    found = [kt.key(n) for n in range(len(kt))]
    confusion = np.zeros((C, C), np.int64)
    for true, got in zip(keys, found):
        confusion[true, got] += 1
    segs = [kt.segments(n) for n in range(len(kt))]
    res = dict(split=args.split, model_file=args.model_file, hop=int(args.hop), samples=int(args.samples), seed=int(args.seed),
               expected_segment=float(args.expected_segment), n_songs=len(kt), key_names=names,
               accuracy=float(np.mean(np.asarray(found) == np.asarray(keys))) if keys else float('nan'),
               confusion=confusion.tolist(), modulating=float(np.mean([len(s) > 1 for s in segs])) if segs else float('nan'),
               songs=[dict(key=names[t], found=names[f], frames=kt.lengths[n], log_evidence=float(kt.log_evidence[n]),
                           segments=[[names[k], int(f0), int(nf)] for k, f0, nf in segs[n]])
                      for n, (t, f) in enumerate(zip(keys, found))])
    print("%s split: %d songs, hop %d: key accuracy %.4f, %.4f of the songs change key"
          % (args.split, res['n_songs'], args.hop, res['accuracy'], res['modulating']))
    print("confusion (row = the song's key, column = the key found):")
    print("%6s " % "" + " ".join("%4s" % n for n in names))
    for n, row in zip(names, confusion):
        print("%6s " % n + " ".join("%4d" % v for v in row))
    for n, s in enumerate(res['songs']):
        print("song %d (%s, %d frames): %s" % (n, s['key'], s['frames'],
                                               ", ".join("%s@%d+%d" % tuple(x) for x in s['segments'])))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
    return res
