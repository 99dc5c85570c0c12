"""Novelty audit: the nearest training passage of every window of a generated piece.

The samplers can run on their own output for as long as one likes and the data sets are small, so "did the sampler just
replay bars of a training chorale, possibly in another key?" is the first question about a generated piece.  nearest()
answers it on the device: every window of W frames of every query piece against every window of every corpus piece, at
every offset and every transposition in -K..K that keeps the window's notes on the keyboard, in Hamming distance over the
binary roll (clv_roll_nearest).  The result names, per window, the distance, the shift and where in the corpus the match
starts; Novelty turns that into the share of a piece that is copied, its longest copied run and the distances' quantiles.

    python -m clvae_amd.novelty --train_file F [--split test] [--against train] [-w 16] [--hop 1] [--transpose 0]
                                [--rolls file.npy] [--out res.json]

scores one split of a data set (or a saved [N, P, 88] array of rolls) against another split."""
import numpy as np

from .keytrack import SPLIT_CHOICES, pack_pieces, window_counts

MAX_WINDOW, MAX_SEMITONES, MAX_WIDTH = 1024, 12, 116


class Novelty:
    """What nearest() returns.  Per query piece n (lists of N arrays over the piece's J_n windows): dist[n] the Hamming
    distance to the nearest corpus window (-1: the window had no candidate), shift[n] the transposition in semitones at
    which it was found, song[n] / frame[n] the corpus piece and the frame in it where the match starts (-1 where dist is
    -1), starts[n] the windows' first frames, notes[n] the sounding notes (set cells) of every window -- dist / notes is
    the share of a window's notes that differ at most.  window, hop, semitones: the call's."""

    def __init__(self, window, hop, semitones, lengths, dist, shift, song, frame, starts, notes):
        self.window, self.hop, self.semitones = int(window), int(hop), int(semitones)
        self.lengths = [int(p) for p in lengths]
        self.dist, self.shift, self.song, self.frame, self.starts, self.notes = dist, shift, song, frame, starts, notes

    def __len__(self):
        return len(self.lengths)

    def _hit(self, n, max_dist):
        d = np.asarray(self.dist[n])
        return (d >= 0) & (d <= max_dist)

    def copied(self, max_dist=0):
        """[N]: the share of each piece's windows with 0 <= dist <= max_dist (0 for a piece without a window)"""
        return np.asarray([float(self._hit(n, max_dist).mean()) if len(self.dist[n]) else 0.0 for n in range(len(self))])

    def longest_copy(self, n, max_dist=0):
        """the frames covered by the longest run of consecutive windows of piece n with 0 <= dist <= max_dist:
        (run - 1) * hop + window, 0 without such a window; consecutive windows must touch (hop <= window)"""
        if self.hop > self.window:
            raise ValueError("longest_copy needs hop <= window (windows %d frames long, %d apart, do not touch)"
                             % (self.window, self.hop))
        run = best = 0
        for h in self._hit(n, max_dist):
            run = run + 1 if h else 0
            best = max(best, run)
        return (best - 1) * self.hop + self.window if best else 0

    def quantiles(self, qs=(0, .1, .5, .9, 1)):
        """the quantiles qs of dist over all windows that had a candidate (NaN without any)"""
        d = np.concatenate([np.asarray(x).reshape(-1) for x in self.dist]) if self.dist else np.zeros(0)
        d = d[d >= 0]
        return np.full(len(qs), np.nan) if d.size == 0 else np.quantile(d.astype(np.float64), qs)

    def closest(self, n):
        """(dist, shift, song, frame, start) of piece n's window nearest to the corpus (the first such window), or None"""
        d = np.asarray(self.dist[n])
        if not (d >= 0).any():
            return None
        j = int(np.argmin(np.where(d >= 0, d, np.iinfo(np.int64).max)))
        return int(d[j]), int(self.shift[n][j]), int(self.song[n][j]), int(self.frame[n][j]), int(self.starts[n][j])

    def summary(self, n, max_dist=0):
        """piece n in numbers: the dictionary the tools print and write"""
        d = np.asarray(self.dist[n])
        d = d[d >= 0]
        c = self.closest(n)
        return dict(frames=self.lengths[n], windows=int(len(self.dist[n])),
                    min_dist=int(d.min()) if d.size else -1, median_dist=float(np.median(d)) if d.size else -1.0,
                    copied=float(self.copied(max_dist)[n]),
                    longest_copy=int(self.longest_copy(n, max_dist)) if self.hop <= self.window else -1,
                    nearest_song=c[2] if c else -1, nearest_frame=c[3] if c else -1, shift=c[1] if c else 0)

    def to_json(self):
        lst = lambda xs: [np.asarray(x).tolist() for x in xs]
        return dict(window=self.window, hop=self.hop, semitones=self.semitones, lengths=list(self.lengths),
                    dist=lst(self.dist), shift=lst(self.shift), song=lst(self.song), frame=lst(self.frame),
                    starts=lst(self.starts), notes=lst(self.notes), copied=self.copied().tolist(),
                    quantiles=[None if np.isnan(q) else float(q) for q in self.quantiles()])


def _int_in(name, v, lo, hi):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or v < lo or (hi is not None and v > hi):
        raise ValueError("%s must be an integer %s, got %r" % (name, ">= %d" % lo if hi is None else "in %d..%d" % (lo, hi), v))
    return int(v)


def _width(pieces):
    if isinstance(pieces, np.ndarray) and pieces.ndim == 3:
        return int(pieces.shape[2])
    pieces = list(pieces)
    if not pieces:
        raise ValueError("no pieces")
    p = np.asarray(pieces[0])
    if p.ndim != 2:
        raise ValueError("every piece must be [frames, notes], got shape %s" % (p.shape,))
    return int(p.shape[1])


def nearest(queries, corpus, window=16, hop=1, semitones=0, exclude=None, device='cuda:0'):
    """The nearest corpus window of every window of every query piece.  queries, corpus: lists of binary [P, D] rolls of
    any lengths, or one [N, P, D] array each, D <= 116 the same on both sides.  window: frames per window (1..1024); hop:
    frames from one query window to the next (the corpus is searched at every offset); semitones: K in 0..12, the match
    may be transposed by -K..K where that keeps the query window's notes inside 0..D-1; exclude: per query piece the index
    of a corpus piece that is no candidate for it (-1 or None: none) -- the leave-one-out baseline, or "how far did vary
    move from its source".  Ties go to the smaller shift (0, -1, +1, -2, ...), then to the earlier corpus frame.  Returns a
    Novelty.  ValueError for rolls that are not 0 / 1, a wrong or too large width, window, hop or semitones out of range,
    an exclude of the wrong length or out of range."""
    W, hop, S = _int_in('window', window, 1, MAX_WINDOW), _int_in('hop', hop, 1, None), _int_in('semitones', semitones, 0, MAX_SEMITONES)
    D = _width(queries)
    if not 1 <= D <= MAX_WIDTH:
        raise ValueError("frames must be 1..%d notes wide, got %d" % (MAX_WIDTH, D))
    q_roll, q_len = pack_pieces(queries, D)
    c_roll, c_len = pack_pieces(corpus, D)
    Nq, Nc = len(q_len), len(c_len)
    if exclude is not None:
        ex = np.asarray([-1 if e is None else e for e in exclude])
        if ex.shape != (Nq,) or ex.dtype.kind not in 'iu':
            raise ValueError("exclude must hold one corpus piece index (or -1) per query piece: %d integers" % Nq)
        if np.any(ex < -1) or np.any(ex >= Nc):
            raise ValueError("exclude must be -1 or a corpus piece index below %d" % Nc)
        ex = ex.astype(np.int32)
    counts = window_counts(q_len, W, hop)
    q_off = np.concatenate([[0], np.cumsum(q_len)]).astype(np.int64)
    c_off = np.concatenate([[0], np.cumsum(c_len)]).astype(np.int64)
    w_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    Wq = int(w_off[-1])

    import torch
    from . import ops
    dev = torch.device(device)
    t = lambda a: torch.as_tensor(a, device=dev)
    roll = lambda r: t(r) if r.size else torch.zeros(1, D, dtype=torch.uint8, device=dev)
    dist = torch.empty(max(Wq, 1), dtype=torch.int32, device=dev)
    shift = torch.empty(max(Wq, 1), dtype=torch.int32, device=dev)
    cframe = torch.empty(max(Wq, 1), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        ops.roll_nearest(Nq, Nc, W, hop, S, D, q_roll.shape[0], c_roll.shape[0], Wq, roll(q_roll), t(q_off), roll(c_roll),
                         t(c_off), t(w_off), None if exclude is None else t(ex), dist, shift, cframe)
        dist, shift, cframe = (x[:Wq].cpu().numpy() for x in (dist, shift, cframe))
    song = np.where(cframe < 0, -1, np.searchsorted(c_off, cframe, side='right') - 1).astype(np.int64)
    frame = np.where(cframe < 0, -1, cframe - c_off[np.maximum(song, 0)]).astype(np.int64)
    cut = lambda x: [x[w_off[n]:w_off[n + 1]] for n in range(Nq)]
    starts = [np.arange(c, dtype=np.int64) * hop for c in counts]
    per_frame = np.concatenate([[0], np.cumsum(q_roll.sum(axis=1, dtype=np.int64))])
    notes = [per_frame[q_off[n] + s + W] - per_frame[q_off[n] + s] for n, s in enumerate(starts)]
    return Novelty(W, hop, S, q_len, cut(dist), cut(shift), cut(song), cut(frame), starts, notes)


# ---- the audit of the two sample.py tools (--novelty W, --novelty_transpose K) ----------------------------------------------
def flatten_rolls(rolls):
    """the rolls a sampling tool is about to write, as a flat list of [t, D] arrays (--morph returns a list per pair)"""
    out = []
    for r in rolls:
        if isinstance(r, (list, tuple)) or (isinstance(r, np.ndarray) and r.ndim == 3):
            out.extend(flatten_rolls(r))
        else:
            out.append((np.asarray(r) > 0).astype(np.uint8))
    return out


def audit_samples(rolls, args, device='cuda:0'):
    """--novelty W [--novelty_transpose K] of cl_vae/sample.py and cl_vrnn/sample.py: the rolls against the songs of the
    training split, a line per sample, then the same figures for the test split's songs as the baseline (a sample that is
    closer to the training set than held-out music is suspect).  Returns (the samples' Novelty, the baseline's), or None
    without the flag or without a roll."""
    W = getattr(args, 'novelty', None)
    if W is None:
        return None
    from .keytrack import split_songs
    K = getattr(args, 'novelty_transpose', 0)
    rolls = flatten_rolls(rolls)
    if not rolls:
        return None
    train = split_songs(args.train_file, 'train')[0]
    test = split_songs(args.train_file, 'test')[0]
    nov = nearest(rolls, train, window=W, semitones=K, device=device)
    base = nearest(test, train, window=W, semitones=K, device=device)
    print("novelty: windows of %d frames, transposed by up to %d semitones, against %d training songs" % (W, K, len(train)))
    for n in range(len(nov)):
        print("sample %d: " % n + describe(nov.summary(n)))
    q = base.quantiles((0, .5))
    print("baseline, %d test songs: min dist %s, median %s, copied %.4f, longest copy %d frames"
          % (len(base), *("%g" % v for v in q), float(np.mean(base.copied())) if len(base) else 0.0,
             max([base.longest_copy(n) for n in range(len(base))] or [0])))
    return nov, base


def describe(s):
    if s['min_dist'] < 0:
        return "%d windows, none with a candidate" % s['windows']
    return ("min dist %d, median %g, copied %.4f, longest copy %d frames, nearest: song %d at frame %d, shift %+d"
            % (s['min_dist'], s['median_dist'], s['copied'], s['longest_copy'], s['nearest_song'], s['nearest_frame'], s['shift']))


# ---- python -m clvae_amd.novelty ------------------------------------------------------------------------------------------
def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog='python -m clvae_amd.novelty',
                                description="novelty audit: the nearest passage of one split's songs (or of saved rolls) in "
                                            "another split, per window, in Hamming distance over the binary roll")
    p.add_argument('--train_file', type=str, required=True, help='file of training data (.pickle)')
    p.add_argument('--split', type=str, default='test', choices=SPLIT_CHOICES, help='split whose songs are scored')
    p.add_argument('--against', type=str, default='train', choices=SPLIT_CHOICES,
                   help='split that is searched; the same as --split: every song leaves itself out')
    p.add_argument('-w', '--window', type=int, default=16, help='frames per window')
    p.add_argument('--hop', type=int, default=1, help='frames from one scored window to the next')
    p.add_argument('--transpose', type=int, default=0, help='also search transpositions by up to this many semitones (0..12)')
    p.add_argument('--rolls', type=str, default='', help='score this saved [N, P, 88] array (.npy) instead of --split')
    p.add_argument('--out', type=str, default='', help='write the results as JSON to this file')
    return p


def main(argv=None):
    import json
    from .keytrack import split_songs
    p = build_parser()
    args = p.parse_args(argv)
    if not 1 <= args.window <= MAX_WINDOW or args.hop < 1 or not 0 <= args.transpose <= MAX_SEMITONES:
        p.error('-w in 1..%d, --hop >= 1, --transpose in 0..%d' % (MAX_WINDOW, MAX_SEMITONES))
    corpus = split_songs(args.train_file, args.against)[0]
    if args.rolls:
        queries, exclude, what = (np.load(args.rolls) > 0).astype(np.uint8), None, args.rolls
    else:
        queries, what = split_songs(args.train_file, args.split)[0], args.split
        exclude = list(range(len(queries))) if args.split == args.against else None
    nov = nearest(queries, corpus, window=args.window, hop=args.hop, semitones=args.transpose, exclude=exclude)
    songs = [nov.summary(n) for n in range(len(nov))]
    qs = (0, .1, .5, .9, 1)
    quant = nov.quantiles(qs)
    order = sorted((n for n in range(len(nov)) if songs[n]['min_dist'] >= 0), key=lambda n: (songs[n]['min_dist'], n))[:10]
    closest = [dict(query=n, song=songs[n]['nearest_song'], frame=songs[n]['nearest_frame'], shift=songs[n]['shift'],
                    dist=songs[n]['min_dist']) for n in order]
    res = dict(query=what, against=args.against, window=args.window, hop=args.hop, transpose=args.transpose,
               leave_one_out=exclude is not None, n_songs=len(nov), n_corpus=len(corpus),
               quantiles={"%g" % q: (None if np.isnan(v) else float(v)) for q, v in zip(qs, quant)},
               copied=float(np.mean(nov.copied())) if len(nov) else 0.0, songs=songs, closest=closest)
    print("%s against %s: %d songs, windows of %d frames every %d, transposed by up to %d%s"
          % (what, args.against, len(nov), args.window, args.hop, args.transpose, ", every song leaves itself out" if exclude else ""))
    print("dist quantiles: " + ", ".join("%g: %s" % (q, "%g" % v) for q, v in zip(qs, quant)))
    print("share of windows copied (dist 0): %.4f" % res['copied'])
    for c in closest:
        print("song %(query)d: nearest is song %(song)d at frame %(frame)d, shift %(shift)+d, dist %(dist)d" % c)
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
    return res


if __name__ == '__main__':
    main()
