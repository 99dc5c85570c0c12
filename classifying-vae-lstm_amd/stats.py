"""Roll statistics audit: does a sample have the corpus's texture?

Likelihood says how probable held-out music is, keytrack which key a piece is in, novelty whether a sample copies the
training set.  profile() says what a batch of rolls LOOKS like, per piece, as integer histograms formed on the device
(clv_roll_stats): which notes sound (pitch) and on which degrees of the key's scale (degree), how many at once (voices), at
which intervals (interval), for how many frames (duration), how many cells change from one frame to the next (change), how
the highest and the lowest voice step (top_step, bottom_step) and how far apart they are (span).  RollStats turns the
table into distributions and a few means -- in_scale, the share of the sounding notes inside the major scale of the key a
sample was generated under, is the Classifying VAE's main claim about its samples -- and compare() measures two batches
against each other, section by section, in Jensen-Shannon divergence.

    python -m clvae_amd.stats --train_file F [--split test] [--against train] [--rolls file.npy] [--max_duration 32]
                              [--out res.json]

profiles one split of a data set (or a saved [N, P, 88] array of rolls) and compares it with another split."""
import numpy as np

from .keytrack import SPLIT_CHOICES, pack_pieces

VOICES, CHANGE, STEP = 16, 16, 24           # CLV_STATS_VOICES, CLV_STATS_CHANGE, CLV_STATS_STEP of include/clvae.h
MAX_DURATION, MAX_WIDTH, MAX_PIECES = 64, 116, 1 << 20
SECTIONS = ('pitch', 'degree', 'voices', 'interval', 'duration', 'change', 'top_step', 'bottom_step', 'span')
IN_SCALE = (0, 2, 4, 5, 7, 9, 11)           # the degrees of the major scale (and of its relative natural minor)


def section_bins(D, Lmax):
    """name -> bins of the section in a row of clv_roll_stats' table, in the row's order"""
    return dict(zip(SECTIONS, (D, 12, VOICES + 1, D, Lmax, CHANGE + 1, 2 * STEP + 1, 2 * STEP + 1, D)))


def _normalised(h):
    h = np.asarray(h, np.float64)
    s = h.sum(axis=-1, keepdims=True)
    return np.divide(h, s, out=np.zeros_like(h), where=s > 0)


def js_divergence(p, q):
    """Jensen-Shannon divergence in bits (0..1) of distributions along the last axis: 0.5 KL(p || m) + 0.5 KL(q || m), m =
    (p + q) / 2, with 0 log 0 = 0; 0 where either side is all zero (an empty section has no distribution to differ from)"""
    p, q = np.broadcast_arrays(np.asarray(p, np.float64), np.asarray(q, np.float64))
    m = 0.5 * (p + q)

    def kl(a):
        ok = a > 0
        return np.sum(np.where(ok, a * np.log2(np.where(ok, a, 1.0) / np.where(ok, m, 1.0)), 0.0), axis=-1)
    both = (p.sum(axis=-1) > 0) & (q.sum(axis=-1) > 0)
    return np.where(both, np.clip(0.5 * kl(p) + 0.5 * kl(q), 0.0, 1.0), 0.0)


class RollStats:
    """What profile() returns.  table: int64 [N, S], the row of every piece as clv_roll_stats wrote it; lengths: the pieces'
    frames; width, max_duration, low: the call's; tonics: [N] pitch classes (-1: unknown, counted as 0) or None."""

    def __init__(self, table, lengths, width, max_duration, low=21, tonics=None):
        self.table = np.asarray(table, np.int64)
        self.lengths = [int(p) for p in lengths]
        self.width, self.max_duration, self.low = int(width), int(max_duration), int(low)
        self.tonics = None if tonics is None else [int(t) for t in tonics]
        self._at, at = {}, 0
        for name, n in section_bins(self.width, self.max_duration).items():
            self._at[name] = (at, n)
            at += n
        if self.table.ndim != 2 or self.table.shape != (len(self.lengths), at):
            raise ValueError("the table must be [%d, %d], got %s" % (len(self.lengths), at, self.table.shape))

    def __len__(self):
        return len(self.lengths)

    def section(self, name):
        """a view [N, bins] of the table"""
        if name not in self._at:
            raise ValueError("no section %r: one of %s" % (name, ", ".join(SECTIONS)))
        at, n = self._at[name]
        return self.table[:, at:at + n]

    def pooled(self, name=None):
        """the sum over the pieces: [bins] of a section, or the whole row [S] without a name"""
        return (self.table if name is None else self.section(name)).sum(axis=0)

    def distribution(self, name):
        """the pooled section, normalised, float64; all zeros for an empty section"""
        return _normalised(self.pooled(name))

    def means(self):
        """the batch in six numbers.  notes_per_frame; empty_frames, the share of frames without a note; note_length, the
        mean length of a note in frames -- an UNDERESTIMATE when the last duration bin is occupied, which holds every
        longer note at max_duration (note_length_clipped is the share of the notes in that bin); change, the mean number of
        cells that differ between consecutive frames (clipped at 16 per pair); span, the mean distance of the outer voices
        over the non-empty frames; in_scale, the share of the sounding cells on the degrees 0, 2, 4, 5, 7, 9, 11 of the
        tonics' major scales.  A figure without a count under it is 0."""
        mean = lambda h: float(np.dot(h, np.arange(len(h))) / h.sum()) if h.sum() else 0.0
        voices, dur, deg = self.pooled('voices'), self.pooled('duration'), self.pooled('degree')
        frames, cells = int(voices.sum()), int(self.pooled('pitch').sum())
        return dict(frames=frames,
                    notes_per_frame=cells / frames if frames else 0.0,
                    empty_frames=float(voices[0]) / frames if frames else 0.0,
                    note_length=float(np.dot(dur, np.arange(1, len(dur) + 1)) / dur.sum()) if dur.sum() else 0.0,
                    note_length_clipped=float(dur[-1]) / float(dur.sum()) if dur.sum() else 0.0,
                    change=mean(self.pooled('change')), span=mean(self.pooled('span')),
                    in_scale=float(deg[list(IN_SCALE)].sum()) / float(deg.sum()) if deg.sum() else 0.0)

    def divergence_to(self, other):
        """[N, sections]: the Jensen-Shannon divergence (bits) of every piece's own distribution to the pooled distribution
        of `other`, section by section in SECTIONS' order -- the odd sample stands out"""
        _same_shape(self, other)
        return np.stack([js_divergence(_normalised(self.section(name)), other.distribution(name)[None, :])
                         for name in SECTIONS], axis=1)

    def to_json(self):
        return dict(width=self.width, max_duration=self.max_duration, low=self.low, lengths=list(self.lengths),
                    tonics=self.tonics, sections={name: list(self._at[name]) for name in SECTIONS},
                    table=self.table.tolist(), pooled={name: self.pooled(name).tolist() for name in SECTIONS},
                    means=self.means())


def _same_shape(a, b):
    if (a.width, a.max_duration) != (b.width, b.max_duration):
        raise ValueError("the two profiles differ in width or max_duration: (%d, %d) and (%d, %d)"
                         % (a.width, a.max_duration, b.width, b.max_duration))


def compare(a, b):
    """two RollStats of the same width and max_duration against each other: per section the Jensen-Shannon divergence of
    the pooled distributions in bits (0: the same, 1: disjoint) and their overlap sum(min(p, q)) (1: the same, 0:
    disjoint), and both sides' means().  float64 on the host: the tables are a few hundred numbers."""
    _same_shape(a, b)
    out = dict(divergence={}, overlap={}, means_a=a.means(), means_b=b.means())
    for name in SECTIONS:
        p, q = a.distribution(name), b.distribution(name)
        out['divergence'][name] = float(js_divergence(p, q))
        out['overlap'][name] = float(np.minimum(p, q).sum())
    return out


def tonic_of(key_map, cls):
    """the pitch class 0..11 of class index `cls` of a data set's key_map (name -> index), through augment.parse_key; a minor
    key is folded onto its relative major (three semitones up), whose scale the natural minor shares -- so in_scale needs
    no mode.  None or -1 (no label) gives -1, unknown."""
    from .augment import parse_key
    if cls is None or int(cls) < 0:
        return -1
    for name, idx in key_map.items():
        if int(idx) == int(cls):
            pc, minor = parse_key(name)
            return (pc + 3) % 12 if minor else pc
    raise ValueError("the key map has no class %d" % int(cls))


def _check_tonics(tonics, N):
    if tonics is None:
        return None
    t = np.asarray([-1 if v is None else v for v in tonics])
    if t.shape != (N,) or t.dtype.kind not in 'iu' or np.any(t < -1) or np.any(t > 11):
        raise ValueError("tonics must hold one pitch class in 0..11 (or -1: unknown) per piece: %d integers" % N)
    return t.astype(np.int32)


def profile(pieces, tonics=None, max_duration=32, low=21, device='cuda:0'):
    """The texture histograms of every piece.  pieces: a list of binary [P_n, D] rolls of any lengths, or one [N, P, D]
    array, D <= 116 -- or a uint8 CUDA tensor [N, P, D] (any non-zero byte sounds), which is used where it lies, without a
    trip through the host.  tonics: None, or per piece the pitch class 0..11 of its key (-1 or None: unknown, counted as
    0) -- the reference point of `degree`; max_duration: the bins of `duration`, 1..64, longer notes in the last; low: the
    MIDI number of note 0.  Returns a RollStats.  ValueError for rolls that are not 0 / 1, a wrong or too large width, no
    piece, a max_duration, low or tonics out of range."""
    from .novelty import _int_in, _width
    Lmax, low = _int_in('max_duration', max_duration, 1, MAX_DURATION), _int_in('low', low, 0, 127)
    on_device = not isinstance(pieces, (np.ndarray, list, tuple)) and hasattr(pieces, 'is_cuda')
    if on_device:
        import torch
        if pieces.dim() != 3 or pieces.dtype != torch.uint8 or not pieces.is_cuda:
            raise ValueError("a tensor of pieces must be a uint8 CUDA tensor [N, P, D], got %s %s on %s"
                             % (pieces.dtype, tuple(pieces.shape), pieces.device))
        N, P, D = (int(v) for v in pieces.shape)
        if N < 1:
            raise ValueError("no pieces")
        lengths = [P] * N
    else:
        D = _width(pieces)
    if not 1 <= D <= MAX_WIDTH:
        raise ValueError("frames must be 1..%d notes wide, got %d" % (MAX_WIDTH, D))
    if not on_device:
        roll_np, lengths = pack_pieces(pieces, D)
        N = len(lengths)
    if N > MAX_PIECES:
        raise ValueError("%d pieces; the limit is %d" % (N, MAX_PIECES))
    ton = _check_tonics(tonics, N)

    import torch
    from . import ops
    dev = pieces.device if on_device else torch.device(device)
    with torch.cuda.device(dev):
        if on_device:
            roll = pieces.contiguous().view(N * P, D)
            off = torch.arange(N + 1, dtype=torch.int64, device=dev) * P
        else:
            roll = torch.as_tensor(roll_np, device=dev) if roll_np.size else None
            off = torch.as_tensor(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), device=dev)
        F = sum(lengths)
        table = torch.empty(N, ops.roll_stats_columns(D, Lmax), dtype=torch.int64, device=dev)
        ops.roll_stats(N, D, Lmax, low, F, roll if F else None, off, None if ton is None else torch.as_tensor(ton, device=dev),
                       table)
        table = table.cpu().numpy()
    return RollStats(table, lengths, D, Lmax, low, None if ton is None else ton.tolist())


# ---- the audit of the two sample.py tools (--stats, --stats_max_duration N) --------------------------------------------------
def describe(m):
    return ("%d frames: %.3f notes per frame, %.4f of the frames empty, notes last %.2f frames%s, %.3f cells change per "
            "frame, span %.2f, in scale %.4f"
            % (m['frames'], m['notes_per_frame'], m['empty_frames'], m['note_length'],
               " (at least: %.4f of them reach the last bin)" % m['note_length_clipped'] if m['note_length_clipped'] else "",
               m['change'], m['span'], m['in_scale']))


def describe_compare(c):
    return ", ".join("%s %.4f" % (name, c['divergence'][name]) for name in SECTIONS)


def audit_samples(rolls, args, keys=None, device='cuda:0'):
    """--stats [--stats_max_duration N] of cl_vae/sample.py and cl_vrnn/sample.py: the means of the rolls' texture, their
    compare() against the songs of the training split, and the same for the test split's songs as the baseline (a sample
    further from the training set than held-out music is suspect).  keys: per sample the class index of the label it was
    generated under (None where unknown) or None -- the tonic of `degree` and in_scale; the songs take theirs from
    split_songs.  Returns (the samples' RollStats, the training songs', the test songs'), or None without the flag or
    without a roll."""
    if not getattr(args, 'stats', False):
        return None
    from .keytrack import split_songs
    from .novelty import flatten_rolls
    Lmax = getattr(args, 'stats_max_duration', None) or 32
    rolls = flatten_rolls(rolls)
    if not rolls:
        return None
    train, train_keys, key_map = split_songs(args.train_file, 'train')
    test, test_keys, _ = split_songs(args.train_file, 'test')
    known = keys is not None and len(keys) == len(rolls)
    tonics = [tonic_of(key_map, k) for k in keys] if known else None
    st = profile(rolls, tonics, max_duration=Lmax, device=device)
    tr = profile(train, [tonic_of(key_map, k) for k in train_keys], max_duration=Lmax, device=device)
    te = profile(test, [tonic_of(key_map, k) for k in test_keys], max_duration=Lmax, device=device)
    print("stats: %d samples, note lengths up to %d frames, %s" % (len(st), Lmax, "degrees from the labels' tonics" if known
                                                                  else "no labels: degrees are pitch classes, C = 0"))
    print("samples' means: " + describe(st.means()))
    print("samples against %d training songs, divergence in bits: %s" % (len(tr), describe_compare(compare(st, tr))))
    div = st.divergence_to(tr)
    for n in range(len(st)):
        worst = int(np.argmax(div[n]))
        print("sample %d: largest divergence %.4f in %s" % (n, div[n, worst], SECTIONS[worst]))
    print("baseline, %d test songs against the training songs: %s" % (len(te), describe_compare(compare(te, tr))))
    print("baseline's means: " + describe(te.means()))
    return st, tr, te


# ---- python -m clvae_amd.stats ------------------------------------------------------------------------------------------------
def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog='python -m clvae_amd.stats',
                                description="roll statistics audit: the texture histograms of one split's songs (or of saved "
                                            "rolls) compared with another split's")
    p.add_argument('--train_file', type=str, required=True, help='file of training data (.pickle)')
    p.add_argument('--split', type=str, default='test', choices=SPLIT_CHOICES, help='split whose songs are profiled')
    p.add_argument('--against', type=str, default='train', choices=SPLIT_CHOICES, help='split they are compared with')
    p.add_argument('--rolls', type=str, default='', help='profile this saved [N, P, 88] array (.npy) instead of --split')
    p.add_argument('--max_duration', type=int, default=32, help='note lengths are counted up to this many frames (1..64)')
    p.add_argument('--out', type=str, default='', help='write the results as JSON to this file')
    return p


def main(argv=None):
    import json
    from .keytrack import split_songs
    p = build_parser()
    args = p.parse_args(argv)
    if not 1 <= args.max_duration <= MAX_DURATION:
        p.error('--max_duration in 1..%d' % MAX_DURATION)
    corpus, corpus_keys, key_map = split_songs(args.train_file, args.against)
    if args.rolls:
        queries, tonics, what = (np.load(args.rolls) > 0).astype(np.uint8), None, args.rolls
    else:
        queries, keys, _ = split_songs(args.train_file, args.split)
        tonics, what = [tonic_of(key_map, k) for k in keys], args.split
    a = profile(queries, tonics, max_duration=args.max_duration)
    b = profile(corpus, [tonic_of(key_map, k) for k in corpus_keys], max_duration=args.max_duration)
    cmp_ = compare(a, b)
    div = a.divergence_to(b)
    res = dict(query=what, against=args.against, max_duration=args.max_duration, n_songs=len(a), n_corpus=len(b),
               compare=cmp_, profile=a.to_json(), against_pooled={name: b.pooled(name).tolist() for name in SECTIONS},
               divergence_to=div.tolist())
    print("%s: %s" % (what, describe(cmp_['means_a'])))
    print("%s: %s" % (args.against, describe(cmp_['means_b'])))
    print("divergence in bits, %s against %s: %s" % (what, args.against, describe_compare(cmp_)))
    print("overlap: " + ", ".join("%s %.4f" % (name, cmp_['overlap'][name]) for name in SECTIONS))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(res, f, indent=1, sort_keys=True)
    return res


if __name__ == '__main__':
    main()
