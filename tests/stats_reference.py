"""numpy reference of the roll statistics audit, written from the contract of clv_roll_stats in include/clvae.h (DESIGN.md
24): plain loops over pieces, frames and notes on the 0 / 1 arrays themselves -- no packed frames, no bit tricks, nothing of
csrc/stats.hip.  tests/test_stats_reference.py anchors it on rolls small enough to count by hand."""
import numpy as np

V, C, M = 16, 16, 24                              # CLV_STATS_VOICES, CLV_STATS_CHANGE, CLV_STATS_STEP
NAMES = ('pitch', 'degree', 'voices', 'interval', 'duration', 'change', 'top_step', 'bottom_step', 'span')
IN_SCALE = (0, 2, 4, 5, 7, 9, 11)


def bins(D, Lmax):
    return dict(pitch=D, degree=12, voices=V + 1, interval=D, duration=Lmax, change=C + 1, top_step=2 * M + 1,
                bottom_step=2 * M + 1, span=D)


def columns(D, Lmax):
    return sum(bins(D, Lmax).values())


def sections(D, Lmax):
    """name -> (first column, bins), in the row's order"""
    out, at = {}, 0
    b = bins(D, Lmax)
    for name in NAMES:
        out[name] = (at, b[name])
        at += b[name]
    return out


def offsets(pieces):
    return np.concatenate([[0], np.cumsum([p.shape[0] for p in pieces])]).astype(np.int64)


def piece_row(piece, D, Lmax, low=21, tonic=0):
    """the row of one piece [P, D] (any non-zero cell sounds) as a dictionary of int64 arrays, one per section"""
    on = np.asarray(piece) != 0
    P = on.shape[0]
    assert on.shape == (P, D)
    tonic = 0 if tonic is None or tonic < 0 else int(tonic)
    r = {name: np.zeros(n, np.int64) for name, n in bins(D, Lmax).items()}
    notes = [[d for d in range(D) if on[t, d]] for t in range(P)]
    for t in range(P):
        f = notes[t]
        for d in f:
            r['pitch'][d] += 1
            r['degree'][(d + low - tonic) % 12] += 1
        r['voices'][min(len(f), V)] += 1
        for i in range(len(f)):
            for j in range(i + 1, len(f)):
                r['interval'][f[j] - f[i]] += 1
        if f:
            r['span'][max(f) - min(f)] += 1
        if t >= 1:
            g = notes[t - 1]
            differ = sum(1 for d in range(D) if on[t, d] != on[t - 1, d])
            r['change'][min(differ, C)] += 1
            if f and g:
                r['top_step'][min(max(max(f) - max(g), -M), M) + M] += 1
                r['bottom_step'][min(max(min(f) - min(g), -M), M) + M] += 1
    for d in range(D):                            # the runs of every note, inside this piece only
        run = 0
        for t in range(P + 1):
            if t < P and on[t, d]:
                run += 1
            elif run:
                r['duration'][min(run, Lmax) - 1] += 1
                run = 0
    return r


def table(pieces, D, Lmax, low=21, tonics=None):
    """int64 [N, columns(D, Lmax)]: the table of clv_roll_stats for the pieces (a list of [P_n, D] arrays)"""
    out = np.zeros((len(pieces), columns(D, Lmax)), np.int64)
    for n, p in enumerate(pieces):
        r = piece_row(p, D, Lmax, low, None if tonics is None else tonics[n])
        out[n] = np.concatenate([r[name] for name in NAMES])
    return out
