"""numpy reference of the novelty audit, written from the contract of clv_roll_nearest in include/clvae.h;
it imports nothing of the package.

For every window of W frames of every query piece (window j starts at frame j * hop) the candidate (s, corpus window)
with the smallest (dist, rank(s), g): s in -S .. S among the shifts that keep every sounding note of the query window
inside 0 .. D-1, the corpus window at any offset of any corpus piece but exclude[n], no window across two pieces,
dist = sum_t sum_d [Q[a + t, d - s] != C[b + t, d]], rank: 0, -1, +1, -2, +2, ..., g = the global corpus frame.

nearest():       per-shift frame distances as a matrix product, |q| + |c| - 2 q.c, W shifted slices summed, masks, argmin.
nearest_loops(): the definition, loop by loop (tiny inputs only).
Both return per query piece n a triple of arrays (dist [J_n] int32, shift [J_n] int32, cframe [J_n] int64), (-1, 0, -1)
where a window has no candidate."""
import numpy as np


def n_windows(P, W, hop):
    return max(0, (P - W) // hop + 1)


def rank(s):
    return 0 if s == 0 else (-2 * s - 1 if s < 0 else 2 * s)


def shifts_in_rank_order(S):
    return sorted(range(-S, S + 1), key=rank)


def offsets(pieces):
    return np.concatenate([[0], np.cumsum([p.shape[0] for p in pieces])]).astype(np.int64)


def shifted(Q, s):
    """Q'[t, d] = Q[t, d - s], 0 where d - s is outside 0 .. D-1"""
    out = np.zeros_like(Q)
    D = Q.shape[1]
    if s >= 0:
        out[:, s:] = Q[:, :D - s]
    else:
        out[:, :D + s] = Q[:, -s:]
    return out


def allowed(window, s):
    """every sounding note d of the window keeps 0 <= d + s < D"""
    notes = np.flatnonzero(window.any(axis=0))
    return notes.size == 0 or (notes[0] + s >= 0 and notes[-1] + s < window.shape[1])


def notes_per_window(piece, W, hop):
    """the number of sounding notes (set cells) of every window of a piece"""
    J = n_windows(piece.shape[0], W, hop)
    per_frame = np.concatenate([[0], np.cumsum(np.asarray(piece, np.int64).sum(axis=1))])
    starts = np.arange(J) * hop
    return (per_frame[starts + W] - per_frame[starts]).astype(np.int64)


def nearest(queries, corpus, W, hop, S, exclude=None):
    queries = [np.asarray(q, np.uint8) for q in queries]
    corpus = [np.asarray(c, np.uint8) for c in corpus]
    D = (queries + corpus)[0].shape[1]
    c_off = offsets(corpus)
    Fc = int(c_off[-1])
    C = np.concatenate(corpus, 0).astype(np.float64) if Fc else np.zeros((0, D))
    nC = Fc - W + 1                                            # corpus window starts, as one string of frames
    piece_of = np.repeat(np.arange(len(corpus)), [c.shape[0] for c in corpus])
    ends = c_off[1:][piece_of] if Fc else np.zeros(0, np.int64)
    inside = (np.arange(Fc) + W <= ends)[:max(nC, 0)]          # the window at g stays in its piece
    csum = C.sum(1)
    out = []
    for n, Q in enumerate(queries):
        J = n_windows(Q.shape[0], W, hop)
        dist, shift, cframe = np.full(J, -1, np.int32), np.zeros(J, np.int32), np.full(J, -1, np.int64)
        if J == 0 or nC <= 0:
            out.append((dist, shift, cframe))
            continue
        ok = inside.copy()
        if exclude is not None and exclude[n] >= 0:
            ok &= piece_of[:nC] != exclude[n]
        starts = np.arange(J) * hop
        nA = Q.shape[0] - W + 1
        for s in shifts_in_rank_order(S):
            Qs = shifted(Q, s).astype(np.float64)
            F = np.rint(Qs.sum(1)[:, None] + csum[None, :] - 2.0 * (Qs @ C.T)).astype(np.int32)     # [P, Fc] frame distances
            Wd = np.zeros((nA, nC), np.int32)
            for t in range(W):
                Wd += F[t:t + nA, t:t + nC]
            Wd = Wd[starts]
            Wd[:, ~ok] = np.iinfo(np.int32).max
            best, arg = Wd.min(1), Wd.argmin(1)                # argmin: the first, i.e. the lowest g
            for j in range(J):
                if best[j] == np.iinfo(np.int32).max or not allowed(Q[starts[j]:starts[j] + W], s):
                    continue
                if dist[j] < 0 or best[j] < dist[j]:           # strictly: an earlier shift has the lower rank
                    dist[j], shift[j], cframe[j] = best[j], s, arg[j]
        out.append((dist, shift, cframe))
    return out


def nearest_loops(queries, corpus, W, hop, S, exclude=None):
    c_off = offsets(corpus)
    out = []
    for n, Q in enumerate(queries):
        P, D = Q.shape
        rows = []
        for j in range(n_windows(P, W, hop)):
            a = j * hop
            best = None
            for s in range(-S, S + 1):
                if any(Q[a + t, d] and not 0 <= d + s < D for t in range(W) for d in range(D)):
                    continue
                for m, Cm in enumerate(corpus):
                    if exclude is not None and exclude[n] == m:
                        continue
                    for b in range(Cm.shape[0] - W + 1):
                        dist = 0
                        for t in range(W):
                            for d in range(D):
                                q = Q[a + t, d - s] if 0 <= d - s < D else 0
                                dist += int(bool(q) != bool(Cm[b + t, d]))
                        key = (dist, rank(s), int(c_off[m]) + b)
                        if best is None or key < best[0]:
                            best = (key, s)
            rows.append((-1, 0, -1) if best is None else (best[0][0], best[1], best[0][2]))
        r = np.asarray(rows, np.int64).reshape(-1, 3)
        out.append((r[:, 0].astype(np.int32), r[:, 1].astype(np.int32), r[:, 2].astype(np.int64)))
    return out


def song_frame(cframe, c_off):
    """global corpus frames -> (piece, frame in the piece); -1 stays -1.  Pieces without frames own no frame."""
    cframe = np.asarray(cframe, np.int64)
    c_off = np.asarray(c_off, np.int64)
    song = np.searchsorted(c_off, cframe, side='right') - 1
    song = np.where(cframe < 0, -1, song)
    frame = np.where(cframe < 0, -1, cframe - c_off[np.maximum(song, 0)])
    return song.astype(np.int64), frame.astype(np.int64)
