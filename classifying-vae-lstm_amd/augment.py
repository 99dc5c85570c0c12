"""Transposition augmentation of the training windows (not in the reference).

Shifting every note of a window by s semitones gives the same music in another key: the frames move by s positions along
the 88 notes and the key label moves with them.  `TransposePlan` says, per window of the training set, which shifts in
-K..K are allowed -- every sounding note of the window stays on the keyboard, and the key it lands in is a class of the
model -- and, per shift, which class each class becomes.  The step's staging launch (csrc/transpose_aug.hip,
ops.gather_transposed; TrainStep.bind_batches(augment=plan)) draws one allowed shift per row and per step and applies it
while it assembles the mini-batch: nothing is materialised, nothing is staged from the host.

    plan = TransposePlan.build([P.y_train, P.x_train], P.train_song_keys, P.key_map, semitones=6)
    model.fit(x, y, ..., augment=plan)

`transpose_rows` states in numpy what the launch does to a batch once the shifts are known.
"""
import numpy as np

MAX_SEMITONES = 12
_LETTERS = {'c': 0, 'd': 2, 'e': 4, 'f': 5, 'g': 7, 'a': 9, 'b': 11}


def parse_key(name):
    """(pitch class 0..11, is_minor) of a key name as the data set's pickles spell them: a letter, then any number of '#' (up a
    semitone) or '-' (down a semitone); upper case = major, lower case = minor.  'C-' is (11, False), 'f#' is (6, True)."""
    name = str(name)
    if not name or name[0].lower() not in _LETTERS or any(ch not in '#-' for ch in name[1:]):
        raise ValueError("not a key name: %r" % (name,))
    pc = _LETTERS[name[0].lower()] + name.count('#') - name.count('-')
    return pc % 12, name[0].islower()


def class_targets(key_map, semitones, n_classes=None):
    """int32 [(2K+1), C]: entry [j, c] is the class that class c becomes under the shift j - K -- the class of the same mode
    whose pitch class is pc(c) + s mod 12 (the lowest index among enharmonic duplicates), -1 when the model has none.  Classes
    without a name in key_map (n_classes > the map's highest index + 1) map to themselves under shift 0 only."""
    K = int(semitones)
    C = int(n_classes) if n_classes is not None else max(key_map.values()) + 1
    keys = {}                                   # class -> (pc, minor)
    for name, c in key_map.items():
        if int(c) < C:
            keys[int(c)] = parse_key(name)
    first = {}                                  # (pc, minor) -> lowest class
    for c in sorted(keys):
        first.setdefault(keys[c], c)
    out = np.full((2 * K + 1, C), -1, np.int32)
    for c in range(C):
        out[K, c] = c
        if c in keys:
            pc, minor = keys[c]
            for j in range(2 * K + 1):
                if j != K:
                    out[j, c] = first.get(((pc + j - K) % 12, minor), -1)
    return out


def note_ranges(windows):
    """(lo, hi) int64 [n]: the lowest and the highest sounding note over all frames of window i of every view in `windows`
    (utils.pianoroll.Windows of the same n rows; or arrays [n, T, D] / [n, D]); lo = D and hi = -1 for a silent window.  One
    pass over each frame store and one sliding minimum / maximum per view: no loop over windows."""
    from numpy.lib.stride_tricks import sliding_window_view
    lo = hi = None
    for w in windows:
        if w is None:
            continue
        if hasattr(w, 'store') and hasattr(w, 'starts'):
            on = np.asarray(w.store) != 0
            D = on.shape[1]
            f_lo = np.where(on.any(axis=1), on.argmax(axis=1), D)
            f_hi = np.where(on.any(axis=1), D - 1 - on[:, ::-1].argmax(axis=1), -1)
            at = np.asarray(w.starts, np.int64) + int(w.t0)
            w_lo = sliding_window_view(f_lo, int(w.length)).min(axis=1)[at]
            w_hi = sliding_window_view(f_hi, int(w.length)).max(axis=1)[at]
        else:
            a = np.asarray(w)
            on = (a != 0).reshape(a.shape[0], -1, a.shape[-1])
            D = on.shape[2]
            notes = on.any(axis=1)
            w_lo = np.where(notes.any(axis=1), notes.argmax(axis=1), D)
            w_hi = np.where(notes.any(axis=1), D - 1 - notes[:, ::-1].argmax(axis=1), -1)
        lo = w_lo if lo is None else np.minimum(lo, w_lo)
        hi = w_hi if hi is None else np.maximum(hi, w_hi)
    if lo is None:
        raise ValueError("no windows")
    return lo.astype(np.int64), hi.astype(np.int64)


class TransposePlan:
    """allowed: uint32 [n], bit j of entry i set = window i may be shifted by j - K semitones; class_map: int32 [(2K+1) * C],
    entry j * C + c = the class that class c becomes under shift j - K, or -1; K: the largest shift.  numpy arrays as
    built, device tensors after .to(device)."""

    def __init__(self, allowed, class_map, K):
        K = int(K)
        if not 0 <= K <= MAX_SEMITONES:
            raise ValueError("semitones must be in 0..%d, got %r" % (MAX_SEMITONES, K))
        self.allowed, self.class_map, self.K = allowed, class_map, K

    @classmethod
    def build(cls, windows, labels, key_map, semitones=6, n_classes=None):
        """windows: the views fit() will read (x, history, target; a list of Windows or arrays with the same rows) -- a window's
        span is the union of their frames; labels: the class of every window (integers [n], or one-hot rows [n, C]);
        key_map: {key name: class}.  Shift s is allowed for a window when every sounding note of its span stays inside
        0..D-1 and the window's class has a target in key_map (class_targets); shift 0 always is."""
        K = int(semitones)
        if not 0 <= K <= MAX_SEMITONES:
            raise ValueError("semitones must be in 0..%d, got %r" % (MAX_SEMITONES, K))
        windows = [w for w in (windows if isinstance(windows, (list, tuple)) else [windows]) if w is not None]
        labels = np.asarray(labels)
        if labels.ndim == 2:
            if n_classes is None:
                n_classes = labels.shape[1]
            labels = labels.argmax(axis=1)
        labels = labels.astype(np.int64)
        cmap = class_targets(key_map, K, n_classes)
        C = cmap.shape[1]
        lo, hi = note_ranges(windows)
        if len(labels) != len(lo) or (len(labels) and (labels.min() < 0 or labels.max() >= C)):
            raise ValueError("labels: one class in 0..%d per window (%d windows)" % (C - 1, len(lo)))
        D = int((windows[0].store if hasattr(windows[0], 'store') else np.asarray(windows[0])).shape[-1])
        s = np.arange(-K, K + 1, dtype=np.int64)[None, :]
        ok = (lo[:, None] + s >= 0) & (hi[:, None] + s <= D - 1)          # (a silent window: D + s >= 0, -1 + s <= D - 1)
        ok &= cmap[:, labels].T >= 0
        ok[:, K] = True
        allowed = (ok.astype(np.uint32) << np.arange(2 * K + 1, dtype=np.uint32)[None, :]).sum(axis=1, dtype=np.uint32)
        return cls(allowed, cmap.reshape(-1), K)

    def to(self, device):
        """The plan with both arrays on `device` (uploaded once; a plan already there is returned as it is)."""
        import torch
        if isinstance(self.allowed, torch.Tensor):
            return TransposePlan(self.allowed.to(device), self.class_map.to(device), self.K)
        allowed = torch.as_tensor(np.ascontiguousarray(self.allowed, np.uint32).view(np.int32), device=device)
        return TransposePlan(allowed, torch.as_tensor(np.ascontiguousarray(self.class_map, np.int32), device=device), self.K)

    def counts(self):
        """how many shifts every window admits (numpy plans)"""
        a = np.ascontiguousarray(self.allowed, np.uint32)
        return np.unpackbits(a.view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1)


def shift_frames(frames, shifts):
    """frames [n, ..., D] moved along the last axis by shifts[i] notes per row i: out[p] = in[p - s] where 0 <= p - s < D,
    else 0."""
    frames = np.asarray(frames)
    out = np.zeros_like(frames)
    D = frames.shape[-1]
    for i, s in enumerate(np.asarray(shifts).astype(int)):
        if s >= 0:
            out[i, ..., s:] = frames[i, ..., :D - s]
        else:
            out[i, ..., :D + s] = frames[i, ..., -s:]
    return out


def transpose_rows(frames, labels, shifts, class_map, K):
    """What the staging launch leaves of a batch whose shifts are known: (frames shifted by shifts[i] per row, labels
    [n, C] with w_out[i, class_map[(s + K) * C + c]] += labels[i, c] for every c whose entry is >= 0).  `frames` may be a
    list of arrays (current, history, target): all of a row move by the row's one shift."""
    many = isinstance(frames, (list, tuple))
    moved = [shift_frames(f, shifts) for f in (frames if many else [frames])]
    labels = np.asarray(labels, np.float32)
    C = labels.shape[1]
    cmap = np.asarray(class_map).reshape(2 * int(K) + 1, C)
    w = np.zeros_like(labels)
    for i, s in enumerate(np.asarray(shifts).astype(int)):
        for c in range(C):
            t = cmap[s + int(K), c]
            if t >= 0:
                w[i, t] += labels[i, c]
    return (moved if many else moved[0]), w
