"""No GPU: transposition augmentation on the host side -- the plan builder against a brute-force loop, key names,
the shift counts of the JSB data sets, the new entry in the header, _lib.SIGNATURES and ops, its refusals on host pointers, the
reserved Philox stream and the --transpose flag."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import clvae_amd  # noqa: F401
import transpose_reference as TR
from clvae_amd import _lib, augment, cli, ops, trainer
from clvae_amd.utils.pianoroll import PianoData, Windows
from helpers import write_jsb_pickle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
D = 88


# ---------------------------------------------------------------- the plan --
def _songs():
    """One frame store of five 'songs' and the windows (T = 3 frames of x behind one history frame) that start in it"""
    rng = np.random.default_rng(4)
    T = 3
    songs = []
    a = np.zeros((8, D), np.uint8); a[:, 40] = 1; a[2, 0] = 1                  # note 0 in one frame
    b = np.zeros((8, D), np.uint8); b[:, 50] = 1; b[5, 87] = 1                 # note 87 in one frame
    c = np.zeros((9, D), np.uint8); c[7:, 30] = 1                              # windows 0..2 of it are silent
    d = np.zeros((8, D), np.uint8); d[:, 44] = 1; d[0, 3] = 1; d[0, 85] = 1    # frame 0 is a HISTORY frame only (window 0)
    e = (rng.random((10, D)) < 0.05).astype(np.uint8); e[:, :9] = 0; e[:, 80:] = 0
    starts, labels, first = [], [], 0
    for k, s in enumerate((a, b, c, d, e)):
        songs.append(s)
        n = s.shape[0] - (T + 1) + 1
        starts += list(first + np.arange(n))
        labels += [k % 4] * n
        first += s.shape[0]
    store = np.vstack(songs)
    starts = np.array(starts, np.int64)
    x, hist = Windows(store, starts, 1, T), Windows(store, starts, 0, T)
    return store, starts, T, x, hist, np.array(labels)


KEY_MAP = {'C': 0, 'G': 1, 'a': 2, 'E-': 3}       # majors at 0, 7, 3; one minor at 9


def _brute(store, starts, T, labels, cmap, K, with_history):
    out = []
    for i, st in enumerate(starts):
        frames = store[st + (0 if with_history else 1): st + T + 1]
        notes = np.nonzero(frames.any(axis=0))[0]
        m = 0
        for j in range(2 * K + 1):
            s = j - K
            fits = all(0 <= n + s <= D - 1 for n in notes)
            if s == 0 or (fits and cmap[j, labels[i]] >= 0):
                m |= 1 << j
        out.append(m)
    return np.array(out, np.uint32)


@pytest.mark.parametrize("K", [0, 1, 6, 12])
def test_plan_builder_equals_a_brute_force_loop(K):
    store, starts, T, x, hist, labels = _songs()
    cmap = augment.class_targets(KEY_MAP, K)
    for views, with_history in (([x, hist], True), ([x], False), ([x, hist, x], True)):
        plan = augment.TransposePlan.build(views, labels, KEY_MAP, semitones=K)
        assert plan.K == K and plan.allowed.dtype == np.uint32 and plan.class_map.dtype == np.int32
        np.testing.assert_array_equal(plan.class_map, cmap.reshape(-1))
        np.testing.assert_array_equal(plan.allowed, _brute(store, starts, T, labels, cmap, K, with_history))
        assert ((plan.allowed >> K) & 1).all()
    # materialised arrays give the same plan as the views
    arr = augment.TransposePlan.build([np.asarray(x), np.asarray(hist)], np.eye(4)[labels], KEY_MAP, semitones=K)
    np.testing.assert_array_equal(arr.allowed, augment.TransposePlan.build([x, hist], labels, KEY_MAP, semitones=K).allowed)


def test_the_cases_the_synthetic_songs_were_written_for():
    store, starts, T, x, hist, labels = _songs()
    K = 12
    keys = {'C': 0, 'D-': 1, 'D': 2, 'E-': 3, 'E': 4, 'F': 5, 'F#': 6, 'G': 7, 'A-': 8, 'A': 9, 'B-': 10, 'B': 11}
    lab = np.zeros(len(starts), np.int64)                                        # every key exists: only the range binds
    full = (1 << 25) - 1
    with_h = augment.TransposePlan.build([x, hist], lab, keys, semitones=K).allowed
    without = augment.TransposePlan.build([x], lab, keys, semitones=K).allowed
    down = sum(1 << j for j in range(K))                                         # all shifts below 0
    up = sum(1 << j for j in range(K + 1, 2 * K + 1))
    assert with_h[0] & down == 0 and with_h[0] & up == up                        # song a, window 0 holds note 0: never down
    assert with_h[4] & down == down                                              # ... window 4 starts behind it
    assert with_h[5 + 2] & up == 0 and with_h[5] & up == up                      # song b: note 87 in its frame 5
    assert with_h[10] == full and with_h[11] == full and with_h[12] == full      # song c: silent windows take every shift
    assert with_h[16] == sum(1 << j for j in range(K - 3, K + 3))                # song d, window 0: notes 3 and 85 in the history frame
    assert without[16] == full                                                   # ... which alone holds them: without it, note 44 only
    assert with_h[17] == full


def test_plan_argument_errors():
    store, starts, T, x, hist, labels = _songs()
    for K in (-1, 13):
        with pytest.raises(ValueError):
            augment.TransposePlan.build([x], labels, KEY_MAP, semitones=K)
        with pytest.raises(ValueError):
            augment.TransposePlan(np.zeros(1, np.uint32), np.zeros(3, np.int32), K)
    with pytest.raises(ValueError):
        augment.TransposePlan.build([x], labels[:-1], KEY_MAP)
    with pytest.raises(ValueError):
        augment.TransposePlan.build([x], labels + 9, KEY_MAP)


def test_key_names():
    pk = augment.parse_key
    assert [pk(k) for k in 'CDEFGAB'] == [(p, False) for p in (0, 2, 4, 5, 7, 9, 11)]
    assert pk('C-') == (11, False) and pk('F-') == (4, False) and pk('B#') == (0, False) and pk('F#') == (6, False)
    assert pk('E-') == (3, False) and pk('e-') == (3, True) and pk('f#') == (6, True) and pk('a') == (9, True)
    assert pk('A--') == (7, False)
    for bad in ('', 'H', 'Cb', '#C', 'C major'):
        with pytest.raises(ValueError):
            pk(bad)
    km = {'C': 0, 'a': 1, 'B#': 2, 'A': 3, 'c': 4, 'e-': 5}
    m = augment.class_targets(km, 3)
    assert m.shape == (7, 6) and (m[3] == np.arange(6)).all()
    assert m[3 + 3, 3] == 0 and m[3 - 3, 0] == 3              # A + 3 = C: the LOWEST index of the enharmonic pair C / B#
    assert m[3 + 3, 1] == 4 and m[3 - 3, 4] == 1              # minors map only to minors: a + 3 = c, never C
    assert m[3 + 3, 4] == 5 and m[3 + 3, 0] == -1             # c + 3 = e-; C + 3 = E- major does not exist
    assert m[3 - 3, 2] == 3 and m[3 + 1, 0] == -1
    majors, minors = {0, 2, 3}, {1, 4, 5}
    for j in range(7):
        for c in range(6):
            if m[j, c] >= 0:
                assert (m[j, c] in minors) == (c in minors)
    wide = augment.class_targets({'C': 0, 'D': 1}, 2, n_classes=4)      # classes without a name stay where they are
    assert (wide[:, 2] == [-1, -1, 2, -1, -1]).all() and wide[4, 0] == 1 and wide[0, 1] == 0


@pytest.mark.parametrize("which,windows,counts", [('all', 10400, {10, 11}), ('Cs', 9800, {2})])
def test_shift_counts_of_the_jsb_data_sets(tmp_path, which, windows, counts):
    """seq_length 16, K = 6, the data as cl_vrnn/train.py --use_x_prev loads it"""
    f = write_jsb_pickle(which, str(tmp_path / "jsb.pickle"))
    P = PianoData(f, batch_size=200, seq_length=16, step_length=1, return_y_next=True, return_y_hist=True, squeeze_x=False,
                  squeeze_y=False, lazy=True)
    plan = augment.TransposePlan.build([P.y_train, P.x_train], P.train_song_keys, P.key_map, semitones=6)
    n = plan.counts()
    assert len(n) == windows and set(n.tolist()) == counts
    if which == 'all':
        assert 'B' not in P.key_map and 'F#' not in P.key_map          # what limits it: the two keys no class stands for
        lo, hi = augment.note_ranges([P.y_train, P.x_train])
        assert lo.min() == 15 and hi.max() == 65                        # the note range never binds


def test_transpose_rows_states_the_rule():
    rng = np.random.default_rng(2)
    X = (rng.random((5, 3, D)) < 0.1).astype(np.uint8)
    X[0, 0, 87] = X[1, 2, 0] = 1
    w = np.eye(4, dtype=np.float32)[[0, 1, 2, 3, 0]]
    K = 2
    cmap = augment.class_targets(KEY_MAP, K).reshape(-1)
    shifts = np.array([2, -2, 0, 1, -1])
    (Xs, Hs), ws = augment.transpose_rows([X, X[:, :1]], w, shifts, cmap, K)
    for i, s in enumerate(shifts):
        for t in range(3):
            np.testing.assert_array_equal(Xs[i, t], TR.shift_frame(X[i, t], int(s)))
        np.testing.assert_array_equal(Hs[i, 0], TR.shift_frame(X[i, 0], int(s)))
        want = np.zeros(4, np.float32)
        t = cmap.reshape(5, 4)[s + K, i % 4]
        if t >= 0:
            want[t] = 1
        np.testing.assert_array_equal(ws[i], want)


# ------------------------------------------------------- the entry point --
def test_entry_is_declared_and_bound(tmp_path):
    hdr = open(os.path.join(ROOT, 'include', 'clvae.h')).read()
    protos = dict(re.findall(r"\b(clv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)))
    i, p, i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    assert 'clv_gather_transposed' in protos
    assert _lib.SIGNATURES['clv_gather_transposed'] == (i, [i64, p, i64, i] + [p] * 13)
    args = lambda n: [a.split()[-1].lstrip('*') for a in protos[n].split(',')]
    plain = args('clv_gather_rows_multi')
    assert args('clv_gather_transposed') == plain[:-1] + ['draw', 'stream']          # the plain gather's list, plus the draw
    assert hasattr(_lib.lib(), 'clv_gather_transposed') and callable(ops.gather_transposed)
    assert _lib.ABI_VERSION == 610 and _lib.lib().clv_version() == 610
    mk = open(os.path.join(ROOT, 'classifying-vae-lstm_amd', 'csrc', 'Makefile')).read()
    assert 'transpose_aug.hip' in mk
    # ops.TransposeDraw against clv_transpose_draw as gcc lays it out
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "clvae.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(clv_transpose_draw));']
    for name, _ in ops.TransposeDraw._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(clv_transpose_draw, %s));' % (name, name))
    lines += ['  return 0;', '}']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I' + os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True, stdin=subprocess.DEVNULL)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, stdin=subprocess.DEVNULL).stdout
    for line in out.splitlines():
        what, val = line.split()
        if what == 'size':
            assert ctypes.sizeof(ops.TransposeDraw) == int(val)
        else:
            assert getattr(ops.TransposeDraw, what).offset == int(val), what


def test_the_reserved_stream():
    assert trainer.TRANSPOSE_STREAM == 0xFFFFFFF9 == TR.TRANSPOSE_STREAM
    streams = [trainer.IW_STREAM_W, trainer.IW_STREAM_Z, trainer.SMC_STREAM, trainer.SMC_W_STREAM, trainer.KEY_STREAM,
               trainer.GIBBS_STREAM, trainer.TRANSPOSE_STREAM]
    assert len(set(streams)) == 7 and trainer.TRANSPOSE_STREAM == min(streams) == trainer.GIBBS_STREAM - 1
    src = open(os.path.join(ROOT, 'classifying-vae-lstm_amd', 'csrc', 'transpose_aug.hip')).read()
    assert re.search(r"constexpr\s+uint32_t\s+TRANSPOSE_STREAM\s*=\s*0xFFFFFFF9u", src)


def _call(nseg=2, u8=(1, 0), row_elems=(2 * D, 10), chunk=(D, 0), out_ld=(D, 0), stride=(D, 0), offset=(0, 0), src=None, out=None,
          draw=None, **dk):
    """clv_gather_transposed on pointers that only look like device memory: a refused call never dereferences them"""
    p = 1 << 20
    n = max(nseg, 2)
    P, I, U = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int32 * n
    pad = lambda t, fill: tuple(t) + (fill,) * (n - len(t))
    kw = dict(allowed=p, class_map=p, K=6, C=10, D=D, label_seg=1, seed=1, first_row=0, step=0, step_dev=None, shift_out=None)
    kw.update(dk)
    d = ops.TransposeDraw(**kw) if draw is None else draw
    return _lib.lib().clv_gather_transposed(4, None, 0, nseg, P(*pad(src or (p,) * 2, p)), U(*pad(u8, 1)), P(*pad(out or (p,) * 2, p)),
                                            I(*pad(row_elems, 2 * D)), I(*pad(chunk, D)), I(*pad(out_ld, D)), I(*pad(stride, D)),
                                            I(*pad(offset, 0)), None, None, None, ctypes.byref(d) if d else None, None)


def test_refused_argument_lists_return_einval():
    assert _call(K=13) == EINVAL and _call(K=-1) == EINVAL
    assert _call(u8=(0, 0)) == EINVAL                                   # a float frame source
    assert _call(D=86) == EINVAL and _call(D=0) == EINVAL               # D not a multiple of 4
    assert _call(stride=(D + 2, 0)) == EINVAL and _call(offset=(3, 0)) == EINVAL
    assert _call(out_ld=(D + 2, 0)) == EINVAL and _call(out_ld=(D - 4, 0)) == EINVAL
    assert _call(allowed=None) == EINVAL and _call(class_map=None) == EINVAL
    assert _call(nseg=5) == EINVAL and _call(nseg=0) == EINVAL
    assert _call(draw=False) == EINVAL
    assert _call(chunk=(44, 0)) == EINVAL and _call(row_elems=(2 * D + 4, 10)) == EINVAL
    assert _call(u8=(1, 1)) == EINVAL and _call(C=9) == EINVAL and _call(label_seg=2) == EINVAL      # the label segment: float rows of C
    assert _call(src=((1 << 20) + 2, 1 << 20)) == EINVAL                # a store that is not 4-byte aligned
    assert _call(out=((1 << 20) + 4, 1 << 20)) == EINVAL                # a float output that is not 16-byte aligned


# -------------------------------------------------------------- the flag --
def test_transpose_flag_on_both_train_tools():
    assert [f.names[0] for f in cli.AUGMENT_FLAGS] == ['--transpose']
    assert cli.AUGMENT_FLAGS[0].default == 0 and cli.AUGMENT_FLAGS[0].kind is int
    import importlib
    for which in ('cl_vae', 'cl_vrnn'):
        TRN = importlib.import_module('clvae_amd.%s.train' % which)
        assert TRN.AUGMENT_FLAGS is cli.AUGMENT_FLAGS
        p = cli.parser_for(which + '.train', cli.OPTIMIZER_FLAGS + cli.AUGMENT_FLAGS)
        assert p.parse_args(['r']).transpose == 0
        assert p.parse_args(['r', '--transpose', '6']).transpose == 6
        for bad in ('-1', '13', 'x'):
            with pytest.raises(SystemExit):
                p.parse_args(['r', '--transpose', bad])
        assert not hasattr(TRN.build_parser().parse_args(['r']), 'transpose')      # the reference's surface stays the reference's
        src = open(TRN.__file__).read()
        assert re.search(r"parser_for\('%s\.train', [A-Z0-9_ +]*AUGMENT_FLAGS\)\.parse_args\(\)" % which, src)


def test_train_plan_builds_the_plan_only_when_asked(tmp_path):
    import types
    f = write_jsb_pickle('Cs', str(tmp_path / "jsb.pickle"))
    P = PianoData(f, batch_size=200, seq_length=16, step_length=1, return_y_next=True, return_y_hist=True, squeeze_x=False,
                  squeeze_y=False, lazy=True)
    w = np.eye(2)[P.train_song_keys]
    plan = types.SimpleNamespace(args=types.SimpleNamespace(transpose=0), rank=1)
    assert cli.TrainPlan.augment(plan, P, w) is None
    assert cli.TrainPlan.augment(types.SimpleNamespace(args=types.SimpleNamespace(), rank=1), P, w) is None
    plan.args.transpose = 6
    got = cli.TrainPlan.augment(plan, P, w)
    assert got.K == 6 and got.class_map.shape == (13 * 2,) and set(got.counts().tolist()) == {2}
    # cl_vae's flattened multi-frame rows have no semitone axis
    flat = types.SimpleNamespace(x_train=np.zeros((4, 60)), y_train=np.zeros((4, 60)))
    with pytest.raises(SystemExit):
        cli.TrainPlan.augment(types.SimpleNamespace(args=types.SimpleNamespace(transpose=6, seq_length=2), rank=1), flat, w)
