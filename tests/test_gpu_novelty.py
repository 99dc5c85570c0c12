"""GPU tests of the novelty audit against tests/novelty_reference.py: clv_roll_nearest's dist, shift and
cframe in exact equality over an edge grid of (D, W, S, hop), over a corpus that spans several workgroups and corpus tiles
(with the batch permuted, taken apart and the corpus permuted), with `exclude`, and novelty.nearest and the tools end to
end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import novelty_reference as NR
from helpers import ROOT, write_jsb_pickle

pytestmark = pytest.mark.gpu

# the tile constants of csrc/novelty.hip: a workgroup walks corpus tiles of RN_NT diagonals for RN_TQ window starts of one
# query piece; clv_roll_nearest launches about 4096 / Nq workgroups per query piece (at most one per corpus tile)
RN_NT, RN_TQ, WG_TARGET = 256, 32, 4096
TAIL = 64


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    return torch.device("cuda:0")


def test_the_tile_constants_are_the_kernels():
    src = open(os.path.join(ROOT, "classifying-vae-lstm_amd", "csrc", "novelty.hip")).read()
    assert "RN_NT = %d;" % RN_NT in src and "RN_TQ = %d;" % RN_TQ in src and "(%d + Nq - 1) / Nq" % WG_TARGET in src


def run(dev, queries, corpus, W, hop, S, exclude=None):
    """clv_roll_nearest through ops.roll_nearest -> per query piece (dist, shift, cframe); -7 behind every output"""
    from clvae_amd import ops
    D = (list(queries) + list(corpus))[0].shape[1]
    q_off, c_off = NR.offsets(queries), NR.offsets(corpus)
    counts = [NR.n_windows(q.shape[0], W, hop) for q in queries]
    w_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    Fq, Fc, Wq = int(q_off[-1]), int(c_off[-1]), int(w_off[-1])
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    cat = lambda ps, F: t(np.concatenate(ps, 0).astype(np.uint8)) if F else torch.zeros(1, D, dtype=torch.uint8, device=dev)
    dist = torch.full((Wq + TAIL,), -7, dtype=torch.int32, device=dev)
    shift = torch.full((Wq + TAIL,), -7, dtype=torch.int32, device=dev)
    cframe = torch.full((Wq + TAIL,), -7, dtype=torch.int64, device=dev)
    need = ops.roll_nearest_workspace_bytes(Fq, Fc, Wq)
    ws = torch.full((need + TAIL,), 0x5A, dtype=torch.uint8, device=dev)
    ops.roll_nearest(len(queries), len(corpus), W, hop, S, D, Fq, Fc, Wq, cat(queries, Fq), t(q_off), cat(corpus, Fc), t(c_off),
                     t(w_off), None if exclude is None else t(np.asarray(exclude, np.int32)), dist, shift, cframe, workspace=ws[:need])
    torch.cuda.synchronize()
    for x in (dist, shift, cframe):
        assert (x[Wq:] == -7).all(), "write behind an output"
    assert (ws[need:] == 0x5A).all(), "write behind the workspace"
    d, s, g = dist.cpu().numpy(), shift.cpu().numpy(), cframe.cpu().numpy()
    return [(d[w_off[n]:w_off[n + 1]], s[w_off[n]:w_off[n + 1]], g[w_off[n]:w_off[n + 1]]) for n in range(len(queries))]


def equal(got, ref, what=""):
    assert len(got) == len(ref)
    for n, (a, b) in enumerate(zip(got, ref)):
        for name, x, y in zip(('dist', 'shift', 'cframe'), a, b):
            assert x.shape == y.shape and np.array_equal(x, y), (what, n, name, x[:12], y[:12])


# ---------------------------------------------------------------------------------------------------------- edge grid
def edge_case(D, W):
    """the pieces of one (D, W): lengths 0, W-1, W, W+1, 63, 64, 65, 200 on both sides at note density 0.05; an all-ones and
    an all-rests piece, notes forced onto key 0 and key D-1, two identical corpus pieces; among the queries a verbatim and
    a transposed excerpt, an embedded excerpt and the trap that straddles two corpus pieces"""
    rng = np.random.default_rng(100 * D + W)
    lengths = [0, W - 1, W, W + 1, 63, 64, 65, 200]
    c = [(rng.random((P, D)) < 0.05).astype(np.uint8) for P in lengths]
    q = [(rng.random((P, D)) < 0.05).astype(np.uint8) for P in lengths]
    c[4][:] = 1
    c[5][:] = 0
    c[6][:, 0] = 1
    c[7][:50, D - 1] = 1
    if D > 4:
        c[7][100:101 + W, D - 2:] = 0                    # so that the excerpt below loses no note when it moves up
    c.append(c[7].copy())                                # two identical pieces: the lower index wins
    q[2][:] = c[7][10:10 + W]                            # verbatim
    q[3][:] = NR.shifted(c[7][100:101 + W], 2 if D > 4 else 0)     # the corpus passage is this excerpt two semitones DOWN
    q[4][:] = 1
    q[5][:] = 0
    q[6][:, 0] = 1
    q[7][120:, D - 1] = 1
    q[7][20:60] = c[6][5:45]                             # a copied stretch inside a longer piece
    h = W // 2
    q.append(np.concatenate([c[6][65 - h:], c[7][:W - h]], 0))     # contiguous in the corpus's frames, across two pieces
    return q, c


GRID = [(1, 1, 0, 1), (1, 33, 12, 3), (1, 16, 1, 1), (33, 2, 1, 1), (33, 16, 12, 3), (33, 33, 0, 1), (88, 1, 12, 1),
        (88, 16, 1, 1), (88, 33, 0, 3), (88, 2, 12, 3), (116, 33, 12, 1), (116, 1, 0, 3), (116, 2, 12, 1), (116, 16, 1, 3)]


@pytest.mark.parametrize("D,W,S,hop", GRID)
def test_edge_grid(dev, D, W, S, hop):
    q, c = edge_case(D, W)
    ref = NR.nearest(q, c, W, hop, S)
    got = run(dev, q, c, W, hop, S)
    equal(got, ref, (D, W, S, hop))
    assert [len(r[0]) for r in got] == [NR.n_windows(p.shape[0], W, hop) for p in q]
    assert len(got[0][0]) == 0 and len(got[1][0]) == 0 and len(got[2][0]) == 1
    if D >= 33:                                          # what the case planted is what was found
        assert got[2][0][0] == 0 and got[2][1][0] == 0
        song, frame = NR.song_frame(got[2][2], NR.offsets(c))
        assert (song[0], frame[0]) == (7, 10)
        if S >= 2:
            assert got[3][0][0] == 0 and got[3][1][0] == -2
        if W >= 2:
            assert got[8][0][0] > 0                      # the straddling trap is no copy
        assert (got[6][1] >= 0).all() and (got[7][1][(120 + hop - 1) // hop:] <= 0).all()


def test_a_corpus_without_a_window_and_an_excluded_only_piece(dev):
    rng = np.random.default_rng(5)
    W = 16
    q = [(rng.random((P, 88)) < 0.05).astype(np.uint8) for P in (40, 15, 16)]
    short = [(rng.random((P, 88)) < 0.05).astype(np.uint8) for P in (15, 0, 3)]
    for got in (run(dev, q, short, W, 1, 3), run(dev, q, [q[0]], W, 1, 3, exclude=[0, 0, 0])):
        assert [len(r[0]) for r in got] == [25, 0, 1]
        for d, s, g in got:
            assert (d == -1).all() and (s == 0).all() and (g == -1).all()
    equal(run(dev, q, short, W, 1, 3), NR.nearest(q, short, W, 1, 3))


# -------------------------------------------------------------------------------------------------------------- tiling
_TILING = {}


def tiling_case():
    """a corpus of 6592 frames in 32 uneven pieces = 26 corpus tiles of RN_NT starts; 40 query pieces of uneven length, the
    longest more than two query tiles of RN_TQ starts, and 260 short ones: at 300 query pieces the entry launches
    ceil(4096 / 300) = 14 workgroups per piece, so each walks two corpus tiles; a piece alone gets one workgroup per tile
    (sized from RN_NT, RN_TQ and the entry's grid rule; the assert below holds the case to them)"""
    if not _TILING:
        rng = np.random.default_rng(77)
        D, W, S = 88, 16, 2
        clen = [int(v) for v in rng.integers(60, 320, 32)]
        assert sum(clen) >= 5000
        c = [(rng.random((P, D)) < 0.05).astype(np.uint8) for P in clen]
        for p in c:                                      # keep the outer keys free: every shift is allowed somewhere
            p[:, :3] = 0
            p[:, D - 3:] = 0
        qlen = [int(v) for v in rng.integers(10, 150, 40)]
        q = [(rng.random((P, D)) < 0.05).astype(np.uint8) for P in qlen]
        for n in range(0, 40, 3):                        # excerpts, some transposed, from all over the corpus
            m = int(rng.integers(0, len(c)))
            P = min(qlen[n], clen[m])
            b = int(rng.integers(0, clen[m] - P + 1))
            q[n][:P] = NR.shifted(c[m][b:b + P], int(rng.integers(-2, 3)))
        q += [(rng.random((int(P), D)) < 0.05).astype(np.uint8) for P in rng.integers(W, W + 4, 260)]
        assert -(-WG_TARGET // len(q)) < -(-(sum(clen) - W + RN_TQ) // RN_NT) and max(qlen) - W + 1 > 2 * RN_TQ
        _TILING.update(D=D, W=W, S=S, q=q, c=c, ref=NR.nearest(q, c, W, 1, S))
    return _TILING


def test_tiling_against_the_reference(dev):
    T = tiling_case()
    got = run(dev, T['q'], T['c'], T['W'], 1, T['S'])
    equal(got, T['ref'])
    assert sum(int((r[0] == 0).sum()) for r in got[:40]) > 40          # the excerpts are found
    T['got'] = got


def test_rows_do_not_depend_on_the_batch(dev):
    T = tiling_case()
    got = T.get('got') or run(dev, T['q'], T['c'], T['W'], 1, T['S'])
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(T['q']))
    permuted = run(dev, [T['q'][i] for i in perm], T['c'], T['W'], 1, T['S'])
    for k, i in enumerate(perm):
        equal([permuted[k]], [got[i]], ('permuted', i))
    for i in (0, 3, 17, 39, 41):                         # alone in a batch of one: one workgroup per corpus tile
        equal(run(dev, [T['q'][i]], T['c'], T['W'], 1, T['S']), [got[i]], ('alone', i))


def test_the_corpus_permuted_gives_the_same_passages(dev):
    T = tiling_case()
    got = T.get('got') or run(dev, T['q'], T['c'], T['W'], 1, T['S'])
    c, W, S = T['c'], T['W'], T['S']
    perm = np.random.default_rng(4).permutation(len(c))
    c2 = [c[i] for i in perm]
    got2 = run(dev, T['q'], c2, W, 1, S)
    off, off2 = NR.offsets(c), NR.offsets(c2)
    checked = zeros = 0
    for n, ((d, s, g), (d2, s2, g2)) in enumerate(zip(got, got2)):
        assert np.array_equal(d, d2), n
        song, frame = NR.song_frame(g, off)
        song2, frame2 = NR.song_frame(g2, off2)
        for j in range(len(d)):
            # the passage (song, frame, shift) is the same wherever the minimum is unique: both runs name A minimum, so
            # if they differ the minimum is not unique, and then the first run's passage is as good in the second corpus
            same = s[j] == s2[j] and perm[song2[j]] == song[j] and frame2[j] == frame[j]
            zeros += int(d[j] == 0)
            if not same:
                assert d[j] > 0, (n, j)                  # a copy has one source
                q = T['q'][n][j:j + W]
                for (sh, sg, fr, cc) in ((s[j], song[j], frame[j], c), (s2[j], song2[j], frame2[j], c2)):
                    assert int((NR.shifted(q, sh) != cc[sg][fr:fr + W]).sum()) == d[j]
            else:
                checked += 1
    assert checked >= zeros > 40
    # shift alone: equal distance at another shift would be a tie between shifts; the rank decides it the same way in both
    ref2 = NR.nearest(T['q'][:40], c2, W, 1, S)
    equal(got2[:40], ref2, 'permuted corpus')


# ------------------------------------------------------------------------------------------------------------- exclude
def test_exclude_is_leave_one_out(dev):
    rng = np.random.default_rng(9)
    D, W, S = 88, 16, 1
    c = [(rng.random((int(P), D)) < 0.05).astype(np.uint8) for P in rng.integers(W, 120, 12)]
    c[5] = c[2].copy()                                   # the planted duplicates
    plain = run(dev, c, c, W, 1, S)
    off = NR.offsets(c)
    for n, (d, s, g) in enumerate(plain):
        assert (d == 0).all() and (s == 0).all()
        song, frame = NR.song_frame(g, off)
        assert (song == (2 if n == 5 else n)).all() and (frame == np.arange(len(d))).all()
    ex = list(range(len(c)))
    loo = run(dev, c, c, W, 1, S, exclude=ex)
    equal(loo, NR.nearest(c, c, W, 1, S, exclude=ex))
    for n, (d, s, g) in enumerate(loo):
        assert (NR.song_frame(g, off)[0] != n).all()
        assert (d == 0).all() if n in (2, 5) else (d > 0).all()
    mixed = [-1 if n % 2 else n for n in ex]
    equal(run(dev, c, c, W, 1, S, exclude=mixed), NR.nearest(c, c, W, 1, S, exclude=mixed))


# ---------------------------------------------------------------------------------------------------------- end to end
def test_nearest_end_to_end(dev):
    from clvae_amd import novelty
    q, c = edge_case(88, 16)
    for hop, S, ex in ((1, 2, None), (3, 0, [7, -1, 7, 8, 4, 5, 6, 7, None])):
        nov = novelty.nearest(q, c, window=16, hop=hop, semitones=S, exclude=ex)
        ref = NR.nearest(q, c, 16, hop, S, None if ex is None else [-1 if e is None else e for e in ex])
        off = NR.offsets(c)
        assert len(nov) == len(q) and nov.lengths == [p.shape[0] for p in q] and (nov.window, nov.hop, nov.semitones) == (16, hop, S)
        for n, (d, s, g) in enumerate(ref):
            song, frame = NR.song_frame(g, off)
            assert np.array_equal(nov.dist[n], d) and np.array_equal(nov.shift[n], s), n
            assert np.array_equal(nov.song[n], song) and np.array_equal(nov.frame[n], frame), n
            assert np.array_equal(nov.starts[n], np.arange(len(d)) * hop)
            assert np.array_equal(nov.notes[n], NR.notes_per_window(q[n], 16, hop)), n
        assert nov.copied()[2] == 1.0 and nov.song[2][0] == (7 if ex is None else 8)       # the verbatim excerpt; its source excluded: the twin
        assert nov.longest_copy(7) >= (40 if hop == 1 else 16)             # the stretch copied into the long piece
    stacked = novelty.nearest(np.stack([q[7], q[7]]), np.stack([c[7], c[8]]), window=16)
    assert np.array_equal(stacked.dist[0], stacked.dist[1]) and len(stacked) == 2


def _save_model(dev, tmp_path, family, C):
    if family == 'cl_vae':
        from clvae_amd.cl_vae.model import get_model
        model, _ = get_model(4, 88, (88, 2), (24, C), 'adam-wn', seed=1, device=dev)
        margs = dict(batch_size=4, original_dim=88, intermediate_dim=88, latent_dim=2, intermediate_class_dim=24, n_classes=C,
                     class_weight=1.0, use_x_prev=False, optimizer='adam-wn')
    else:
        from clvae_amd.cl_vrnn.model import get_model
        model, _ = get_model(4, 88, 88, 2, 8, C, True, 'adam-wn', seed=1, device=dev)
        margs = dict(batch_size=4, original_dim=88, intermediate_dim=88, latent_dim=2, seq_length=8, n_classes=C, class_weight=1.0,
                     use_x_prev=True, optimizer='adam-wn')
    model.save_weights(str(tmp_path / "m.h5"))
    json.dump(margs, open(str(tmp_path / "m.json"), 'w'))
    return str(tmp_path / "m.h5")


@pytest.mark.parametrize("family", ['cl_vae', 'cl_vrnn'])
def test_sample_tool_with_the_audit(dev, tmp_path, family):
    from clvae_amd.keytrack import split_songs
    data = write_jsb_pickle('all', str(tmp_path / "jsb.pickle"))
    n_test, C = len(split_songs(data, 'test')[0]), len(split_songs(data, 'test')[2])
    h5 = _save_model(dev, tmp_path, family, C)
    sdir = str(tmp_path / "samples")
    os.makedirs(sdir)
    script = os.path.join(ROOT, 'classifying-vae-lstm_amd', family, 'sample.py')
    r = subprocess.run([sys.executable, script, 'a', '-n', '3', '-t', '8', '--device_loop', '-i', h5, '--train_file', data,
                        '--sample_dir', sdir, '--novelty', '4', '--novelty_transpose', '2'],
                       capture_output=True, text=True, timeout=240, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert sum(l.startswith("sample ") for l in lines) == 3
    assert any(l.startswith("novelty: windows of 4 frames, transposed by up to 2 semitones") for l in lines)
    assert any(l.startswith("baseline, %d test songs" % n_test) for l in lines)
    assert len([f for f in os.listdir(sdir) if f.endswith('.mid')]) >= 3


def test_module_tool_train_against_train(dev, tmp_path):
    from clvae_amd.keytrack import split_songs
    data = write_jsb_pickle('all', str(tmp_path / "jsb.pickle"))
    rolls = split_songs(data, 'train')[0]
    out = str(tmp_path / "f.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'clvae_amd.novelty', '--train_file', data, '--split', 'train', '--against', 'train',
                        '--transpose', '1', '--out', out], capture_output=True, text=True, timeout=240, stdin=subprocess.DEVNULL,
                       cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.load(open(out))
    assert res['n_songs'] == len(rolls) == len(res['songs']) and res['leave_one_out'] and res['window'] == 16
    for n, s in enumerate(res['songs']):
        assert s['frames'] == rolls[n].shape[0] and s['nearest_song'] != n               # no self-match
    assert len(res['closest']) == min(10, sum(s['min_dist'] >= 0 for s in res['songs']))
    assert all(c['song'] != c['query'] for c in res['closest'])
    assert "dist quantiles" in r.stdout and "leaves itself out" in r.stdout
