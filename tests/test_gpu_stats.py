"""GPU tests of the roll statistics audit against tests/stats_reference.py: clv_roll_stats' table in exact
integer equality over an edge grid of (D, Lmax), at piece boundaries, over tiles and workgroups (one long piece, a thousand
short ones, both at once), alone and in any batch, into a used buffer, and stats.profile and the tools end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stats_reference as SR
from helpers import ROOT, write_jsb_pickle

pytestmark = pytest.mark.gpu

RS_NT = 256             # frames of a tile of csrc/stats.hip
TAIL = 64


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    return torch.device("cuda:0")


def test_the_tile_constant_is_the_kernels():
    src = open(os.path.join(ROOT, "classifying-vae-lstm_amd", "csrc", "stats.hip")).read()
    assert "RS_NT = %d;" % RS_NT in src


def run(dev, pieces, Lmax, tonics=None, low=21, table=None):
    """clv_roll_stats through ops.roll_stats -> int64 [N, S]; -7 behind the table (and in it, before the call)"""
    from clvae_amd import ops
    D, N = pieces[0].shape[1], len(pieces)
    off = SR.offsets(pieces)
    F, S = int(off[-1]), SR.columns(D, Lmax)
    assert ops.roll_stats_columns(D, Lmax) == S
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    roll = t(np.concatenate(pieces, 0).astype(np.uint8)) if F else None
    if table is None:
        table = torch.full((N * S + TAIL,), -7, dtype=torch.int64, device=dev)
    ops.roll_stats(N, D, Lmax, low, F, roll, t(off), None if tonics is None else t(np.asarray(tonics, np.int32)), table)
    torch.cuda.synchronize()
    assert (table[N * S:] == -7).all(), "write behind the table"
    return table[:N * S].cpu().numpy().reshape(N, S)


def equal(got, ref, D, Lmax, what=""):
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.int64
    if not np.array_equal(got, ref):
        for name, (at, n) in SR.sections(D, Lmax).items():
            for k in range(got.shape[0]):
                assert np.array_equal(got[k, at:at + n], ref[k, at:at + n]), (what, 'piece', k, name, got[k, at:at + n], ref[k, at:at + n])
        raise AssertionError(what)


# ---------------------------------------------------------------------------------------------------------- edge grid
def edge_case(D, Lmax):
    """five pieces of 0, 1, 2, 37 and 300 frames at note density 0.05; in the longest one note held for 70 frames (longer
    than every Lmax) and one frame with every note on (clips `voices`, `change`, and holds the largest interval)"""
    rng = np.random.default_rng(1000 * D + Lmax)
    pieces = [(rng.random((P, D)) < 0.05).astype(np.uint8) for P in (0, 1, 2, 37, 300)]
    pieces[4][100:170, D // 2] = 1
    pieces[4][99, D // 2] = pieces[4][170, D // 2] = 0
    pieces[4][200] = 1
    pieces[3][5] = 0                                      # an empty frame inside a piece
    pieces[1][0, D - 1] = 3                               # any non-zero byte sounds; the last note of the last word
    return pieces


@pytest.mark.parametrize("D", [1, 32, 33, 64, 65, 88, 116])
@pytest.mark.parametrize("Lmax", [1, 8, 64])
def test_edge_grid(dev, D, Lmax):
    pieces = edge_case(D, Lmax)
    tonics = [7, -1, 11, 0, 4]
    for ton in (None, tonics):
        ref = SR.table(pieces, D, Lmax, 21, ton)
        got = run(dev, pieces, Lmax, ton)
        equal(got, ref, D, Lmax, (D, Lmax, ton))
    sec = SR.sections(D, Lmax)
    assert not got[0].any()                               # the piece of 0 frames
    at, n = sec['voices']
    assert got[4, at + min(D, SR.V)] >= 1                 # the full frame
    at, n = sec['duration']
    assert got[4, at + n - 1] >= 1                        # the held note reaches the last bin, whatever Lmax
    if D > 1:
        at, n = sec['interval']
        assert got[4, at + D - 1] >= 1 and got[4, at] == 0
    at, n = sec['change']
    assert got[:, at:at + n].sum(1).tolist() == [0, 0, 1, 36, 299]
    # low moves the degrees, nothing else
    moved = run(dev, pieces, Lmax, tonics, low=0)
    equal(moved, SR.table(pieces, D, Lmax, 0, tonics), D, Lmax, 'low 0')


# ---------------------------------------------------------------------------------------------------- piece boundaries
def test_nothing_crosses_a_piece_boundary(dev):
    """the same note sounds in the last frame of every piece and the first of the next, the highest note jumps there: one
    string of frames cut into pieces at many places, among them the multiples of the tile"""
    D, Lmax = 88, 16
    rng = np.random.default_rng(11)
    whole = (rng.random((700, D)) < 0.04).astype(np.uint8)
    whole[:, 30] = 1                                      # held across every cut
    whole[:, 50:] = 0                                     # the top voice moves inside 30..49: no step reaches 24
    cuts = [0, 1, 2, 9, 10, 255, 256, 257, 300, 511, 512, 513, 600, 700]
    for c in cuts[1:-1]:
        whole[c - 1, 40] = 1                              # the top voice: 40 before the cut, 80 after it
        whole[c - 1, 41:] = 0
        whole[c, 80] = 1
    pieces = [whole[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    ref = SR.table(pieces, D, Lmax)
    got = run(dev, pieces, Lmax)
    equal(got, ref, D, Lmax)
    sec = SR.sections(D, Lmax)
    at, n = sec['change']
    assert got[:, at:at + n].sum() == 700 - len(pieces)   # P - 1 entries per piece
    at, n = sec['top_step']
    assert got[:, at + n - 1].sum() == 0                  # no step of +40 (clamped to +24): it would cross a cut
    at, n = sec['duration']
    pitch30 = got[:, 30]
    assert np.array_equal(pitch30, np.diff(cuts))
    assert got[:, at:at + n].sum() > len(pieces)
    # against the uncut string: the cuts make more and shorter notes, the same cells
    one = run(dev, [whole], Lmax)
    assert np.array_equal(one[0, :D], got[:, :D].sum(0)) and one[0, at:at + n].sum() < got[:, at:at + n].sum()
    equal(one, SR.table([whole], D, Lmax), D, Lmax, 'uncut')


# -------------------------------------------------------------------------------------------------------------- tiling
_TILING = {}


def tiling_case():
    """one piece of 3000 frames (12 tiles) with a note held across every multiple of 64 frames and runs that end on either
    side of every tile boundary; 1024 pieces of 8 frames (32 to a tile); the reference's rows of both, computed once"""
    if not _TILING:
        rng = np.random.default_rng(21)
        D, Lmax = 88, 32
        long = (rng.random((3000, D)) < 0.05).astype(np.uint8)
        long[:, 44] = 1
        long[1500, 44] = 0                                # two runs of 1500 and 1499 frames
        for b in range(RS_NT, 3000, RS_NT):               # runs that start before a tile boundary and end behind it
            long[b - 40:b + 1, 10] = 1
            long[b - 41, 10] = long[b + 1, 10] = 0
            long[b - 3:b + 29, 12] = 1
            long[b - 4, 12] = long[b + 29, 12] = 0
        short = [(rng.random((8, D)) < 0.06).astype(np.uint8) for _ in range(1024)]
        for n in range(0, 1024, 5):
            short[n][:, 50] = 1                           # held through the whole piece, and into the next one's frames
        tonics = [int(v) for v in rng.integers(-1, 12, 1025)]
        _TILING.update(D=D, Lmax=Lmax, long=long, short=short, tonics=tonics,
                       ref_long=SR.table([long], D, Lmax, 21, tonics[:1]), ref_short=SR.table(short, D, Lmax, 21, tonics[1:]))
    return _TILING


def test_one_long_piece(dev):
    T = tiling_case()
    equal(run(dev, [T['long']], T['Lmax'], T['tonics'][:1]), T['ref_long'], T['D'], T['Lmax'])
    at, n = SR.sections(T['D'], T['Lmax'])['duration']
    assert T['ref_long'][0, at + n - 1] >= 2 + 11 * 2     # the two long runs, and a run of 41 and one of 32 per boundary


def test_a_thousand_short_pieces(dev):
    T = tiling_case()
    equal(run(dev, T['short'], T['Lmax'], T['tonics'][1:]), T['ref_short'], T['D'], T['Lmax'])


def test_long_and_short_in_one_call(dev):
    T = tiling_case()
    got = run(dev, T['short'][:500] + [T['long']] + T['short'][500:], T['Lmax'],
              T['tonics'][1:501] + T['tonics'][:1] + T['tonics'][501:])
    ref = np.concatenate([T['ref_short'][:500], T['ref_long'], T['ref_short'][500:]])
    equal(got, ref, T['D'], T['Lmax'])


# -------------------------------------------------------------------------------------------------- batch independence
def test_rows_do_not_depend_on_the_batch(dev):
    D, Lmax = 88, 24
    rng = np.random.default_rng(31)
    lengths = [0, 1, 7, 64, 255, 256, 257, 300, 0, 40, 513, 3, 90, 129, 31, 1000]
    pieces = [(rng.random((P, D)) < 0.06).astype(np.uint8) for P in lengths]
    tonics = [int(v) for v in rng.integers(-1, 12, len(pieces))]
    got = run(dev, pieces, Lmax, tonics)
    equal(got, SR.table(pieces, D, Lmax, 21, tonics), D, Lmax)
    perm = rng.permutation(len(pieces))
    permuted = run(dev, [pieces[i] for i in perm], Lmax, [tonics[i] for i in perm])
    assert np.array_equal(permuted, got[perm])
    for i in (0, 2, 5, 10, 15):                           # alone, and in a batch of two
        assert np.array_equal(run(dev, [pieces[i]], Lmax, [tonics[i]])[0], got[i]), i
        assert np.array_equal(run(dev, [pieces[15], pieces[i]], Lmax, [tonics[15], tonics[i]])[1], got[i]), i
    half = run(dev, pieces[8:], Lmax, tonics[8:])
    assert np.array_equal(half, got[8:])


def test_the_table_is_overwritten(dev):
    D, Lmax = 88, 16
    rng = np.random.default_rng(41)
    pieces = [(rng.random((P, D)) < 0.05).astype(np.uint8) for P in (50, 0, 300)]
    S = SR.columns(D, Lmax)
    table = torch.full((3 * S + TAIL,), -7, dtype=torch.int64, device=dev)
    first = run(dev, pieces, Lmax, table=table).copy()    # into -7s
    second = run(dev, pieces, Lmax, table=table)          # into its own result
    assert np.array_equal(first, second)
    equal(second, SR.table(pieces, D, Lmax), D, Lmax)
    other = [(rng.random((P, D)) < 0.05).astype(np.uint8) for P in (10, 20, 0)]
    equal(run(dev, other, Lmax, table=table), SR.table(other, D, Lmax), D, Lmax, 'another batch into the same buffer')


# ---------------------------------------------------------------------------------------------------------- end to end
def test_profile_end_to_end(dev, tmp_path):
    from clvae_amd import stats
    from clvae_amd.keytrack import split_songs
    data = write_jsb_pickle('Cs', str(tmp_path / "jsb.pickle"))
    rolls, keys, key_map = split_songs(data, 'train')
    tonics = [stats.tonic_of(key_map, k) for k in keys]
    st = stats.profile(rolls, tonics, max_duration=32)
    ref = SR.table(rolls, 88, 32, 21, tonics)
    assert st.table.dtype == np.int64 and np.array_equal(st.table, ref)
    assert st.lengths == [r.shape[0] for r in rolls] and (st.width, st.max_duration, st.low) == (88, 32, 21)
    for name, (at, n) in SR.sections(88, 32).items():
        assert np.array_equal(st.section(name), ref[:, at:at + n]) and np.array_equal(st.pooled(name), ref[:, at:at + n].sum(0))
    m = st.means()
    assert m['frames'] == sum(st.lengths) and 3.0 < m['notes_per_frame'] < 4.5 and m['in_scale'] > 0.9   # chorales, in their keys
    assert stats.profile(rolls, None).means()['in_scale'] < m['in_scale']     # the tonics matter: the songs are not all in C
    same = stats.compare(st, st)
    assert all(v == 0.0 for v in same['divergence'].values()) and all(abs(v - 1) < 1e-12 for v in same['overlap'].values())
    # a device tensor gives the table of the same rolls passed as numpy, without a trip through the host
    rng = np.random.default_rng(51)
    block = (rng.random((6, 70, 88)) < 0.05).astype(np.uint8)
    ton = [0, 5, -1, 11, 2, 7]
    a = stats.profile(block, ton, max_duration=16)
    b = stats.profile(torch.as_tensor(block, device=dev), ton, max_duration=16)
    assert np.array_equal(a.table, b.table) and np.array_equal(a.table, SR.table(list(block), 88, 16, 21, ton))
    assert b.lengths == [70] * 6
    loud = stats.profile(torch.as_tensor(block * 200, device=dev), ton, max_duration=16)        # any non-zero byte
    assert np.array_equal(loud.table, a.table)
    # only notes of the C major scale, under tonic 0: in_scale is 1
    cmaj = np.zeros((3, 40, 88), np.uint8)
    scale = [d for d in range(88) if (d + 21) % 12 in SR.IN_SCALE]
    cmaj[:, :, scale] = (rng.random((3, 40, len(scale))) < 0.1).astype(np.uint8)
    assert cmaj.sum() > 100
    assert stats.profile(cmaj, [0, 0, 0]).means()['in_scale'] == 1.0
    assert stats.profile(cmaj, [1, 1, 1]).means()['in_scale'] < 0.5           # C major's notes under D flat


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
    n_train, n_test, C = len(split_songs(data, 'train')[0]), len(split_songs(data, 'test')[0]), len(split_songs(data, 'test')[2])
    h5 = _save_model(dev, tmp_path, family, C)
    sdir = str(tmp_path / "samples")
    os.makedirs(sdir)
    script = os.path.join(ROOT, 'classifying-vae-lstm_amd', family, 'sample.py')
    r = subprocess.run([sys.executable, script, 'a', '-n', '3', '-t', '8', '--device_loop', '-i', h5, '--train_file', data,
                        '--sample_dir', sdir, '--stats', '--stats_max_duration', '8'],
                       capture_output=True, text=True, timeout=240, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert any(l.startswith("stats: 3 samples, note lengths up to 8 frames, degrees from the labels' tonics") for l in lines)
    assert any(l.startswith("samples' means: ") and "notes per frame" in l and "in scale" in l for l in lines)
    assert any(l.startswith("samples against %d training songs, divergence in bits: pitch " % n_train) for l in lines)
    assert sum(l.startswith("sample ") and "largest divergence" in l for l in lines) == 3
    assert any(l.startswith("baseline, %d test songs against the training songs: pitch " % n_test) for l in lines)
    assert any(l.startswith("baseline's means: ") for l in lines)
    assert len([f for f in os.listdir(sdir) if f.endswith('.mid')]) >= 3


def test_module_tool_test_against_train(dev, tmp_path):
    from clvae_amd import stats
    from clvae_amd.keytrack import split_songs
    data = write_jsb_pickle('all', str(tmp_path / "jsb.pickle"))
    out = str(tmp_path / "res.json")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'clvae_amd.stats', '--train_file', data, '--split', 'test', '--against', 'train',
                        '--out', out], capture_output=True, text=True, timeout=240, stdin=subprocess.DEVNULL, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.load(open(out))
    sec = SR.sections(88, 32)
    for split, pooled in (('test', res['profile']['pooled']), ('train', res['against_pooled'])):
        rolls, keys, key_map = split_songs(data, split)
        ref = SR.table(rolls, 88, 32, 21, [stats.tonic_of(key_map, k) for k in keys]).sum(0)
        for name, (at, n) in sec.items():
            assert pooled[name] == ref[at:at + n].tolist(), (split, name)
    assert res['n_songs'] == len(split_songs(data, 'test')[0]) == len(res['profile']['table']) == len(res['divergence_to'])
    assert res['query'] == 'test' and res['against'] == 'train' and res['max_duration'] == 32
    assert set(res['compare']['divergence']) == set(SR.NAMES) and all(0 <= v <= 1 for v in res['compare']['divergence'].values())
    assert res['compare']['means_a']['in_scale'] > 0.9
    assert "divergence in bits, test against train" in r.stdout and "overlap: pitch" in r.stdout
