"""CPU tests of the roll statistics audit: the C ABI surface of clv_roll_stats, the library's and profile()'s
refusals, RollStats / compare on hand-built tables, tonic_of, and the argument surfaces of the tools."""
import ctypes
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import clvae_amd  # noqa: F401
import stats_reference as SR
from clvae_amd import _lib
from helpers import ROOT

COLUMNS, STATS = 'clv_roll_stats_column_count', 'clv_roll_stats'


def _header():
    return open(os.path.join(ROOT, "include", "clvae.h")).read()


def _protos():
    hdr = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    return dict(re.findall(r"\b(clv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))


def test_the_entries_are_declared_bound_and_exported():
    protos = _protos()
    for name, nargs in ((COLUMNS, 2), (STATS, 10)):
        assert name in protos, name
        assert len(protos[name].split(',')) == nargs
        r, args = _lib.SIGNATURES[name]
        assert r is ctypes.c_int and len(args) == nargs
        assert hasattr(_lib.lib(), name)
    a = _lib.SIGNATURES[STATS][1]
    assert all(t is ctypes.c_int for t in a[:4]) and a[4] is ctypes.c_int64 and all(t is ctypes.c_void_p for t in a[5:])
    hdr = _header()
    assert int(re.search(r"#define\s+CLV_ABI_VERSION\s+(\d+)", hdr).group(1)) == 610
    assert _lib.ABI_VERSION == 610 and _lib.lib().clv_version() == 610
    for name, value in (('CLV_STATS_VOICES', SR.V), ('CLV_STATS_CHANGE', SR.C), ('CLV_STATS_STEP', SR.M)):
        assert int(re.search(r"#define\s+%s\s+(\d+)" % name, hdr).group(1)) == value
    from clvae_amd import ops
    assert callable(ops.roll_stats) and callable(ops.roll_stats_columns)
    src = open(os.path.join(ROOT, "classifying-vae-lstm_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bstats\.hip\b", src, flags=re.M)


def test_column_count():
    f = _lib.lib().clv_roll_stats_column_count
    for D in (1, 2, 31, 32, 33, 64, 65, 88, 115, 116):
        for Lmax in (1, 2, 8, 32, 63, 64):
            assert f(D, Lmax) == SR.columns(D, Lmax), (D, Lmax)
    for D, Lmax in ((0, 32), (-1, 32), (117, 32), (88, 0), (88, -1), (88, 65), (0, 0), (1 << 30, 1 << 30)):
        assert f(D, Lmax) == 0, (D, Lmax)
    from clvae_amd import ops, stats
    assert ops.roll_stats_columns(88, 32) == 440 == sum(stats.section_bins(88, 32).values())
    assert stats.section_bins(88, 32) == SR.bins(88, 32) and tuple(stats.section_bins(5, 3)) == SR.NAMES == stats.SECTIONS
    assert (stats.VOICES, stats.CHANGE, stats.STEP, stats.IN_SCALE) == (SR.V, SR.C, SR.M, SR.IN_SCALE)


ORDER = ('N', 'D', 'Lmax', 'low', 'F', 'roll', 'off', 'tonic', 'table', 'stream')


def _args(**kw):
    """a well-formed argument list (pointers: any non-NULL value; the entry refuses before it reads them)"""
    p = ctypes.c_void_p(4096)
    a = dict(N=3, D=88, Lmax=32, low=21, F=64, roll=p, off=p, tonic=p, table=p, stream=None)
    a.update(kw)
    return [a[k] for k in ORDER]


@pytest.mark.parametrize("bad", [dict(N=0), dict(N=-1), dict(N=(1 << 20) + 1), dict(D=0), dict(D=-1), dict(D=117),
                                 dict(Lmax=0), dict(Lmax=-1), dict(Lmax=65), dict(low=-1), dict(low=128), dict(F=-1),
                                 dict(roll=None), dict(off=None), dict(table=None), dict(roll=None, off=None, table=None),
                                 dict(F=0, off=None), dict(F=0, table=None), dict(F=0, roll=None, tonic=None, N=0)])
def test_the_entry_refuses_before_the_device(bad):
    """CLV_EINVAL (-1) on a machine without a GPU: nothing was touched or launched"""
    assert _lib.lib().clv_roll_stats(*_args(**bad)) == -1


# ------------------------------------------------------------------------------------------------------------- profile()
def test_profile_refuses_with_value_errors_before_the_device():
    import torch
    from clvae_amd.stats import profile
    ok = np.zeros((20, 88))
    bad_calls = [
        dict(pieces=[np.full((20, 88), 2.0)]), dict(pieces=[np.full((20, 88), 0.5)]),        # not binary
        dict(pieces=[ok, np.zeros((20, 87))]),                                               # the widths differ
        dict(pieces=[np.zeros((20, 117))]), dict(pieces=np.zeros((2, 20, 120))),             # wider than 116
        dict(pieces=[np.zeros(88)]), dict(pieces=[]),
        dict(pieces=torch.zeros(2, 20, 88, dtype=torch.uint8)),                              # a tensor, but not on the device
        dict(pieces=torch.zeros(2, 20, 88)),
        dict(pieces=[ok], max_duration=0), dict(pieces=[ok], max_duration=65), dict(pieces=[ok], max_duration=8.0),
        dict(pieces=[ok], max_duration=True),
        dict(pieces=[ok], low=-1), dict(pieces=[ok], low=128), dict(pieces=[ok], low=21.0),
        dict(pieces=[ok], tonics=[0, 0]), dict(pieces=[ok, ok], tonics=[0]),                 # the wrong length
        dict(pieces=[ok], tonics=[12]), dict(pieces=[ok], tonics=[-2]), dict(pieces=[ok], tonics=[0.5]),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            profile(device='cuda:0', **kw)
    assert not torch.cuda.is_initialized()


# ------------------------------------------------------------------------------------------------- RollStats and compare
def _stats(rows, D=5, Lmax=3):
    """a RollStats from the reference's rows of small pieces: no device"""
    from clvae_amd.stats import RollStats
    return RollStats(SR.table(rows, D, Lmax, low=21, tonics=[9] * len(rows)), [p.shape[0] for p in rows], D, Lmax, 21,
                     [9] * len(rows))


def _roll(D, *frames):
    r = np.zeros((len(frames), D), np.uint8)
    for t, f in enumerate(frames):
        r[t, list(f)] = 1
    return r


def test_rollstats_sections_means_and_json():
    from clvae_amd.stats import RollStats
    a, b = _roll(5, (0, 2), (0, 2, 4), (), (1, 4)), _roll(5, (3,), (3,))
    st = _stats([a, b])
    assert len(st) == 2 and st.lengths == [4, 2] and st.table.dtype == np.int64 and st.table.shape == (2, 162)
    assert np.array_equal(st.section('pitch'), [[2, 1, 2, 0, 2], [0, 0, 0, 2, 0]])
    assert st.section('duration').base is st.table                                        # a view
    assert np.array_equal(st.pooled('duration'), [3, 3, 0]) and np.array_equal(st.pooled(), st.table.sum(0))
    np.testing.assert_allclose(st.distribution('duration'), [.5, .5, 0])
    assert st.distribution('interval').dtype == np.float64
    assert not _stats([b]).distribution('interval').any()                                 # an empty section: all zeros
    m = st.means()
    assert m['frames'] == 6
    np.testing.assert_allclose([m['notes_per_frame'], m['empty_frames'], m['note_length'], m['note_length_clipped']],
                               [9 / 6, 1 / 6, 9 / 6, 0.0])
    np.testing.assert_allclose(m['change'], (1 + 3 + 2 + 0) / 4)
    np.testing.assert_allclose(m['span'], (2 + 4 + 3 + 0 + 0) / 5)
    # degrees (note d is degree d here): 0, 2, 4 in the scale, 1 and 3 not
    np.testing.assert_allclose(m['in_scale'], 6 / 9)
    long = _stats([np.ones((7, 5), np.uint8)]).means()
    assert long['note_length'] == 3.0 and long['note_length_clipped'] == 1.0              # 7 frames, counted as 3
    j = json.loads(json.dumps(st.to_json()))
    assert j['table'] == st.table.tolist() and j['lengths'] == [4, 2] and j['sections']['degree'] == [5, 12]
    assert j['pooled']['pitch'] == [2, 1, 2, 2, 2] and j['means']['frames'] == 6 and j['tonics'] == [9, 9]
    with pytest.raises(ValueError):
        st.section('tempo')
    with pytest.raises(ValueError):
        RollStats(np.zeros((2, 161), np.int64), [4, 2], 5, 3)
    empty = RollStats(np.zeros((1, 162), np.int64), [0], 5, 3).means()
    assert all(v == 0 for v in empty.values())


def _js(p, q):
    """the written formula: 0.5 sum p log2(p / m) + 0.5 sum q log2(q / m), m = (p + q) / 2, 0 log 0 = 0"""
    m = [(x + y) / 2 for x, y in zip(p, q)]
    kl = lambda a: sum(x * np.log2(x / y) for x, y in zip(a, m) if x > 0)
    return 0.5 * kl(p) + 0.5 * kl(q)


def test_compare():
    from clvae_amd.stats import SECTIONS, compare, js_divergence
    a = _stats([_roll(5, (0, 2), (0, 2, 4), (), (1, 4)), _roll(5, (3,), (3,))])
    b = _stats([_roll(5, (0, 1), (1, 2), (1, 2, 3), (0, 4), (4,))])
    same = compare(a, a)
    assert set(same) == {'divergence', 'overlap', 'means_a', 'means_b'} and same['means_a'] == a.means()
    for name in SECTIONS:
        assert same['divergence'][name] == 0.0 and abs(same['overlap'][name] - 1.0) < 1e-15, name
    ab, ba = compare(a, b), compare(b, a)
    assert ab['means_a'] == ba['means_b'] == a.means()
    for name in SECTIONS:
        p, q = a.distribution(name), b.distribution(name)
        assert abs(ab['divergence'][name] - _js(p, q)) <= 1e-12, name
        assert abs(ab['overlap'][name] - sum(min(x, y) for x, y in zip(p, q))) <= 1e-12, name
        assert abs(ab['divergence'][name] - ba['divergence'][name]) <= 1e-15 and ab['overlap'][name] == ba['overlap'][name]
        assert 0.0 <= ab['divergence'][name] <= 1.0
    assert 0 < ab['divergence']['pitch'] < 1 and 0 < ab['overlap']['pitch'] < 1
    # disjoint: notes {0, 1} against {3, 4}, one note per frame, steps up against steps down
    lo, hi = _stats([_roll(5, (0,), (1,), (0,), (1,))]), _stats([_roll(5, (4, 3), (3, 4), (4, 3))])
    d = compare(lo, hi)
    for name in ('pitch', 'degree', 'voices', 'change'):
        assert abs(d['divergence'][name] - 1.0) < 1e-15 and d['overlap'][name] == 0.0, name
    # an empty section on either side (no frame with two notes: no interval): divergence 0, overlap 0
    assert d['divergence']['interval'] == 0.0 and d['overlap']['interval'] == 0.0
    assert float(js_divergence(np.zeros(4), np.zeros(4))) == 0.0
    # per piece against the pooled other side
    rows = a.divergence_to(b)
    assert rows.shape == (2, len(SECTIONS)) and rows.dtype == np.float64
    for n in range(2):
        for k, name in enumerate(SECTIONS):
            h = a.section(name)[n].astype(np.float64)
            want = _js(h / h.sum(), b.distribution(name)) if h.sum() and b.pooled(name).sum() else 0.0
            assert abs(rows[n, k] - want) <= 1e-12, (n, name)
    assert np.array_equal(a.divergence_to(a)[:, :1] > 0, [[True], [True]])                # each piece differs from the pool
    with pytest.raises(ValueError):
        compare(a, _stats([_roll(6, (0,))], D=6))
    with pytest.raises(ValueError):
        a.divergence_to(_stats([_roll(5, (0,))], Lmax=4))


def test_tonic_of():
    from clvae_amd.stats import tonic_of
    key_map = {'A': 0, 'B-': 1, 'C': 2, 'E-': 3, 'F#': 4, 'a': 5, 'f#': 6, 'c': 7}
    assert [tonic_of(key_map, c) for c in range(8)] == [9, 10, 0, 3, 6, 0, 9, 3]         # minor: its relative major
    assert tonic_of(key_map, None) == -1 and tonic_of(key_map, -1) == -1
    assert tonic_of(key_map, np.int64(2)) == 0
    with pytest.raises(ValueError):
        tonic_of(key_map, 8)


# ----------------------------------------------------------------------------------------------------------- the tools
FLAG_LISTS = ('DEVICE_LOOP_FLAGS', 'HARMONIZE_FLAGS', 'TEMPERATURE_FLAGS', 'VARY_FLAGS', 'MORPH_FLAGS', 'RESUME_FLAGS',
              'VOICES_FLAGS', 'GIBBS_FLAGS', 'STATS_FLAGS', 'NOVELTY_FLAGS', 'LIVE_FLAGS')


@pytest.mark.parametrize("tool", ['cl_vae.sample', 'cl_vrnn.sample'])
def test_parser_rules_of_the_two_flags(tool, capsys):
    from clvae_amd import cli
    p = cli.parser_for(tool, sum((getattr(cli, n) for n in FLAG_LISTS), []))
    ns = p.parse_args(['run'])
    assert ns.stats is False and ns.stats_max_duration == 32
    ns = p.parse_args(['run', '--stats'])
    assert ns.stats is True and ns.stats_max_duration == 32
    assert p.parse_args(['run', '--stats', '--stats_max_duration', '1']).stats_max_duration == 1
    assert p.parse_args(['run', '--stats', '--stats_max_duration', '64', '--vary']).stats_max_duration == 64
    assert p.parse_args(['run', '--stats', '--host_loop', '--novelty', '8']).stats is True       # a post-process: any route
    for bad in (['--stats_max_duration', '8'], ['--stats_max_duration', '32'], ['--stats', '--stats_max_duration', '0'],
                ['--stats', '--stats_max_duration', '65'], ['--stats', '--stats_max_duration', '-1'],
                ['--stats', '--stats_max_duration', 'x'], ['--stats', '3']):
        with pytest.raises(SystemExit):
            p.parse_args(['run'] + bad)
    capsys.readouterr()
    # a parser without the flags is not touched by their rules
    plain = cli.parser_for(tool).parse_args(['run'])
    assert not hasattr(plain, 'stats') and not hasattr(plain, 'stats_max_duration')


def test_stats_check():
    from clvae_amd import cli
    cli.stats_check(types.SimpleNamespace(stats=False), 40)
    cli.stats_check(types.SimpleNamespace(), 40)
    cli.stats_check(types.SimpleNamespace(stats=True), 88)
    with pytest.raises(SystemExit):
        cli.stats_check(types.SimpleNamespace(stats=True), 40)                           # cl_vae's flattened windows


def test_audit_samples_is_silent_without_the_flag(capsys):
    from clvae_amd import stats
    assert stats.audit_samples([np.zeros((4, 88))], types.SimpleNamespace(stats=False, train_file='none')) is None
    assert stats.audit_samples([np.zeros((4, 88))], types.SimpleNamespace(train_file='none')) is None
    assert stats.audit_samples([], types.SimpleNamespace(stats=True, train_file='none')) is None
    assert capsys.readouterr().out == ""


def test_the_tools_print_their_help():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'clvae_amd.stats', '--help'], capture_output=True, text=True, timeout=120,
                       stdin=subprocess.DEVNULL, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ('--train_file', '--split', '--against', '--rolls', '--max_duration', '--out'):
        assert flag in r.stdout, flag
    for which in ('cl_vae', 'cl_vrnn'):
        script = os.path.join(ROOT, 'classifying-vae-lstm_amd', which, 'sample.py')
        r = subprocess.run([sys.executable, script, '--help'], capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
        assert r.returncode == 0, r.stderr[-2000:]
        assert '--stats' in r.stdout and '--stats_max_duration' in r.stdout
