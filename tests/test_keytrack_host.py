"""CPU tests of key tracking: the C ABI surface of the two entry points, the library's and track()'s
refusals, KeyTrack's segment bookkeeping, the reference HMM of tests/keytrack_reference.py against brute-force enumeration,
and the two keys.py tools' argument surfaces."""
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

import clvae_amd  # noqa: F401
import keytrack_reference as KR
from clvae_amd import _lib
from helpers import ROOT


def _protos():
    hdr = open(os.path.join(ROOT, "include", "clvae.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return dict(re.findall(r"\b(clv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))


def test_both_entries_are_declared_and_bound_with_their_argument_counts():
    protos = _protos()
    for name, nargs in (('clv_key_track_windows', 19), ('clv_key_track_smooth', 12)):
        assert name in protos, name
        assert len(protos[name].split(',')) == nargs
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
        assert hasattr(_lib.lib(), name)
    w = _lib.SIGNATURES['clv_key_track_windows'][1]
    assert w[14] is ctypes.c_uint64 and w[15] is ctypes.c_int64               # seed, piece0
    assert _lib.SIGNATURES['clv_key_track_smooth'][1][6] is ctypes.c_double      # kappa


def test_abi_version_and_the_reserved_stream():
    from clvae_amd import trainer
    assert _lib.ABI_VERSION == 610 and _lib.lib().clv_version() == 610
    assert trainer.KEY_STREAM == 0xFFFFFFFB == KR.KEY_STREAM
    reserved = [trainer.IW_STREAM_W, trainer.IW_STREAM_Z, trainer.SMC_STREAM, trainer.SMC_W_STREAM, trainer.KEY_STREAM]
    assert len(set(reserved)) == len(reserved)
    src = open(os.path.join(ROOT, "classifying-vae-lstm_amd", "csrc", "key_track.hip")).read()
    assert re.search(r"KT_STREAM\s*=\s*0xFFFFFFFBu", src)


def _windows_args(**kw):
    """a well-formed argument list (pointers: any non-NULL, 8-byte aligned value; the entry refuses before it reads them)"""
    p = ctypes.c_void_p(4096)
    a = dict(N=1, T=4, D=88, Hd=88, C=5, hop=1, K=0, frames=p, piece_off=p, win_off=p, Kh=p, bh=p, Ka=p, ba=p, seed=0, piece0=0,
             wargs=p, logp=p, stream=None)
    a.update(kw)
    return [a[k] for k in ('N', 'T', 'D', 'Hd', 'C', 'hop', 'K', 'frames', 'piece_off', 'win_off', 'Kh', 'bh', 'Ka', 'ba', 'seed',
                           'piece0', 'wargs', 'logp', 'stream')]


def _smooth_args(**kw):
    p = ctypes.c_void_p(4096)
    a = dict(N=1, C=5, win_off=p, logp=p, log_prior=None, log_trans=p, kappa=1.0, post=p, path=p, log_evidence=p, piece_post=p,
             stream=None)
    a.update(kw)
    return [a[k] for k in ('N', 'C', 'win_off', 'logp', 'log_prior', 'log_trans', 'kappa', 'post', 'path', 'log_evidence',
                           'piece_post', 'stream')]


@pytest.mark.parametrize("bad", [dict(frames=None), dict(piece_off=None), dict(win_off=None), dict(Kh=None), dict(bh=None),
                                 dict(Ka=None), dict(ba=None), dict(wargs=None), dict(logp=None), dict(C=1), dict(C=33),
                                 dict(D=87), dict(D=130), dict(Hd=87), dict(Hd=130), dict(hop=0), dict(K=1025), dict(K=-1),
                                 dict(T=0), dict(T=94), dict(N=0), dict(piece0=-1)])
def test_the_windows_entry_refuses_before_the_device(bad):
    """CLV_EINVAL (-1) on a machine without a GPU: nothing was launched"""
    assert _lib.lib().clv_key_track_windows(*_windows_args(**bad)) == -1


@pytest.mark.parametrize("bad", [dict(win_off=None), dict(logp=None), dict(log_trans=None), dict(post=None), dict(path=None),
                                 dict(log_evidence=None), dict(piece_post=None), dict(C=1), dict(C=33), dict(N=0),
                                 dict(kappa=0.0), dict(kappa=-0.5), dict(kappa=1.5), dict(kappa=float('nan'))])
def test_the_smoothing_entry_refuses_before_the_device(bad):
    assert _lib.lib().clv_key_track_smooth(*_smooth_args(**bad)) == -1


# ------------------------------------------------------------------------------------------------------------ track()
def _fake_model(T=4, C=5, D=88):
    """what track() reads before it touches the device"""
    return types.SimpleNamespace(engine=types.SimpleNamespace(cfg=dict(D=D, C=C, T=T)))


def test_track_refuses_with_value_errors():
    from clvae_amd.keytrack import track
    m, C = _fake_model(), 5
    ok = np.zeros((10, 88))
    A = KR.sticky(C, 1, 64)
    bad_calls = [
        dict(pieces=[np.zeros((10, 87))]),                            # a wrong frame width
        dict(pieces=np.zeros((2, 10, 80))),
        dict(pieces=[np.zeros(88)]),
        dict(pieces=[]),
        dict(pieces=[np.full((10, 88), 2.0)]),                        # not binary
        dict(pieces=[np.full((10, 88), 0.5)]),
        dict(pieces=[ok], hop=0), dict(pieces=[ok], hop=-1), dict(pieces=[ok], hop=1.5), dict(pieces=[ok], hop=True),
        dict(pieces=[ok], samples=-1), dict(pieces=[ok], samples=1025), dict(pieces=[ok], samples=2.0),
        dict(pieces=[ok], prior=np.full(4, 0.25)),                    # shape
        dict(pieces=[ok], prior=np.full(5, 0.3)),                     # not normalised
        dict(pieces=[ok], prior=np.array([0.5, 0.5, 0.0, 0.0, 0.0])),  # a zero entry
        dict(pieces=[ok], trans=np.full((5, 4), 0.25)),
        dict(pieces=[ok], trans=A * 1.1),
        dict(pieces=[ok], trans=np.eye(5)),
        dict(pieces=[ok], kappa=0.0), dict(pieces=[ok], kappa=-1.0), dict(pieces=[ok], kappa=1.01),
        dict(pieces=[ok], kappa=float('nan')),
        dict(pieces=[ok], hop=64, expected_segment=64),               # the sticky matrix needs hop < expected_segment
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            track(m, **kw)


def _kt(hop, T, lengths, paths, C=4):
    from clvae_amd.keytrack import KeyTrack, window_counts
    counts = window_counts(lengths, T, hop)
    assert [len(p) for p in paths] == counts
    z = [np.zeros((c, 1)) for c in counts]
    pp = np.full((len(lengths), C), 1.0 / C)
    pp[:, 2] += 0.1
    return KeyTrack(T, hop, C, lengths, [np.arange(c) * hop for c in counts], z, z, z, [np.asarray(p, np.int32) for p in paths],
                    pp, np.zeros(len(lengths)))


def test_segments_and_modulation_cover_a_piece_exactly():
    # hop 1, T 4, 10 frames -> 7 windows; the last window speaks for frames 6..9
    kt = _kt(1, 4, [10, 3, 0], [[0, 0, 1, 1, 1, 3, 3], [], []])
    assert kt.segments(0) == [(0, 0, 2), (1, 2, 3), (3, 5, 5)]
    assert kt.segments(1) == [(2, 0, 3)]                  # no window: one segment in key(n)
    assert kt.segments(2) == []
    assert kt.key(1) == 2
    # hop 3, T 4, 17 frames -> 5 windows at 0, 3, 6, 9, 12; the tail 15, 16 belongs to the last
    kt3 = _kt(3, 4, [17, 4], [[1, 1, 2, 2, 2], [3]])
    assert kt3.segments(0) == [(1, 0, 6), (2, 6, 11)]
    assert kt3.segments(1) == [(3, 0, 4)]
    rng = np.random.default_rng(0)
    for hop, T in ((1, 4), (3, 4), (4, 4), (5, 2), (2, 7)):
        from clvae_amd.keytrack import window_counts
        lengths = [int(v) for v in rng.integers(0, 40, 12)] + [T - 1, T, T + 1, T + hop, T + hop + 1]
        paths = [rng.integers(0, 4, c) for c in window_counts(lengths, T, hop)]
        k = _kt(hop, T, lengths, paths)
        for n, P in enumerate(lengths):
            segs = k.segments(n)
            assert KR.segments_cover(segs, P), (hop, T, P, segs)
            assert all(a[0] != b[0] for a, b in zip(segs, segs[1:]))           # a new segment is a new key
            mod = k.modulation(n)
            assert [nf for _, nf in mod] == [s[2] for s in segs] and sum(nf for _, nf in mod) == P
            for (w, _), s in zip(mod, segs):
                assert w.shape == (1, 4) and w[0, s[0]] == 1 and w.sum() == 1
            if P:
                from clvae_amd.stream import check_plan
                check_plan(mod, 1, 4)                      # the list stream.modulate takes
    lab = kt.labels()
    assert lab.shape == (3, 4) and (lab.argmax(1) == 2).all() and (lab.sum(1) == 1).all()


# ------------------------------------------------------------------------------------------------- the reference HMM
@pytest.mark.parametrize("J", [1, 5])
@pytest.mark.parametrize("kappa", [1.0, 0.25])
def test_reference_hmm_against_all_paths(J, kappa):
    rng = np.random.default_rng(10 * J + int(4 * kappa))
    C = 3
    logp = np.log(rng.dirichlet(np.ones(C), J))
    logp[J // 2] = [-80.0, 0.0, -80.0]                   # a one-hot-sharp row
    prior = rng.dirichlet(np.ones(C))
    trans = rng.dirichlet(np.ones(C), C)
    for lp in (np.log(prior), None):
        r = KR.smooth(logp, lp, np.log(trans), kappa)
        b = KR.brute(logp, lp, np.log(trans), kappa)
        np.testing.assert_allclose(r['post'], b['post'], atol=1e-12)
        np.testing.assert_allclose(r['post'].sum(1), 1.0, atol=1e-12)
        assert abs(r['log_evidence'] - b['log_evidence']) < 1e-12 * max(1.0, abs(b['log_evidence']))
        assert abs(r['best'] - b['best']) < 1e-12 * max(1.0, abs(b['best']))
        assert abs(KR.path_score(r['path'], logp, lp, np.log(trans), kappa) - b['best']) < 1e-12 * max(1.0, abs(b['best']))
        z = (np.log(prior) if lp is not None else np.full(C, -np.log(C))) + kappa * logp.sum(0)
        np.testing.assert_allclose(r['piece_post'], np.exp(z - KR.logsumexp(z)), atol=1e-14)
    e = KR.smooth(np.zeros((0, C)), np.log(prior), np.log(trans), kappa)
    np.testing.assert_allclose(e['piece_post'], prior, atol=1e-15)
    assert e['log_evidence'] == 0.0 and e['post'].shape == (0, C)


def test_reference_windows_and_logp_bounds():
    rng = np.random.default_rng(3)
    piece = (rng.random((11, 6)) < 0.3).astype(np.float64)
    for T, hop, J in ((4, 1, 8), (4, 3, 3), (4, 4, 2), (11, 1, 1), (12, 1, 0), (1, 2, 6)):
        X, starts = KR.windows(piece, T, hop)
        assert X.shape == (J, T * 6) and KR.n_windows(11, T, hop) == J
        for j, t in enumerate(starts):
            np.testing.assert_array_equal(X[j].reshape(T, 6), piece[t:t + T])
    wargs = rng.standard_normal((7, 8))
    lp, b = KR.logp0(wargs, np.zeros_like(wargs))
    np.testing.assert_allclose(np.exp(lp).sum(1), 1.0, atol=1e-14)
    assert (b > 0).all() and (b < 1e-4).all()
    # an fp32 evaluation of the same contract stays inside the bound
    s32 = np.concatenate([wargs[:, :4].astype(np.float32), np.zeros((7, 1), np.float32)], 1)
    m32 = s32.max(1, keepdims=True)
    lp32 = s32 - (m32 + np.log(np.exp(s32 - m32).sum(1, keepdims=True, dtype=np.float32)))
    lp_r, b_r = KR.logp0(wargs[:, :].astype(np.float32), np.zeros_like(wargs))
    assert (np.abs(lp32 - lp_r) <= b_r).all()
    eps = rng.standard_normal((3, 7, 4))
    lk, bk = KR.logpK(wargs, eps)
    assert lk.shape == (7, 5) and (bk > 0).all()
    np.testing.assert_allclose(KR.logpK(wargs, eps[:1] * 0)[0], KR.logp0(wargs, np.zeros_like(wargs))[0], atol=1e-14)
    assert KR.eps_index(3, 7, 2) == ((3 << 24) + 7) * 32 + 2


# ----------------------------------------------------------------------------------------------------------- the tools
@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_keys_tools_print_their_help(which):
    script = os.path.join(ROOT, 'classifying-vae-lstm_amd', which, 'keys.py')
    r = subprocess.run([sys.executable, script, '--help'], capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ('run_name', '-i', '--train_file', '--split', '--hop', '--samples', '--seed', '--expected_segment', '--out'):
        assert flag in r.stdout, flag
