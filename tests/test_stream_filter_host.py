"""CPU tests of the filter stream's host surface: the three ABI additions in header, library and binding,
the sample tools' --live / --max_lag flags and their refusals, FilterStream's refusals and its bookkeeping over a stand-in
engine, FilterState's round trip."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import clvae_amd  # noqa: F401,E402
from clvae_amd import _lib, cli  # noqa: E402
from clvae_amd.engine_generate import Constraints, FilterEmit, FilterState, GenState, chunk_frames  # noqa: E402
from clvae_amd.harmonize import FREE, accompany  # noqa: E402
from clvae_amd.stream import FilterStream  # noqa: E402
from helpers import ROOT  # noqa: E402

ENTRIES = ('clv_smc_resample_carry', 'clv_smc_commit', 'clv_smc_collapse')


# ------------------------------------------------------------------ the ABI additions
def test_header_library_and_binding_hold_the_three_entries():
    hdr = open(os.path.join(ROOT, "include", "clvae.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = dict(re.findall(r"\b(clv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", code))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in protos, name
        assert hasattr(lib, name), name
        restype, argtypes = _lib.SIGNATURES[name]
        args = [a.strip() for a in protos[name].split(",")]
        assert restype is ctypes.c_int and len(args) == len(argtypes), name
        for a, t in zip(args, argtypes):
            if "*" in a:
                assert t is ctypes.c_void_p, (name, a)
            elif re.match(r"(uint64_t|int64_t)\b", a):
                assert ctypes.sizeof(t) == 8, (name, a)
            elif re.match(r"double\b", a):
                assert t is ctypes.c_double, (name, a)
            else:
                assert ctypes.sizeof(t) == 4 and t is not ctypes.c_float, (name, a)
    # the carry entry is clv_smc_resample plus (uint32_t t0, int carry) in front of the stream
    base, carry = [[a.strip() for a in protos[n].split(",")] for n in ('clv_smc_resample', 'clv_smc_resample_carry')]
    assert carry == base[:-1] + ['uint32_t t0', 'int carry'] + base[-1:]


def test_additions_keep_the_abi_version():
    hdr = open(os.path.join(ROOT, "include", "clvae.h")).read()
    assert _lib.ABI_VERSION == 610 and int(re.search(r"#define\s+CLV_ABI_VERSION\s+(\d+)", hdr).group(1)) == 610
    assert _lib.lib().clv_version() == 610
    assert re.search(r"still 610: \+ clv_smc_resample_carry", hdr)


def test_the_collapse_stream_is_in_the_stream_map_and_free():
    from clvae_amd import trainer
    src = open(os.path.join(ROOT, "classifying-vae-lstm_amd", "csrc", "smc.hip")).read()
    assert trainer.COLLAPSE_STREAM == 0xFFFFFFF8
    assert re.search(r"COLLAPSE_STREAM\s*=\s*0xFFFFFFF8u", src)
    streams = [v for k, v in vars(trainer).items() if k.endswith('_STREAM') or k.startswith('IW_STREAM')]
    assert len(streams) == len(set(streams))


# ------------------------------------------------------------------ the flags
LIVE_SET = cli.DEVICE_LOOP_FLAGS + cli.HARMONIZE_FLAGS + cli.VARY_FLAGS + cli.MORPH_FLAGS + cli.RESUME_FLAGS \
    + cli.GIBBS_FLAGS + cli.LIVE_FLAGS


@pytest.mark.parametrize("tool", ['cl_vae.sample', 'cl_vrnn.sample'])
def test_live_flags_parse_and_are_refused_where_they_do_not_apply(tool):
    p = cli.parser_for(tool, LIVE_SET)
    base = ['run', '--harmonize', 'top', '--particles', '8']
    ns = p.parse_args(base + ['--live', '4'])
    assert ns.live == 4 and ns.max_lag is None and cli.live_kwargs(ns) == (4, dict(max_lag=None))
    ns = p.parse_args(base + ['--live', '4', '--max_lag', '2'])
    assert cli.live_kwargs(ns) == (4, dict(max_lag=2))
    assert cli.live_kwargs(p.parse_args(base)) == (None, {})
    assert cli.live_kwargs(types.SimpleNamespace()) == (None, {})
    for extra in (['--sweeps', '2'], ['--infer_key', 'discrete'], ['--chunk', '2'], ['--modulate', 'C@2'], ['--host_loop']):
        with pytest.raises(SystemExit):
            p.parse_args(base + ['--live', '4'] + extra)
    for argv in (['run', '--vary', '--live', '4'], ['run', '--morph', '2', '--live', '4'],      # neither takes --particles
                 ['run', '--harmonize', 'top', '--live', '4'], ['run', '--live', '4'],          # --live needs the filter
                 base + ['--live', '0'], base + ['--max_lag', '2'], base + ['--live', '4', '--max_lag', '-1']):
        with pytest.raises(SystemExit):
            p.parse_args(argv)


def test_both_sample_tools_take_the_live_flags():
    for which in ('cl_vae', 'cl_vrnn'):
        src = open(os.path.join(ROOT, "classifying-vae-lstm_amd", which, "sample.py")).read()
        assert re.search(r"NOVELTY_FLAGS \+ LIVE_FLAGS\)\.parse_args\(\)", src) and 'live_harmonize(' in src


# ------------------------------------------------------------------ FilterStream's refusals
def _model(kind='cl_vae', engine=None):
    engine = engine or types.SimpleNamespace()
    engine.STATE_KIND, engine.cfg = kind, dict(D=88, C=3)
    return types.SimpleNamespace(engine=engine)


def test_filter_stream_refusals_come_before_the_model_is_touched():
    nothing = types.SimpleNamespace(engine=None)
    x, w = np.zeros((2, 88)), np.eye(3)[[0, 1]]
    for kw in (dict(w_prior=object()), dict(infer_key='discrete'), dict(sweeps=2), dict(n_out=2), dict(n_out=True),
               dict(nonsense=1)):
        with pytest.raises(ValueError):
            FilterStream(nothing, x, w, 4, **kw)
    for particles in (0, -1, 2.5, 4.0, True, None, '4'):
        with pytest.raises(ValueError):
            FilterStream(nothing, x, w, particles)
    for lag in (-1, 1.5, True):
        with pytest.raises(ValueError):
            FilterStream(nothing, x, w, 4, max_lag=lag)
    for tau in (-0.1, 1.5):
        with pytest.raises(ValueError):
            FilterStream(nothing, x, w, 4, resample_threshold=tau)
    with pytest.raises(ValueError):
        accompany(nothing, x, None, particles=4)                    # no key per particle: a label is needed
    with pytest.raises(ValueError):
        accompany(nothing, x, w, voice='middle', particles=4)
    FilterStream(_model(), x, w, 4, n_out=1, max_lag=0)             # what one path per melody means anyway
    for bad_x, bad_w in ((np.zeros((2, 4, 88)), w), (x, np.eye(3)), (np.zeros((2, 87)), w)):
        with pytest.raises(ValueError):
            FilterStream(_model(), bad_x, bad_w, 4)
    with pytest.raises(ValueError):
        FilterStream(_model('cl_vrnn'), x, w, 4)                    # cl_vrnn seeds are [N, S, 88]


class _Engine:
    """A stand-in for the engine's filter: every advance of n frames commits floor(pending / 2) frames of melody 0 and all
    of melody 1; frames carry the index of the step they belong to in note 0."""

    def __init__(self):
        self.calls = []

    def _state(self, state, n):
        if state is None:
            state = types.SimpleNamespace(len=np.zeros(2, np.int64), done=np.zeros(2, np.int64), t=0, logZ=torch.zeros(2),
                                          collapses=torch.zeros(2, dtype=torch.int32))
            state.pending = lambda: state.len.copy()
        state.len = state.len + n
        state.t += n
        return state

    def _emit(self, state, counts, picks=None):
        frames = torch.zeros(2, int(counts.max()), 88, dtype=torch.uint8)
        for m in range(2):
            frames[m, :counts[m], 0] = torch.arange(state.done[m], state.done[m] + counts[m], dtype=torch.uint8)
        state.done = state.done + counts
        state.len = state.len - counts
        return FilterEmit(state, frames, counts, torch.ones(2, 1, dtype=torch.float64), np.full(2, -1) if picks is None else picks)

    def filter_advance(self, state, x_seed, w, clamp, particles, tau, **kw):
        self.calls.append(('advance', state is None, x_seed is None, chunk_frames(clamp), kw))
        state = self._state(state, chunk_frames(clamp))
        return self._emit(state, np.array([state.len[0] // 2, state.len[1]]))

    def filter_collapse(self, state, index, seed=0, final=False):
        self.calls.append(('finish' if final else 'collapse', None if index is None else list(index)))
        which = np.ones(2, bool) if index is None else np.isin(np.arange(2), index)
        if not final:
            state.collapses += torch.as_tensor(which.astype(np.int32))
        return self._emit(state, np.where(which, state.len, 0), np.where(which, 1, -1))


def test_filter_stream_bookkeeping_over_a_stand_in_engine():
    eng = _Engine()
    s = FilterStream(_model(engine=eng), np.zeros((2, 88)), np.eye(3)[[0, 1]], 4, seed=9)
    assert np.array_equal(s.pending, [0, 0]) and s.t == 0 and [e.shape for e in s.emitted] == [(0, 88), (0, 88)]
    with pytest.raises(ValueError):
        s.collapse()
    with pytest.raises(ValueError):
        s.finish()
    roll = np.full((2, 3, 88), FREE, np.uint8)
    frames, counts = s.advance(roll)
    assert frames.dtype == np.float64 and frames.shape == (2, 3, 88) and np.array_equal(counts, [1, 3])
    assert np.array_equal(s.pending, [2, 0]) and s.t == 3 and s.ess.shape == (2, 1)
    assert eng.calls[0][:4] == ('advance', True, False, 3) and eng.calls[0][4]['seed'] == 9
    frames, counts = s.advance(Constraints.between(1, 4, roll=roll[:, :2]), temperature=0.8)
    assert np.array_equal(counts, [2, 2]) and eng.calls[1][:4] == ('advance', False, True, 2)
    assert eng.calls[1][4]['temperature'] == 0.8
    with pytest.raises(ValueError):
        s.advance(roll, temperature=0.0)
    with pytest.raises(ValueError):
        s.advance(roll, w=np.eye(3)[[1, 0]])                # the label is the stream's
    with pytest.raises(ValueError):
        s.fork()
    frames, counts = s.collapse([0])
    assert np.array_equal(counts, [2, 0]) and np.array_equal(s.picks, [1, -1]) and np.array_equal(s.collapses, [1, 0])
    frames, counts = s.finish()
    assert np.array_equal(counts, [0, 0]) and s.finished and np.array_equal(s.pending, [0, 0])
    for m, e in enumerate(s.emitted):                       # every frame once, in order
        assert e.shape == (5, 88) and np.array_equal(e[:, 0], np.arange(5))
    for call in (lambda: s.advance(roll), s.collapse, s.finish):
        with pytest.raises(ValueError):
            call()


def test_max_lag_collapses_the_melodies_that_fall_behind():
    eng = _Engine()
    s = FilterStream(_model(engine=eng), np.zeros((2, 88)), np.eye(3)[[0, 1]], 4, max_lag=2)
    roll = np.full((2, 4, 88), FREE, np.uint8)
    frames, counts = s.advance(roll)                        # melody 0 commits 2 of 4: 2 pending, within the lag
    assert np.array_equal(counts, [2, 4]) and np.array_equal(s.pending, [2, 0]) and np.array_equal(s.collapses, [0, 0])
    frames, counts = s.advance(roll)                        # 6 pending, 3 commit, 3 left: collapsed, all 6 go out in order
    assert np.array_equal(counts, [6, 4]) and np.array_equal(s.pending, [0, 0]) and np.array_equal(s.collapses, [1, 0])
    assert np.array_equal(frames[0, :6, 0], np.arange(2, 8)) and eng.calls[-1] == ('collapse', [0])
    assert np.array_equal(s.emitted[0][:, 0], np.arange(8))


# ------------------------------------------------------------------ FilterState
def _state(kind, N=2, P=3, D=88, cap=4):
    rng = np.random.default_rng(5)
    R = N * P
    n = 5 if kind == 'cl_vrnn' else 2
    gen = GenState(kind, None, 17, rows=torch.as_tensor(rng.random((R, n, D)).astype(np.float32)))
    i32 = lambda a: torch.as_tensor(np.asarray(a, np.int32))
    return FilterState(gen, P, logW=torch.as_tensor(rng.standard_normal(R)), logZ=torch.as_tensor(rng.standard_normal(N)),
                       nres=i32([3, 1]), collapses=i32([0, 2]), pend_anc=i32(rng.integers(0, R, (cap, R))),
                       pend_hist=torch.as_tensor(rng.integers(0, 2, (cap, R, D)).astype(np.uint8)), head=i32([3, 1]),
                       len=i32([2, 4]))


@pytest.mark.parametrize("kind", ['cl_vrnn', 'cl_vae'])
def test_filter_state_round_trip_clone_and_reserve(kind, tmp_path):
    s = _state(kind)
    assert (s.N, s.P, s.R, s.D, s.cap, s.t, s.kind) == (2, 3, 6, 88, 4, 17, kind) and np.array_equal(s.pending(), [2, 4])
    np.savez(str(tmp_path / "s.npz"), **s.to_numpy())
    back = FilterState.from_numpy(np.load(str(tmp_path / "s.npz")), torch.device('cpu'))
    c = s.clone()
    for other in (back, c):
        assert other.P == s.P and other.t == s.t and other.kind == kind
        assert torch.equal(other.gen.rows, s.gen.rows)
        for k in FilterState.ARRAYS:
            a, b = getattr(other, k), getattr(s, k)
            assert a.dtype == b.dtype and torch.equal(a, b) and a.data_ptr() != b.data_ptr(), k
    # a larger ring holds every melody's live steps in order from slot 0 on
    live = [[(s.pend_anc[(int(s.head[m]) + j) % 4, m * 3:(m + 1) * 3].clone(),
              s.pend_hist[(int(s.head[m]) + j) % 4, m * 3:(m + 1) * 3].clone()) for j in range(int(s.len[m]))] for m in range(2)]
    s.reserve(3)
    assert s.cap == 4
    s.reserve(5)
    assert s.cap >= 5 and np.array_equal(s.head.numpy(), [0, 0]) and np.array_equal(s.pending(), [2, 4])
    for m in range(2):
        for j, (a, h) in enumerate(live[m]):
            assert torch.equal(s.pend_anc[j, m * 3:(m + 1) * 3], a) and torch.equal(s.pend_hist[j, m * 3:(m + 1) * 3], h)
    with pytest.raises(ValueError):
        FilterState.from_numpy(dict(t=np.asarray(0)), torch.device('cpu'))
    with pytest.raises(ValueError):
        FilterState(s.gen, 4, **{k: getattr(s, k) for k in FilterState.ARRAYS})     # 4 particles do not divide 6 rows


def test_chunk_frames():
    roll = np.zeros((2, 5, 88), np.uint8)
    assert chunk_frames(roll) == 5 and chunk_frames(torch.zeros(2, 3, 88, dtype=torch.uint8)) == 3
    assert chunk_frames(Constraints.between(1, 2, roll=roll)) == 5
    assert chunk_frames(Constraints(None, np.zeros((2, 7, 2), np.uint8))) == 7
    for bad in (None, Constraints.exactly(3), np.zeros((2, 88), np.uint8), np.zeros((2, 0, 88), np.uint8)):
        with pytest.raises(ValueError):
            chunk_frames(bad)
