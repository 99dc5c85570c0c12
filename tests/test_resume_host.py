"""Host side of resumable generation, no GPU: the two declarations and their bindings, what the
launchers refuse before any device work, GenState on CPU tensors, the public calls' refusals, the sample tools' --chunk /
--modulate and every rule between them and the other flags, and the validation of a modulation plan."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import clvae_amd  # noqa: F401
from clvae_amd import _lib, cli, ops, stream as ST
from clvae_amd.engine_generate import (STATE_FIELDS, GenState, VaeGenerate, VrnnGenerate, resume_args, state_widths)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 88
EINVAL = -1


# ------------------------------------------------------------------------------------- declarations and bindings
def test_declarations_and_bindings():
    hdr = open(os.path.join(ROOT, 'include', 'clvae.h')).read()
    C = _lib.C
    for name, n_args in (('clv_vrnn_generate', 35), ('clv_vae_generate', 29)):
        m = re.search(r'\bint %s\(([^;]*?)\);' % name, hdr, re.S)
        assert m, name
        params = [p.strip() for p in m.group(1).split(',')]
        assert len(params) == n_args, name
        # t0, state_in, state_out sit between the two temperatures and the outputs; the roll and the flag before those
        assert params[-10:-8] == ['const uint8_t* clamp', 'int tempered'], name
        assert params[-8:] == ['float inv_temperature', 'float z_temperature', 'uint32_t t0', 'const float* state_in',
                               'float* state_out', 'float* Xs', 'float* xhat', 'void* stream'], name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
        assert argtypes[-10:] == [C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_uint32] + [C.c_void_p] * 5, name
        # both families give their seed frames where they always did: right after the 64-bit seed
        seed = argtypes.index(C.c_uint64)
        assert params[seed:seed + 3] == ['uint64_t seed', 'const float* x_seed', 'const float* w'], name
        assert hdr.count(name + '_resume') == 0 and name + '_resume' not in _lib.SIGNATURES, name
    assert _lib.ABI_VERSION == 610 and re.search(r'#define CLV_ABI_VERSION 610\b', hdr)      # _resume took over clv_*_generate
    for f in (ops.vrnn_generate, ops.vae_generate):
        sig = inspect.signature(f).parameters
        assert sig['t0'].default == 0 and sig['state_in'].default is None and sig['state_out'].default is None
    assert not hasattr(ops, 'vrnn_generate_resume') and not hasattr(ops, 'vae_generate_resume')
    for cls in (VrnnGenerate, VaeGenerate):
        sig = inspect.signature(cls.generate).parameters
        assert sig['state'].default is None and sig['return_state'].default is False
    for which in ('cl_vae', 'cl_vrnn'):
        M = importlib.import_module('clvae_amd.%s.model' % which)
        sig = inspect.signature(M.generate_samples_device).parameters
        assert sig['state'].default is None and sig['return_state'].default is False
        assert 'state' in M.generate_samples_device.__doc__ and 'DESIGN.md 16' in M.generate_samples_device.__doc__


def _vrnn_call(lib, p, **over):
    a = dict(N=1, S=1, nsteps=2, L=2, C=4, gate=0, x_seed=p, w=p, W=[p] * 13, clamp=None, inv_T=1.0, Tz=1.0, t0=0,
             state_in=None, state_out=None, Xs=p, xhat=None)
    a.update(over)
    return lib.clv_vrnn_generate(a['N'], a['S'], a['nsteps'], D, 88, a['L'], a['C'], a['gate'], 0, 1, a['x_seed'], a['w'],
                                 *a['W'], a['clamp'], 1, a['inv_T'], a['Tz'], a['t0'], a['state_in'], a['state_out'], a['Xs'],
                                 a['xhat'], None)


def _vae_call(lib, p, **over):
    a = dict(N=1, nsteps=2, L=2, C=4, x_seed=None, w=p, W=[p] * 8, clamp=None, inv_T=1.0, Tz=1.0, t0=0, state_in=p,
             state_out=None, Xs=p, xhat=None)
    a.update(over)
    return lib.clv_vae_generate(a['N'], a['nsteps'], D, 88, a['L'], a['C'], 1, 0, 1, a['x_seed'], a['w'], *a['W'], a['clamp'],
                                1, a['inv_T'], a['Tz'], a['t0'], a['state_in'], a['state_out'], a['Xs'], a['xhat'], None)


def test_launchers_refuse_before_any_device_work():
    """CLV_EINVAL with no GPU: null required pointers, everything the generate mode refuses, the step overflow, a cl_vae
    call from / to a state without state_in or with a seed frame beside it.  (No accepted call is made here: its pointers are
    host memory.)"""
    lib = _lib.lib()
    p = np.zeros(64 * 1024, np.float32).ctypes.data
    U32 = 2 ** 32 - 1
    nan = float('nan')
    for bad in (dict(w=None), dict(Xs=None), dict(x_seed=None), dict(N=0), dict(S=-1), dict(nsteps=-1), dict(S=0, nsteps=0),
                dict(L=0), dict(L=33), dict(C=0), dict(C=33), dict(gate=7), dict(inv_T=0.0), dict(inv_T=-1.0), dict(inv_T=nan),
                dict(Tz=-1.0), dict(Tz=nan), dict(clamp=p, nsteps=0), dict(N=2 ** 16, nsteps=2 ** 10, clamp=p),
                dict(t0=U32), dict(t0=U32 - 2), dict(t0=U32 - 2, state_in=p, state_out=p),
                dict(t0=2 ** 31, S=2 ** 30, nsteps=2 ** 30 + 1, state_in=p)):
        assert _vrnn_call(lib, p, **bad) == EINVAL, bad
    for k in range(13):
        if k == 6:
            continue                                    # Kx_dec: NULL means a model without use_x_prev
        W = [p] * 13
        W[k] = None
        assert _vrnn_call(lib, p, W=W) == EINVAL, k
    for bad in (dict(state_in=None), dict(state_in=None, state_out=p), dict(state_in=None, t0=1), dict(x_seed=p),
                dict(x_seed=p, state_out=p, t0=3), dict(w=None), dict(Xs=None), dict(N=0), dict(nsteps=0),
                dict(L=0), dict(L=33), dict(C=33), dict(inv_T=0.0), dict(Tz=-1.0), dict(t0=U32), dict(t0=U32 - 1),
                dict(t0=2 ** 31, nsteps=2 ** 31)):
        assert _vae_call(lib, p, **bad) == EINVAL, bad
    for k in range(8):
        W = [p] * 8
        W[k] = None
        assert _vae_call(lib, p, W=W) == EINVAL, k


# ------------------------------------------------------------------------------------------------------ GenState
def _state(kind, N=3, t=7, seed=0):
    rng = np.random.default_rng(seed)
    return GenState(kind, {k: torch.as_tensor(rng.standard_normal((N, D)).astype(np.float32)) for k in STATE_FIELDS[kind]}, t)


@pytest.mark.parametrize("kind", ['cl_vrnn', 'cl_vae'])
def test_state_round_trip_select_and_clone(kind, tmp_path):
    s = _state(kind)
    names = STATE_FIELDS[kind]
    assert s.kind == kind and s.N == 3 and s.t == 7 and tuple(s.rows.shape) == (3, len(names), D)
    assert list(s.tensors()) == list(names) and all(torch.equal(getattr(s, k), s[k]) for k in names)
    # to_numpy -> np.savez -> np.load -> from_numpy
    d = s.to_numpy()
    assert set(d) == set(names) | {'t'} and all(d[k].dtype == np.float32 and d[k].shape == (3, D) for k in names)
    np.savez(str(tmp_path / "state.npz"), **d)
    back = GenState.from_numpy(np.load(str(tmp_path / "state.npz")), 'cpu')
    assert back.kind == kind and back.t == 7 and all(torch.equal(back[k], s[k]) for k in names)
    # select: rows by index, repeats allowed; the original is untouched
    f = s.select([0, 0, 2, 1])
    assert f.N == 4 and f.t == 7 and f.kind == kind
    for k in names:
        assert torch.equal(f[k], s[k][[0, 0, 2, 1]])
    assert torch.equal(s.select(np.array([1]))[names[0]], s[names[0]][1:2])
    assert torch.equal(s.select(torch.tensor([2, 2]))[names[0]], s[names[0]][[2, 2]])
    for bad in ([], [3], [-1], [0.5], [True], [[0, 1]], 1):
        with pytest.raises(ValueError):
            s.select(bad)
    # clone: equal and independent
    c = s.clone()
    c.rows.zero_()
    assert float(s.rows.abs().sum()) > 0 and c.t == s.t
    with pytest.raises(AttributeError):
        s.no_such_field


def test_state_refusals():
    z = lambda *shape: torch.zeros(*shape)
    good = {k: z(2, D) for k in STATE_FIELDS['cl_vrnn']}
    GenState('cl_vrnn', good, 0)
    for bad_t in (-1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError):
            GenState('cl_vrnn', good, bad_t)
    with pytest.raises(ValueError):
        GenState('cl_rnn', good, 0)
    with pytest.raises(ValueError):
        GenState('cl_vae', good, 0)                                     # another family's fields
    with pytest.raises(ValueError):
        GenState('cl_vrnn', dict(good, x=z(3, D)), 0)                   # rows disagree
    with pytest.raises(ValueError):
        GenState('cl_vrnn', dict(good, x=z(2, D).double()), 0)
    with pytest.raises(ValueError):
        GenState('cl_vrnn', dict(good, x=z(D)), 0)
    with pytest.raises(ValueError):
        GenState.from_numpy(dict(x_in=np.zeros((2, D), np.float32), t=np.asarray(0)), 'cpu')        # hist is missing
    with pytest.raises(ValueError):
        GenState.from_numpy(dict(x_in=np.zeros((2, D)), hist=np.zeros((2, D))), 'cpu')               # t is missing
    # a fresh start
    f = GenState.fresh('cl_vrnn', dict(D=D, H=D), 'cpu', N=4)
    assert f.t == 0 and f.N == 4 and float(f.rows.abs().sum()) == 0
    x = np.eye(D)[:2]
    f = GenState.fresh('cl_vae', dict(D=D, H=D), 'cpu', seed_frame=x)
    assert f.t == 0 and torch.equal(f.x_in, f.hist) and np.array_equal(f.x_in.numpy(), x.astype(np.float32))
    with pytest.raises(ValueError):
        GenState.fresh('cl_vae', dict(D=D, H=D), 'cpu', seed_frame=np.zeros((2, 87)))


def test_resume_args():
    cfg = dict(D=D, H=D)
    s = _state('cl_vrnn', t=100)
    W = state_widths('cl_vrnn', cfg)
    assert W == dict(h_enc=D, c_enc=D, h_dec=D, c_dec=D, x=D) and state_widths('cl_vae', cfg) == dict(x_in=D, hist=D)
    assert resume_args(None, 'cl_vrnn', 3, W, 10) == 0 and resume_args(s, 'cl_vrnn', 3, W, 10) == 100
    assert resume_args(_state('cl_vrnn', t=2 ** 32 - 11), 'cl_vrnn', 3, W, 10) == 2 ** 32 - 11     # the last step: 2^32 - 1
    for bad in (dict(state=_state('cl_vae')), dict(N=4), dict(widths=dict(W, x=87)), dict(widths=dict(W, h_enc=64)),
                dict(state=_state('cl_vrnn', t=2 ** 32 - 10)), dict(state='state'), dict(state=s.to_numpy())):
        kw = dict(state=s, kind='cl_vrnn', N=3, widths=W, nframes=10)
        kw.update(bad)
        with pytest.raises(ValueError):
            resume_args(**kw)


# ----------------------------------------------------------------------------------------------- the public calls
class _Engine:
    """an engine that must not be reached: the arguments are checked first"""
    cfg = dict(D=D, C=4, L=2, H=88, T=8, use_x_prev=True)
    device = 'cpu'

    def generate(self, *a, **kw):
        raise AssertionError("the arguments are checked first")


class _Model:
    def __init__(self, kind):
        self.engine = _Engine()
        self.engine.STATE_KIND = kind


@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_public_calls_refuse_with_value_errors(which):
    M = importlib.import_module('clvae_amd.%s.model' % which)
    other = 'cl_vrnn' if which == 'cl_vae' else 'cl_vae'
    model, N, w = _Model(which), 3, np.eye(4)[[0, 1, 2]]
    seeds = np.zeros((N, 2, D)) if which == 'cl_vrnn' else np.zeros((N, D))
    roll = np.full((N, 4, D), 255, np.uint8)
    s = _state(which, N=N)
    gen = lambda seeds_, **kw: M.generate_samples_device(model, seeds_, 4, w, **kw)
    cases = [
        (None, dict(state=s, particles=4, clamp=roll)),                  # a state together with particles
        (seeds, dict(return_state=True, particles=4, clamp=roll)),
        (None, dict(state=_state(other, N=N))),                          # a state of the other family
        (None, dict(state=_state(which, N=N + 1))),                      # wrong N
        (None, dict(state=_state(which, N=N, t=2 ** 32 - 4))),           # t overflow: t + 4 frames > 2^32 - 1
        (None, dict(state=s.to_numpy())),                                # not a GenState
        (None, dict()),                                                  # neither seeds nor a state
        (None, dict(return_state=True)),
        (None, dict(state=s, temperature=0.0)),
    ]
    wide = {k: torch.zeros(N, 64) for k in STATE_FIELDS[which]}
    cases.append((None, dict(state=GenState(which, wide, 0))))           # wrong widths
    if which == 'cl_vae':
        cases.append((seeds, dict(state=s)))                             # cl_vae seeds together with a state
    else:
        cases.append((seeds, dict(state=_state(which, N=N, t=2 ** 32 - 6))))      # S counts too: t + 2 + 4
        cases.append((np.zeros((N, D)), dict(state=s)))                  # seeds that are not [N, S, 88]
    for sd, kw in cases:
        with pytest.raises(ValueError):
            gen(sd, **kw)
    with pytest.raises(ValueError):
        M.generate_samples_device(model, None, 4, np.eye(4)[[0, 1]], state=s)           # w of another N
    with pytest.raises(AssertionError):                                  # and good calls do get through to the engine
        gen(None, state=s, clamp=roll, temperature=0.7)
    with pytest.raises(AssertionError):
        gen(None if which == 'cl_vae' else seeds, state=s, return_state=True)
    with pytest.raises(AssertionError):
        gen(seeds, return_state=True)


# ---------------------------------------------------------------------------------------------------- the tools
def test_parse_modulate():
    assert cli.parse_modulate('G@3', 10) == [('G', 3)]
    assert cli.parse_modulate('G@3, a@7 ,C#@9', 10) == [('G', 3), ('a', 7), ('C#', 9)]
    assert cli.parse_modulate('x@y@2', 10) == [('x@y', 2)]               # the frame follows the last @
    for bad, t in (('G', 10), ('@3', 10), ('G@', 10), ('G@x', 10), ('G@1.5', 10), ('G@0', 10), ('G@-1', 10), ('G@10', 10),
                   ('G@5,a@5', 10), ('G@6,a@5', 10), ('G@3,,a@5', 10), ('', 10), ('G@1', 1)):
        with pytest.raises(ValueError):
            cli.parse_modulate(bad, t)


@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_flag_rules(which, capsys):
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    assert [f.names[0] for f in cli.RESUME_FLAGS] == ['--chunk', '--modulate']
    # the reference's own tables stay verbatim: the flags are this implementation's list
    assert not any(f.names[0] in ('--chunk', '--modulate') for t in cli.TABLES.values() for f in t)
    assert not hasattr(S.build_parser().parse_args(['r']), 'chunk')
    parser = cli.parser_for('%s.sample' % which, cli.DEVICE_LOOP_FLAGS + cli.HARMONIZE_FLAGS + cli.TEMPERATURE_FLAGS
                            + cli.VARY_FLAGS + cli.MORPH_FLAGS + cli.RESUME_FLAGS)
    a = parser.parse_args(['r'])
    assert a.chunk is None and a.modulate is None and not cli.resuming(a)
    assert cli.resume_kwargs(a, {'G': 1}, 2, 4) == {}
    a = parser.parse_args(['r', '-t', '10', '--chunk', '4', '--temperature', '0.8', '--z_temperature', '0.5', '--harmonize', 'top'])
    assert a.chunk == 4 and cli.resuming(a) and cli.resume_kwargs(a, {'G': 1}, 2, 4) == dict(chunk=4)
    a = parser.parse_args(['r', '-t', '10', '--modulate', 'G@3,a@7', '--device_loop'])
    kw = cli.resume_kwargs(a, {'G': 1, 'a': 3}, 2, 4)
    assert kw['chunk'] is None and [f for f, _ in kw['changes']] == [3, 7]
    assert np.array_equal(kw['changes'][0][1], np.eye(4)[[1, 1]]) and np.array_equal(kw['changes'][1][1], np.eye(4)[[3, 3]])
    with pytest.raises(ValueError):
        cli.resume_kwargs(a, {'G': 1}, 2, 4)                              # a name the key map does not hold
    assert parser.parse_args(['r', '--chunk', '1', '--modulate', 'G@31']).modulate == 'G@31'         # -t defaults to 32
    for bad in (['--chunk', '0'], ['--chunk', '-2'], ['--chunk', 'x'], ['--chunk', '4', '--host_loop'], ['--chunk', '4', '--vary'],
                ['--chunk', '4', '--morph', '2'], ['--chunk', '4', '--harmonize', 'top', '--particles', '4'],
                ['--modulate', 'G@3', '--host_loop'], ['--modulate', 'G@3', '--vary'], ['--modulate', 'G@3', '--morph', '2'],
                ['--modulate', 'G@3', '--harmonize', 'bottom', '--particles', '2'], ['--modulate', 'G'], ['--modulate', 'G@0'],
                ['--modulate', 'G@32'], ['--modulate', 'G@5', '-t', '5'], ['--modulate', 'G@4,a@4'], ['--modulate', 'G@5,a@4']):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(['r'] + bad)
        assert e.value.code == 2, bad
    capsys.readouterr()
    if which == 'cl_vae':           # both imply the device loop
        assert S.on_device(parser.parse_args(['r', '--chunk', '4'])) and S.on_device(parser.parse_args(['r', '--modulate', 'G@3']))
        assert not S.on_device(parser.parse_args(['r']))
    src = open(S.__file__).read()
    assert 'RESUME_FLAGS' in src.split("if __name__ == '__main__':")[1]


def test_chunk_bounds():
    assert ST.chunk_bounds(10, 4) == [(0, 4), (4, 8), (8, 10)]
    assert ST.chunk_bounds(10, None) == [(0, 10)]
    assert ST.chunk_bounds(10, 4, [5]) == [(0, 4), (4, 5), (5, 8), (8, 10)]
    assert ST.chunk_bounds(8, 4, [4]) == [(0, 4), (4, 8)]
    assert ST.chunk_bounds(3, 10) == [(0, 3)]


def test_plan_validation():
    w = np.eye(4)[[0, 1]]
    plan = ST.check_plan([(w, 5), (w[::-1], np.int64(6))], 2, 4)
    assert [n for _, n in plan] == [5, 6] and plan[0][0].dtype == np.float64 and np.array_equal(plan[1][0], w[::-1])
    for bad in ([], None, 5, [(w, 5, 1)], [(w,)], [(w, 0)], [(w, -1)], [(w, 1.5)], [(w, True)], [(w, 5), (np.eye(4)[[0]], 6)],
                [(np.eye(3)[[0, 1]], 5)], [(w[0], 5)], [w, 5]):
        with pytest.raises(ValueError):
            ST.check_plan(bad, 2, 4)
    with pytest.raises(ValueError):
        ST.modulate(_Model('cl_vrnn'), np.zeros((2, 1, D)), [(w, 5)], temperature=0.0)
    with pytest.raises(ValueError):
        ST.modulate(_Model('cl_vrnn'), np.zeros((2, 1, D)), [(w, 5)], z_prior=True)          # not a temperature
    with pytest.raises(ValueError):
        ST.modulate(_Model('cl_vrnn'), np.zeros((2, 1, D)), [(w, 0)])
    with pytest.raises(ValueError):
        ST.Stream(type('M', (), {'engine': object()})(), np.zeros((2, 1, D)), w)              # neither family's model


# ------------------------------------------------------------------------------ cl_vae: frames are read as on / off
class _VaeHost(VaeGenerate):
    """the cl_vae sampling mixin without a device: its refusals come before its first launch"""
    cfg = dict(D=D, C=4, L=2, H=88, T=8, use_x_prev=True)
    device = 'cpu'


def test_cl_vae_generate_refuses_frames_that_are_not_binary():
    w = torch.eye(4)[[0, 1]]
    good = torch.zeros(2, D)
    good[0, 5] = 1.0
    for entry in (0.5, 2.0, float('nan')):
        bad = good.clone()
        bad[1, 64] = entry
        by_hand = GenState('cl_vae', dict(x_in=good, hist=bad), 3)
        loaded = GenState.from_numpy(dict(x_in=bad.numpy(), hist=good.numpy(), t=np.int64(3)), 'cpu')
        for persistent in (True, False):
            kw = dict(persistent=persistent)
            with pytest.raises(ValueError, match='on/off'):
                _VaeHost().generate(bad, w, 4, **kw)
            with pytest.raises(ValueError, match='on/off'):
                _VaeHost().generate(bad, w, 4, return_state=True, **kw)
            for state in (by_hand, loaded, by_hand.clone(), loaded.select([1, 1]), GenState.fresh('cl_vae', _VaeHost.cfg, 'cpu', seed_frame=bad)):
                assert not state.binary
                with pytest.raises(ValueError, match='on/off'):
                    _VaeHost().generate(None, w, 4, state=state, **kw)
    # what a sampler returns is marked, and its copies and selections with it: those rows are not read again
    st = GenState('cl_vae', dict(x_in=good, hist=good), 3)._sampled()
    assert st.binary and st.clone().binary and st.select([0, 0]).binary
    assert not GenState.from_numpy(st.to_numpy(), 'cpu').binary
