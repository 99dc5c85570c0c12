"""No GPU: the host side of voice-count constraints: engine_generate.Constraints and its checks, the routes a
plain roll, a voiceless Constraints and one with voices take (ops monkeypatched), the --voices flag, the two C entries'
bindings and their refusals on host pointers, and the pinned signatures."""
import ctypes
import inspect

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import clvae_amd  # noqa: F401
from clvae_amd import _lib, cli, ops
from clvae_amd import engine_generate as EG
from clvae_amd.engine_generate import Constraints
from clvae_amd.harmonize import voice_constraints, voice_counts

FREE = 255
D = 88
CPU = torch.device('cpu')


def _pairs(N, T, lo, hi):
    return np.broadcast_to(np.array([lo, hi], np.uint8), (N, T, 2)).copy()


# ------------------------------------------------------------------ Constraints
def test_helpers_build_the_pairs():
    c = Constraints.exactly(4)
    assert c.voices == (4, 4) and c.roll is None
    assert Constraints.between(3, 4).voices == (3, 4) and Constraints(voices=4).voices == (4, 4)
    assert Constraints(voices=[2, 5]).voices == (2, 5)
    src = np.zeros((2, 3, D))
    src[0, 0, [3, 9, 40]] = 1
    src[1, 2, 5] = 0.5
    a = Constraints.as_in(src)
    assert a.voices.dtype == np.uint8 and a.voices.shape == (2, 3, 2)
    assert a.voices[0, 0].tolist() == [3, 3] and a.voices[1, 2].tolist() == [1, 1] and a.voices[0, 1].tolist() == [0, 0]
    roll = np.full((2, 3, D), FREE, np.uint8)
    assert Constraints.exactly(1, roll=roll).roll is roll
    for bad in (lambda: Constraints.exactly(16), lambda: Constraints.exactly(-1), lambda: Constraints.between(4, 3),
                lambda: Constraints.exactly(True), lambda: Constraints.exactly(2.0), lambda: Constraints(voices=(1, 2, 3)),
                lambda: Constraints(voices='four'), lambda: Constraints(roll=Constraints()),
                lambda: Constraints.as_in(np.ones((1, 1, D))), lambda: Constraints.as_in(np.zeros((3, D)))):
        with pytest.raises(ValueError):
            bad()


def test_resolve_returns_none_a_roll_or_itself():
    N, T = 2, 3
    roll = np.full((N, T, D), FREE, np.uint8)
    roll[0, 1, 4] = 1
    assert EG.clamp_roll(Constraints(), N, T, D, CPU) is None
    r = EG.clamp_roll(Constraints(roll), N, T, D, CPU)
    assert isinstance(r, torch.Tensor) and torch.equal(r, EG.clamp_roll(roll, N, T, D, CPU))
    c = EG.clamp_roll(Constraints.between(3, 4, roll=roll), N, T, D, CPU)
    assert isinstance(c, Constraints) and c.voices.dtype == torch.uint8 and tuple(c.voices.shape) == (N, T, 2)
    assert bool((c.voices == torch.tensor([3, 4], dtype=torch.uint8)).all()) and c.voices.is_contiguous()
    assert torch.equal(c.roll, r) and EG.clamp_parts(c) == (c.roll, c.voices)
    assert EG.clamp_roll(c, N, T, D, CPU) is c                   # a resolved one passes through a second check
    assert EG.clamp_parts(r) == (r, None) and EG.clamp_parts(None) == (None, None)
    v = _pairs(N, T, 0, 255)
    v[1, 2] = (2, 2)
    c = Constraints(None, torch.from_numpy(v)).resolve(N, T, D, CPU)
    assert c.roll is None and np.array_equal(c.voices.numpy(), v)
    part = c[1:2]                                                # sequences, as the filter's chunks take them
    assert part._key is not None and tuple(part.voices.shape) == (1, T, 2) and part.voices.is_contiguous()
    assert EG.clamp_roll(part, 1, T, D, CPU) is part
    sl = Constraints(roll, v)[:, 1:3]                            # frames, as a Stream's chunks take them
    assert sl.roll.shape == (N, 2, D) and sl.voices.shape == (N, 2, 2) and sl._key is None
    assert Constraints.exactly(2, roll=roll)[:, 1:3].voices == (2, 2)
    rep = Constraints(roll, v).repeat_rows(3)
    assert rep.roll.shape == (3 * N, T, D) and np.array_equal(rep.voices[3], v[1]) and np.array_equal(rep.voices[2], v[0])


def test_shape_dtype_and_pair_refusals():
    N, T = 2, 3
    for voices, match in ((_pairs(N + 1, T, 1, 1), "voices must have shape"), (_pairs(N, T, 1, 1).astype(np.int32), "uint8"),
                          (torch.zeros(N, T, 2), "uint8"), (_pairs(N, T, 5, 3), "a pair is"), (_pairs(N, T, 0, 16), "a pair is"),
                          (_pairs(N, T, 1, 255), "a pair is")):
        with pytest.raises(ValueError, match=match):
            Constraints(None, voices).resolve(N, T, D, CPU)
    with pytest.raises(ValueError, match="D <= 128"):
        Constraints.exactly(1).resolve(N, T, 129, CPU)
    with pytest.raises(ValueError, match="clamp must have shape"):
        Constraints.exactly(1, roll=np.zeros((N, T + 1, D), np.uint8)).resolve(N, T, D, CPU)


def test_infeasible_frames_are_refused_with_their_place():
    N, T = 3, 4
    roll = np.full((N, T, D), FREE, np.uint8)
    roll[2, 1, :5] = 1
    with pytest.raises(ValueError, match=r"frame 1 of sequence 2 is infeasible: the roll forces 5 notes on, more than hi = 4"):
        Constraints.between(0, 4, roll=roll).resolve(N, T, D, CPU)
    assert isinstance(Constraints.between(0, 5, roll=roll).resolve(N, T, D, CPU), Constraints)
    tight = np.zeros((N, T, D), np.uint8)
    tight[:, :, :2] = FREE
    tight[1, 3, 7] = 1
    with pytest.raises(ValueError, match=r"frame 0 of sequence 0 is infeasible: 0 notes forced on and 2 free are fewer than lo = 3"):
        Constraints.between(3, 4, roll=tight).resolve(N, T, D, CPU)
    v = _pairs(N, T, 0, 255)                                     # free frames are never infeasible
    v[1, 3] = (3, 3)
    assert isinstance(Constraints(tight, v).resolve(N, T, D, CPU), Constraints)
    v[1, 2] = (3, 3)
    with pytest.raises(ValueError, match="frame 2 of sequence 1"):
        Constraints(tight, v).resolve(N, T, D, CPU)
    with pytest.raises(ValueError, match="particle sampling needs"):
        EG.smc_args(Constraints(), 4, 0.5, 1, N, T, D, CPU)
    assert isinstance(EG.smc_args(Constraints.exactly(2), 4, 0.5, 1, N, T, D, CPU), Constraints)


def test_harmonize_voices_argument():
    src = np.zeros((1, 2, D))
    src[0, 0, [30, 40, 50]] = 1
    src[0, 1, [35, 45]] = 1
    roll = voice_constraints(src, 'top')
    assert voice_counts(4, src, roll).voices == (4, 4) and voice_counts((3, 4), src, roll).voices == (3, 4)
    c = voice_counts('source', src, roll)
    assert c.roll is roll and c.voices[0, :, 0].tolist() == [3, 2]
    assert isinstance(c.resolve(1, 2, D, CPU), Constraints)
    for bad in ('sauce', (1, 2, 3), 16, 2.5):
        with pytest.raises(ValueError):
            voice_counts(bad, src, roll)
    low = np.zeros((1, 1, D))
    low[0, 0, 1] = 1                                             # the kept top voice has one free note below it
    with pytest.raises(ValueError, match="infeasible"):
        voice_counts(4, low, voice_constraints(low, 'top')).resolve(1, 1, D, CPU)


# ------------------------------------------------------------------ routes, ops monkeypatched
class _Eng:
    cfg = dict(D=D, H=88, L=3, C=4, T=8, use_x_prev=True)
    device = CPU


class _Rows:
    def __init__(self, R):
        self.eng, self.R = _Eng(), R
        self.zargs, self.z, self.xhat = torch.zeros(R, 6), torch.zeros(R, 3), torch.zeros(R, D)

    def encode(self, x, w):
        pass

    def decode(self, w, z, xp, act):
        pass

    def carried(self, x_enc, x_next):
        return [x_next]


@pytest.fixture
def calls(monkeypatch):
    log = []
    for name in ('take_frame', 'philox_normal', 'philox_uniform', 'gauss_fwd', 'scale_temper', 'sigmoid_temper', 'i32_add',
                 'bernoulli_sample', 'bernoulli_sample_clamped', 'bernoulli_sample_voices', 'smc_sample', 'smc_sample_voices',
                 'smc_resample', 'smc_w_posterior', 'gather_rows'):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: log.append((_n, a)))
    return log


def _frame_calls(calls, clamp, N=2, T=3):
    del calls[:]
    w = torch.zeros(N, 4)
    chain = EG._Chain(_Rows(N), w, w, T, 0, None, 'sample', clamp=EG.clamp_roll(clamp, N, T, D, CPU), S=1)
    chain.frame()
    return chain, list(calls)


def test_a_plain_roll_and_a_voiceless_constraints_reach_the_same_calls(calls):
    N, T = 2, 3
    roll = np.full((N, T, D), FREE, np.uint8)
    roll[0, 0, 3] = 1
    names = lambda log: [n for n, _ in log]
    _, free = _frame_calls(calls, None)
    _, none = _frame_calls(calls, Constraints())
    assert names(free) == names(none) and 'bernoulli_sample' in names(free)
    ca, a = _frame_calls(calls, roll)
    cb, b = _frame_calls(calls, Constraints(roll))
    assert names(a) == names(b) and 'bernoulli_sample_clamped' in names(a) and 'bernoulli_sample_voices' not in names(a)
    draw = lambda log: [args for n, args in log if n.startswith('bernoulli_sample')][0]
    assert draw(a)[:4] == draw(b)[:4] == (N * D, D, T, 1) and torch.equal(draw(a)[6], draw(b)[6])
    cv, v = _frame_calls(calls, Constraints.between(3, 4, roll=roll))
    assert names(v) == [n if n != 'bernoulli_sample_clamped' else 'bernoulli_sample_voices' for n in names(a)]
    args = draw(v)
    assert args[:4] == (N * D, D, T, 1) and torch.equal(args[6], draw(a)[6]) and args[7] is cv.voices
    assert args[8] is cv.counter and args[9] is cv.x_next and tuple(args[7].shape) == (N, T, 2)
    _, v = _frame_calls(calls, Constraints.exactly(2))              # counts alone: the roll pointer is NULL
    assert draw(v)[6] is None and draw(v)[7] is not None


def test_the_filter_takes_the_voices_twin_only_under_voices(calls):
    G, P, T = 2, 3, 4
    roll = np.full((G, T, D), FREE, np.uint8)
    xhat, u, x = torch.zeros(G * P, D), torch.zeros(G * P, D), torch.zeros(G * P, D)
    counter = torch.zeros(1, dtype=torch.int32)
    for clamp, want in ((roll, 'smc_sample'), (Constraints(roll), 'smc_sample'),
                        (Constraints.exactly(4, roll=roll), 'smc_sample_voices'), (Constraints.exactly(4), 'smc_sample_voices')):
        del calls[:]
        smc = EG._Smc(G, P, T, 1, D, 0.5, 0, 0, EG.smc_args(clamp, P, 0.5, 1, G, T, D, CPU), CPU)
        smc.step(xhat, u, counter, x, lambda *a: calls.append(('gather', a)))
        assert [n for n, _ in calls] == [want, 'smc_resample', 'gather']
        args = calls[0][1]
        assert args[:5] == (G * P, D, P, T, 1)
        if want == 'smc_sample_voices':
            assert args[8] is smc.voices and tuple(args[8].shape) == (G, T, 2) and args[9] is counter
            assert (args[7] is None) == (clamp.roll is None)


def test_voices_take_the_chain_where_a_roll_takes_the_persistent_kernel(monkeypatch):
    made, ran = [], []

    class Chain:
        def __init__(self, rows, *a, **kw):
            made.append(kw.get('clamp'))

        def run(self, *a, **kw):
            pass

        x_enc = x_dec = torch.zeros(2, D)

    monkeypatch.setattr(EG, '_Chain', Chain)
    monkeypatch.setattr(EG.VrnnGenerate, '_persistent_ok', lambda self: True)
    monkeypatch.setattr(EG.VrnnGenerate, '_weights', lambda self, encoder=True: ())
    monkeypatch.setattr(EG.VrnnGenerate, 'ROWS', staticmethod(lambda eng, R: None))
    monkeypatch.setattr(EG, '_VrnnRows', lambda eng, R: None)
    for name in ('_vary_op', '_decode_op'):
        monkeypatch.setattr(EG.VrnnGenerate, name, staticmethod(lambda *a, _n=name, **kw: ran.append((_n, kw.get('clamp')))))
    monkeypatch.setattr(ops, 'vrnn_generate', lambda *a, **kw: ran.append(('generate', kw.get('clamp'))))
    eng = EG.VrnnGenerate()
    eng.cfg, eng.device, eng.gate_act = _Eng.cfg, CPU, 0
    N, T = 2, 3
    roll = np.full((N, T, D), FREE, np.uint8)
    src, w, z = torch.zeros(N, T, D), torch.zeros(N, 4), torch.zeros(N, T, 3)
    x_seed = torch.zeros(N, 1, D)
    for clamp in (roll, Constraints(roll)):
        eng.vary(src, w, clamp=clamp)
        eng.decode_latents(z, w, clamp=clamp)
        eng.generate(x_seed, w, T, clamp=clamp)
    assert not made and [n for n, _ in ran] == ['_vary_op', '_decode_op', 'generate'] * 2
    assert all(isinstance(c, torch.Tensor) and torch.equal(c, ran[0][1]) for _, c in ran)
    del ran[:]
    con = Constraints.between(3, 4, roll=roll)
    eng.vary(src, w, clamp=con, persistent=True)
    eng.decode_latents(z, w, clamp=con, persistent=True)
    eng.generate(x_seed, w, T, clamp=con, persistent=True)
    assert not ran and len(made) == 3 and all(isinstance(c, Constraints) and c.voices is not None for c in made)


# ------------------------------------------------------------------ the flag
def test_voices_flag_rules():
    from clvae_amd.cl_vae import sample as vs
    from clvae_amd.cl_vrnn import sample as rs
    assert [f.names for f in cli.VOICES_FLAGS] == [('--voices',)]
    assert cli.parse_voices('4') == (4, 4) and cli.parse_voices('3:4') == (3, 4) and cli.parse_voices('0:15') == (0, 15)
    for bad in ('x', '4:', ':4', '5:3', '16', '-1', '3:4:5', '2.5'):
        with pytest.raises(ValueError):
            cli.parse_voices(bad)
    for tool, mod in (('cl_vae.sample', vs), ('cl_vrnn.sample', rs)):
        assert '--voices' not in {s for a in mod.build_parser()._actions for s in a.option_strings}
        p = cli.parser_for(tool, cli.DEVICE_LOOP_FLAGS + cli.HARMONIZE_FLAGS + cli.VOICES_FLAGS)
        a = p.parse_args(['r', '--harmonize', 'top', '--voices', '4'])
        assert a.voices == '4' and cli.voices_kwargs(a) == (4, 4) and not a.device_loop
        assert cli.voices_kwargs(p.parse_args(['r', '--voices', '3:4'])) == (3, 4)
        assert cli.voices_kwargs(p.parse_args(['r'])) is None
        assert cli.voices_kwargs(mod.build_parser().parse_args(['r'])) is None
        for argv in (['r', '--voices', '5:3'], ['r', '--voices', 'many'], ['r', '--voices', '16'],
                     ['r', '--voices', '4', '--host_loop']):
            with pytest.raises(SystemExit):
                p.parse_args(argv)
        assert mod.count_clamp(p.parse_args(['r'])) == {}
        assert mod.count_clamp(p.parse_args(['r', '--voices', '2:3']))['clamp'].voices == (2, 3)
    assert vs.on_device(cli.parser_for('cl_vae.sample', cli.VOICES_FLAGS).parse_args(['r', '--voices', '4']))
    assert not vs.on_device(cli.parser_for('cl_vae.sample', cli.VOICES_FLAGS).parse_args(['r']))


# ------------------------------------------------------------------ bindings and refusals on host pointers
def test_bindings_and_einval():
    sig = _lib.SIGNATURES
    assert sig['clv_bernoulli_sample_voices'] == (ctypes.c_int, [ctypes.c_int64] + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 8)
    assert sig['clv_smc_sample_voices'] == (ctypes.c_int, [ctypes.c_int] * 5 + [ctypes.c_void_p] * 10)
    L = _lib.lib()
    p = 1 << 20                     # looks like device memory; a refused call never dereferences it
    EINVAL = -1
    ok_b = [4 * D, D, 2, 0, p, p, None, p, p, p, None, None]
    ok_s = [4, D, 2, 2, 0, p, p, None, p, p, p, p, p, None, None]

    def changed(args, **at):
        a = list(args)
        for i, v in at.items():
            a[int(i[1:])] = v
        return a
    for a in (changed(ok_b, _0=0), changed(ok_b, _0=4 * D + 1), changed(ok_b, _1=0), changed(ok_b, _0=4 * 129, _1=129),
              changed(ok_b, _2=0), changed(ok_b, _3=-1), changed(ok_b, _4=None), changed(ok_b, _5=None),
              changed(ok_b, _7=None), changed(ok_b, _8=None), changed(ok_b, _9=None),
              changed(ok_b, _0=(2 ** 31) * 2, _1=2)):
        assert L.clv_bernoulli_sample_voices(*a) == EINVAL, a
    for a in (changed(ok_s, _0=0), changed(ok_s, _2=0), changed(ok_s, _2=3), changed(ok_s, _1=129), changed(ok_s, _3=0),
              changed(ok_s, _4=-1), changed(ok_s, _5=None), changed(ok_s, _6=None), changed(ok_s, _8=None),
              changed(ok_s, _9=None), changed(ok_s, _10=None), changed(ok_s, _11=None), changed(ok_s, _12=None)):
        assert L.clv_smc_sample_voices(*a) == EINVAL, a


# ------------------------------------------------------------------ what must not move
def test_the_pinned_surfaces_are_what_they_were():
    for cls in (EG.VaeGenerate, EG.VrnnGenerate):
        for name in ('generate', 'vary', 'decode_latents', 'generate_smc'):
            params = list(inspect.signature(getattr(cls, name)).parameters)
            assert 'clamp' in params and 'voices' not in params, (cls.__name__, name)
    assert _lib.ABI_VERSION == 610
    structs = {n for n in dir(_lib) if isinstance(getattr(_lib, n), type) and issubclass(getattr(_lib, n), ctypes.Structure)
               and getattr(_lib, n) is not ctypes.Structure}
    assert len(structs) == 14
    assert [f.names[0] for f in cli.DEVICE_LOOP_FLAGS] == ['--device_loop', '--host_loop', '--seed']
    assert [f.names[0] for f in cli.HARMONIZE_FLAGS] == ['--harmonize', '--particles', '--infer_key']
    assert [f.names[0] for f in cli.RESUME_FLAGS] == ['--chunk', '--modulate']
