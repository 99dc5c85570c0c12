"""Host side of latent paths in and out, no GPU: the five declarations and bindings, every refused
argument of the decoding and of morph(), and the sample tools' --morph flag and its rules."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import clvae_amd  # noqa: F401
from clvae_amd import _lib, cli, morph as MO, ops
from clvae_amd.engine_generate import (VaeGenerate, VrnnGenerate, decode_args, decode_latents_numpy, decode_temper,
                                       encode_latents_numpy)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 88

ENTRY_POINTS = (('clv_vrnn_vary', 33), ('clv_vae_vary', 28), ('clv_vrnn_decode', 25), ('clv_vae_decode', 22),
                ('clv_lerp_rows', 9))


def test_declarations_and_bindings():
    hdr = open(os.path.join(ROOT, 'include', 'clvae.h')).read()
    C = _lib.C
    for name, n_args in ENTRY_POINTS:
        m = re.search(r'\bint %s\(([^;]*?)\);' % name, hdr, re.S)
        assert m, name
        assert len(m.group(1).split(',')) == n_args, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
    for name in ('clv_vrnn_vary', 'clv_vae_vary'):                 # zout sits between xhat and the stream
        params = [p.strip() for p in re.search(r'\bint %s\(([^;]*?)\);' % name, hdr, re.S).group(1).split(',')]
        assert params[-4:] == ['float* Xs', 'float* xhat', 'float* zout', 'void* stream'], name
        assert _lib.SIGNATURES[name][1][-4:] == [C.c_void_p] * 4 and _lib.SIGNATURES[name][1][-5] is C.c_float, name
    for gone in ('clv_vrnn_vary_latents', 'clv_vae_vary_latents'):        # ABI 610: they took over clv_*_vary
        assert gone not in _lib.SIGNATURES and gone not in hdr, gone
    for name in ('clv_vrnn_decode', 'clv_vae_decode'):             # one temperature (the notes') ahead of Xs, xhat, stream
        at = _lib.SIGNATURES[name][1]
        assert at[7] is C.c_uint64 and at[-4] is C.c_float and at.count(C.c_float) == 1
        assert all(a is C.c_void_p for a in at[-3:])
    assert _lib.SIGNATURES['clv_lerp_rows'][1][:2] == [C.c_int64, C.c_int64]
    assert _lib.ABI_VERSION == 610
    assert re.search(r'#define CLV_ABI_VERSION 610\b', hdr)
    for f in (ops.vrnn_vary, ops.vae_vary, ops.vrnn_decode, ops.vae_decode, ops.lerp_rows):
        assert callable(f)
    assert all(inspect.signature(f).parameters['zout'].default is None for f in (ops.vrnn_vary, ops.vae_vary))
    assert not hasattr(ops, 'vrnn_vary_latents') and not hasattr(ops, 'vae_vary_latents')
    # the C side documents the contract it cannot check from a host pointer
    doc = hdr[hdr.index('latent paths in and out'):hdr.index('int clv_lerp_rows')]
    assert "caller's contract" in doc and 'noise_rows' in doc


def test_host_refusals_of_the_library():
    """what the entry points refuse before they touch a device: NULL pointers and sizes below 1 (no GPU is needed: the
    checks come first)"""
    lib = _lib.lib()
    one = np.ones(4, np.float32)
    p = one.ctypes.data
    i32 = np.zeros(4, np.int32).ctypes.data
    assert lib.clv_lerp_rows(0, 4, p, i32, p, i32, p, p, None) == -1
    assert lib.clv_lerp_rows(1, 0, p, i32, p, i32, p, p, None) == -1
    for k in range(6):
        a = [p, i32, p, i32, p, p]
        a[k] = None
        assert lib.clv_lerp_rows(1, 4, *a, None) == -1, k
    W = [p] * 7                                                # Kx_dec .. bo
    ok = dict(N=1, T=1, z=p, w=p, Xs=p, inv_T=1.0)

    def vrnn(N, T, z, w, Xs, inv_T, L=2):
        return lib.clv_vrnn_decode(N, T, D, 88, L, 4, 0, 1, z, None, None, w, None, *W, None, inv_T, Xs, None, None)

    def vae(N, T, z, w, Xs, inv_T, L=2):
        return lib.clv_vae_decode(N, T, D, 88, L, 4, 1, 1, z, None, None, w, None, p, p, p, p, None, inv_T, Xs, None, None)
    for call in (vrnn, vae):
        for bad in (dict(N=0), dict(T=0), dict(N=-2), dict(z=None), dict(w=None), dict(Xs=None), dict(inv_T=0.0),
                    dict(inv_T=-1.0), dict(inv_T=float('nan')), dict(inv_T=float('inf')), dict(L=0), dict(L=33),
                    dict(N=2 ** 20, T=2 ** 11, L=2),             # N*T*L = 2^32
                    dict(N=2 ** 16, T=2 ** 10, L=1)):            # N*T*D = 88 * 2^26 >= 2^32
            assert call(**dict(ok, **bad)) == -1, (call.__name__, bad)
    # with a zout clv_*_vary refuse what they refuse without one (here: no sources), and N*T*L >= 2^32
    assert lib.clv_vrnn_vary(1, 1, D, 88, 2, 4, 0, 0, 1, None, None, p, p, *([p] * 13), None, 1.0, 1.0, p, None, p,
                             None) == -1
    assert lib.clv_vae_vary(1, 1, D, 88, 2, 4, 1, 0, 1, None, None, p, p, *([p] * 8), None, 1.0, 1.0, p, None, p,
                            None) == -1
    assert lib.clv_vrnn_vary(2 ** 20, 2 ** 11, D, 88, 2, 4, 0, 0, 1, p, None, p, p, *([p] * 13), None, 1.0, 1.0, p,
                             None, p, None) == -1
    assert lib.clv_vae_vary(2 ** 20, 2 ** 11, D, 88, 2, 4, 1, 0, 1, p, None, p, p, *([p] * 8), None, 1.0, 1.0, p, None,
                            p, None) == -1


def test_signatures_of_the_python_layers():
    from clvae_amd.cl_vae import model as MV
    from clvae_amd.cl_vrnn import model as MR
    for M in (MV, MR):
        sig = inspect.signature(M.encode_latents_device).parameters
        assert list(sig) == ['model', 'sources', 'w_enc', 'seed', 'z_temperature']
        assert sig['seed'].default == 0 and sig['z_temperature'].default == 1.0
        sig = inspect.signature(M.decode_latents_device).parameters
        assert list(sig) == ['model', 'z', 'w_dec', 'x0', 'history', 'seed', 'clamp', 'temperature', 'noise_rows', 'return_xhat']
        assert sig['x0'].default is None and sig['history'].default == 'own' and sig['noise_rows'].default is None
        assert 'z_temperature' not in sig and 'z_prior' not in sig          # the path is given
        assert inspect.signature(M.vary_samples_device).parameters['return_latents'].default is False
    for f in (VrnnGenerate.decode_latents, VaeGenerate.decode_latents):
        sig = inspect.signature(f).parameters
        assert sig['persistent'].default is True and sig['use_graph'].default is True and sig['history'].default == 'own'
    for f in (VrnnGenerate.vary, VaeGenerate.vary):
        assert inspect.signature(f).parameters['zout'].default is None
    sig = inspect.signature(MO.morph).parameters
    assert list(sig) == ['model', 'a', 'b', 'steps', 'w_a', 'w_b', 'z_temperature', 'common_noise', 'seed', 'temperature',
                         'clamp']
    assert sig['steps'].default == 8 and sig['z_temperature'].default == 0.0 and sig['common_noise'].default is True
    assert 'variance' in MO.morph.__doc__                                  # why the means are mixed by default


def _args(N=2, T=3, L=2, C=4, **over):
    kw = dict(z=np.zeros((N, T, L)), w_dec=np.eye(C)[np.zeros(N, int)], x0=None, history='own', clamp=None, noise_rows=None)
    kw.update(over)
    return kw


def test_decode_args_accepts_and_normalises():
    z, w, x0, hist, clamp, nr = decode_args(D=D, L=2, C=4, device='cpu', **_args())
    assert z.dtype == torch.float32 and tuple(z.shape) == (2, 3, 2) and x0 is None and hist is None and clamp is None
    assert nr is None
    roll = np.full((2, 3, D), 255, np.uint8)
    out = decode_args(D=D, L=2, C=4, device='cpu', **_args(x0=np.ones((2, D)), history=np.zeros((2, 3, D)), clamp=roll,
                                                           noise_rows=[5, 0]))
    assert tuple(out[2].shape) == (2, D) and tuple(out[3].shape) == (2, 3, D) and out[4].dtype == torch.uint8
    assert out[5].dtype == torch.int32 and out[5].tolist() == [5, 0]
    out = decode_args(D=D, L=2, C=4, device='cpu', **_args(z=torch.zeros(2, 3, 2, dtype=torch.float64),
                                                           noise_rows=torch.tensor([1, 1])))
    assert out[0].dtype == torch.float32 and out[5].tolist() == [1, 1]
    assert decode_temper(1.0) == 1.0 and decode_temper(0.5) == 2.0


@pytest.mark.parametrize("bad", [
    dict(z=None), dict(w_dec=None), dict(z=np.zeros((2, 3))), dict(z=np.zeros((2, 3, 3))), dict(z=np.zeros((2, 0, 2))),
    dict(z=np.zeros((0, 3, 2))), dict(z=np.zeros((2, 3, 2, 1))),
    dict(w_dec=np.eye(4)[[0]]), dict(w_dec=np.eye(5)[[0, 1]]), dict(w_dec=np.zeros(4)),
    dict(x0=np.zeros(D)), dict(x0=np.zeros((3, D))), dict(x0=np.zeros((2, 87))),
    dict(history='source'), dict(history=None), dict(history=np.zeros((2, 2, D))), dict(history=np.zeros((2, 3, 87))),
    dict(history=np.zeros((3, D))),
    dict(clamp=np.zeros((2, 3, D))), dict(clamp=np.zeros((2, 2, D), np.uint8)),
    dict(noise_rows=[0, -1]), dict(noise_rows=[0]), dict(noise_rows=[0, 1, 2]), dict(noise_rows=[0.0, 1.0]),
    dict(noise_rows=[True, False]), dict(noise_rows=[0, 2 ** 31]), dict(noise_rows=np.zeros((2, 1), int)),
], ids=lambda b: ','.join('%s=%s' % (k, getattr(v, 'shape', v)) for k, v in b.items()))
def test_decode_args_refuses(bad):
    with pytest.raises(ValueError):
        decode_args(D=D, L=2, C=4, device='cpu', **_args(**bad))


class _Engine:
    """an engine that must not be reached: the arguments are checked first"""
    cfg = dict(D=D, C=4, L=2, H=88, T=8, use_x_prev=True)
    device = 'cpu'

    def vary(self, *a, **kw):
        raise AssertionError("the arguments are checked first")

    decode_latents = vary


class _Model:
    engine = _Engine()


@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_public_calls_refuse_with_value_errors(which):
    M = importlib.import_module('clvae_amd.%s.model' % which)
    z, w = np.zeros((2, 3, 2)), np.eye(4)[[0, 1]]
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=True), dict(temperature=float('nan')),
               dict(temperature=1e46), dict(history='source'), dict(x0=np.zeros((1, D))), dict(clamp=np.zeros((2, 3, D))),
               dict(noise_rows=[0, -3]), dict(noise_rows=[1])):
        with pytest.raises(ValueError):
            M.decode_latents_device(_Model(), z, w, **kw)
    with pytest.raises(ValueError):
        M.decode_latents_device(_Model(), np.zeros((2, 3, 5)), w)           # the last dimension is not L
    with pytest.raises(ValueError):
        decode_latents_numpy(_Engine(), z, w, temperature=np.bool_(True))
    with pytest.raises(TypeError):
        M.decode_latents_device(_Model(), z, w, z_temperature=0.5)          # the path is given: no latent temperature
    with pytest.raises(AssertionError):                                 # and a good call does get through to the engine
        M.decode_latents_device(_Model(), z, w, x0=np.zeros((2, D)), history=np.zeros((2, 3, D)), temperature=0.5,
                                noise_rows=[4, 4])
    src = np.zeros((2, 3, D))
    for kw in (dict(z_temperature=-0.5), dict(z_temperature=False), dict(z_temperature=float('inf'))):
        with pytest.raises(ValueError):
            M.encode_latents_device(_Model(), src, w, **kw)
    with pytest.raises(ValueError):
        M.encode_latents_device(_Model(), src[0], w)
    with pytest.raises(ValueError):
        encode_latents_numpy(_Engine(), src, None)
    with pytest.raises(AssertionError):
        M.encode_latents_device(_Model(), src, w, seed=3, z_temperature=0.0)


def test_morph_refuses_with_value_errors(monkeypatch):
    a, b, w = np.zeros((2, 9, D)), np.zeros((2, 9, D)), np.eye(4)[[0, 1]]
    ok = dict(w_a=w, w_b=w)
    for bad in (dict(b=np.zeros((2, 8, D))), dict(b=np.zeros((3, 9, D))), dict(steps=0), dict(steps=-1), dict(steps=True),
                dict(steps=2.5), dict(a=np.zeros((2, 9, 87))), dict(a=np.zeros((2, 9, D, 1))), dict(w_a=np.eye(3)[[0, 1]]),
                dict(w_b=np.eye(4)[[0]]), dict(temperature=True), dict(temperature=0.0), dict(z_temperature=-1.0),
                dict(z_temperature=False), dict(clamp=np.zeros((2, 9, D))), dict(clamp=np.zeros((1, 9, D), np.uint8))):
        kw = dict(ok, a=a, b=b)
        kw.update(bad)
        with pytest.raises(ValueError):
            MO.morph(_Model(), kw.pop('a'), kw.pop('b'), **kw)
    with pytest.raises(ValueError, match='seq_length'):                 # cl_vrnn infers a label from seq_length = 8 frames
        MO.morph(_Model(), np.zeros((1, 7, D)), np.zeros((1, 7, D)))
    with pytest.raises(ValueError):
        MO.decode(_Model(), np.zeros((2, 3, 5)), w)                     # a z whose last dimension is not L
    with pytest.raises(ValueError):
        MO.encode(_Model(), np.zeros((2, 3, 87)), w)
    with pytest.raises(AssertionError):                                 # a good call reaches the engine
        MO.decode(_Model(), np.zeros((3, 2)), w[0])
    with pytest.raises(AssertionError):
        MO.encode(_Model(), np.zeros((3, D)), w[0], z_temperature=0.0)


# ------------------------------------------------------------------------------------------------- the sample tools
@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_flag_rules(which, capsys):
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    assert [f.names[0] for f in cli.MORPH_FLAGS] == ['--morph']
    # the reference's own tables stay verbatim: the flag is this implementation's
    assert not any(f.names[0] == '--morph' for t in cli.TABLES.values() for f in t)
    assert not hasattr(S.build_parser().parse_args(['r']), 'morph')
    parser = cli.parser_for('%s.sample' % which, cli.DEVICE_LOOP_FLAGS + cli.HARMONIZE_FLAGS + cli.TEMPERATURE_FLAGS
                            + cli.VARY_FLAGS + cli.MORPH_FLAGS)
    assert parser.parse_args(['r']).morph is None
    a = parser.parse_args(['r', '--morph', '4', '--temperature', '0.8', '--infer_w'])
    assert a.morph == 4 and a.infer_w and cli.morph_kwargs(a) == dict(temperature=0.8)
    assert cli.morph_kwargs(parser.parse_args(['r', '--morph', '4', '--z_temperature', '0.5'])) == dict(temperature=1.0,
                                                                                                     z_temperature=0.5)
    for bad in (['--morph', '4', '--harmonize', 'top'], ['--morph', '4', '--vary'], ['--morph', '4', '--host_loop'],
                ['--morph', '0'], ['--morph', '-2'], ['--morph', 'x'], ['--morph']):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(['r'] + bad)
        assert e.value.code == 2
    capsys.readouterr()
    if which == 'cl_vae':           # --morph implies the device loop, as --vary does
        assert S.on_device(parser.parse_args(['r', '--morph', '2'])) and not S.on_device(parser.parse_args(['r']))
    src = open(S.__file__).read()
    assert 'MORPH_FLAGS' in src.split("if __name__ == '__main__':")[1]


# ------------------------------------------------------------------------------ cl_vae: frames are read as on / off
class _VaeHost(VaeGenerate):
    """the cl_vae sampling mixin without a device: its refusals come before its first launch"""
    cfg = dict(D=D, C=4, L=2, H=88, T=8, use_x_prev=True)
    device = 'cpu'


def test_cl_vae_decode_refuses_frames_that_are_not_binary():
    z, w = np.zeros((2, 3, 2)), np.eye(4)[[0, 1]]
    for entry in (0.5, 2.0, float('nan')):
        x0, hist = np.zeros((2, D)), np.zeros((2, 3, D))
        x0[1, 0] = entry
        hist[0, 2, 63] = entry
        for persistent in (True, False):
            with pytest.raises(ValueError, match='on/off'):
                _VaeHost().decode_latents(z, w, x0=x0, persistent=persistent)
            with pytest.raises(ValueError, match='on/off'):
                _VaeHost().decode_latents(z, w, history=hist, persistent=persistent)
