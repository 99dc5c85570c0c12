"""Host side of re-decoding, no GPU: the new declarations and bindings, every refused argument, the sample
tools' flags and their rules, and vary()'s handling of to_key and of sources too short to infer a label from."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import clvae_amd  # noqa: F401
from clvae_amd import _lib, cli, ops, vary as V
from clvae_amd.engine_generate import VARY_HISTORY, VaeGenerate, VrnnGenerate, vary_args, vary_samples_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 88


def test_declarations_and_bindings():
    hdr = open(os.path.join(ROOT, 'include', 'clvae.h')).read()
    C = _lib.C
    for name, n_args in (('clv_vrnn_vary', 33), ('clv_vae_vary', 28), ('clv_take_frame', 7)):
        m = re.search(r'\bint %s\(([^;]*?)\);' % name, hdr, re.S)
        assert m, name
        assert len(m.group(1).split(',')) == n_args, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == n_args, name
    for name in ('clv_vrnn_vary', 'clv_vae_vary'):               # the roll and two temperatures ahead of Xs, xhat, zout, stream
        at = _lib.SIGNATURES[name][1]
        assert at[8] is C.c_uint64 and at[-7:-4] == [C.c_void_p, C.c_float, C.c_float] and all(a is C.c_void_p for a in at[-4:])
        params = [p.strip() for p in re.search(r'\bint %s\(([^;]*?)\);' % name, hdr, re.S).group(1).split(',')]
        assert params[8] == 'uint64_t seed' and params[-7:] == ['const uint8_t* clamp', 'float inv_temperature',
            'float z_temperature', 'float* Xs', 'float* xhat', 'float* zout', 'void* stream'], name
    assert _lib.ABI_VERSION == 610
    assert re.search(r'#define CLV_ABI_VERSION 610\b', hdr)
    for f in (ops.vrnn_vary, ops.vae_vary, ops.take_frame):
        assert callable(f)
    mk = open(os.path.join(ROOT, 'classifying-vae-lstm_amd', 'csrc', 'Makefile')).read()
    assert 'generate.hip' in mk and 'vae_generate.hip' in mk        # the VR instances live in the two generation files


def test_signatures_of_the_python_layers():
    from clvae_amd.cl_vae import model as MV
    from clvae_amd.cl_vrnn import model as MR
    for f in (MV.vary_samples_device, MR.vary_samples_device):
        sig = inspect.signature(f).parameters
        assert list(sig)[:3] == ['model', 'sources', 'w_enc']
        assert sig['w_dec'].default is None and sig['x0'].default is None and sig['history'].default == 'own'
        assert sig['seed'].default == 0 and sig['clamp'].default is None and sig['return_xhat'].default is False
        assert sig['temperature'].default == 1.0 and sig['z_temperature'].default == 1.0
        assert 'z_prior' not in sig and 'use_z_prior' not in sig        # it would discard the source
    for f in (VrnnGenerate.vary, VaeGenerate.vary):
        sig = inspect.signature(f).parameters
        assert sig['persistent'].default is True and sig['use_graph'].default is True and sig['history'].default == 'own'
    assert VARY_HISTORY == ('own', 'source')


def _args(N=2, T=3, C=4, **over):
    kw = dict(sources=np.zeros((N, T, D)), w_enc=np.eye(C)[np.zeros(N, int)], w_dec=None, x0=None, history='own', clamp=None)
    kw.update(over)
    return kw


def test_vary_args_accepts_and_normalises():
    src, w_enc, w_dec, x0, clamp, hist_source = vary_args(D=D, C=4, device='cpu', **_args())
    assert src.dtype == torch.float32 and tuple(src.shape) == (2, 3, D) and w_dec is w_enc and x0 is None and clamp is None
    assert hist_source is False
    roll = np.full((2, 3, D), 255, np.uint8)
    out = vary_args(D=D, C=4, device='cpu', **_args(w_dec=np.eye(4)[[1, 2]], x0=np.ones((2, D)), history='source', clamp=roll))
    assert out[2] is not out[1] and tuple(out[3].shape) == (2, D) and out[4].dtype == torch.uint8 and out[5] is True
    out = vary_args(D=D, C=4, device='cpu', **_args(sources=torch.zeros(2, 3, D, dtype=torch.float64)))
    assert out[0].dtype == torch.float32


@pytest.mark.parametrize("bad", [
    dict(history='lagged'), dict(history=None), dict(history=True),
    dict(w_enc=None), dict(w_enc=None, w_dec=np.eye(4)[[0, 1]]),
    dict(sources=np.zeros((2, D))), dict(sources=np.zeros((2, 3, 87))), dict(sources=np.zeros((2, 0, D))),
    dict(sources=np.zeros((0, 3, D))), dict(sources=np.zeros((2, 3, D, 1))),
    dict(w_enc=np.eye(4)[[0]]), dict(w_enc=np.eye(5)[[0, 1]]), dict(w_enc=np.zeros(4)),
    dict(w_dec=np.eye(4)[[0, 1, 2]]), dict(w_dec=np.eye(3)[[0, 1]]),
    dict(x0=np.zeros(D)), dict(x0=np.zeros((3, D))), dict(x0=np.zeros((2, 87))),
    dict(clamp=np.zeros((2, 3, D))), dict(clamp=np.zeros((2, 2, D), np.uint8)), dict(clamp=np.zeros((1, 3, D), np.uint8)),
], ids=lambda b: ','.join('%s=%s' % (k, getattr(v, 'shape', v)) for k, v in b.items()))
def test_vary_args_refuses(bad):
    with pytest.raises(ValueError):
        vary_args(D=D, C=4, device='cpu', **_args(**bad))


class _Engine:
    """an engine that must not be reached: the arguments are checked first"""
    cfg = dict(D=D, C=4, L=2, H=88, T=8, use_x_prev=True)
    device = 'cpu'

    def vary(self, *a, **kw):
        raise AssertionError("the arguments are checked first")


class _Model:
    engine = _Engine()


@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_public_calls_refuse_with_value_errors(which):
    M = importlib.import_module('clvae_amd.%s.model' % which)
    src, w = np.zeros((2, 3, D)), np.eye(4)[[0, 1]]
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=True), dict(temperature=float('nan')),
               dict(temperature=1e46), dict(z_temperature=-0.5), dict(z_temperature=False), dict(z_temperature=float('inf')),
               dict(history='lagged'), dict(w_dec=np.eye(3)[[0, 1]]), dict(x0=np.zeros((1, D))),
               dict(clamp=np.zeros((2, 3, D)))):
        with pytest.raises(ValueError):
            M.vary_samples_device(_Model(), src, w, **kw)
    with pytest.raises(ValueError):
        M.vary_samples_device(_Model(), src, None, w)                    # w_dec without w_enc
    with pytest.raises(ValueError):
        M.vary_samples_device(_Model(), src[0], w)
    with pytest.raises(ValueError):
        vary_samples_numpy(_Engine(), src, w, temperature=np.bool_(True))
    with pytest.raises(AssertionError):                                 # and a good call does get through to the engine
        M.vary_samples_device(_Model(), src, w, w_dec=w[::-1], x0=np.zeros((2, D)), history='source', temperature=0.5)


# ------------------------------------------------------------------------------------------------- vary / to_key
def test_key_rows():
    key_map = {'C': 0, 'G': 2, 'a': 3}
    assert np.array_equal(V.key_rows(2, 3, 4), np.tile(np.eye(4)[2], (3, 1)))
    assert np.array_equal(V.key_rows(np.int64(0), 1, 4), np.eye(4)[[0]])
    assert np.array_equal(V.key_rows('G', 2, 4, key_map), np.tile(np.eye(4)[2], (2, 1)))
    rows = np.random.default_rng(0).dirichlet(np.ones(4), 3)
    assert np.array_equal(V.key_rows(rows, 3, 4), rows) and V.key_rows(rows, 3, 4).dtype == np.float64
    assert np.array_equal(V.key_rows(rows[0], 3, 4), np.tile(rows[0], (3, 1)))
    assert np.array_equal(V.key_rows(rows.tolist(), 3, 4), rows)
    for bad in (True, False, -1, 4, 'G', 1.5, np.zeros((2, 4)), np.zeros((3, 5)), np.zeros(3)):
        with pytest.raises(ValueError):
            V.key_rows(bad, 3, 4)
    with pytest.raises(ValueError):
        V.key_rows('H', 3, 4, key_map)
    with pytest.raises(ValueError):
        V.key_rows('a', 3, 3, key_map)                                   # the map's index is outside this model's classes


def test_vary_passes_its_labels_on_and_refuses_short_sources(monkeypatch):
    from clvae_amd.cl_vrnn import model as MR
    seen = {}

    def spy(model, sources, w_enc, w_dec=None, **kw):
        seen.update(w_enc=w_enc, w_dec=w_dec, kw=kw)
        return np.zeros_like(sources)
    monkeypatch.setattr(MR, 'vary_samples_device', spy)
    src, w = np.zeros((2, 9, D)), np.eye(4)[[0, 1]]
    V.vary(_Model(), src, w)
    assert seen['w_enc'] is w and seen['w_dec'] is None and seen['kw']['history'] == 'own'
    V.vary(_Model(), src, w, to_key=3, history='source', seed=5, temperature=0.7)
    assert np.array_equal(seen['w_dec'], np.eye(4)[[3, 3]]) and seen['kw']['history'] == 'source'
    assert seen['kw']['seed'] == 5 and seen['kw']['temperature'] == 0.7
    V.transfer_key(_Model(), src, 'G', w=w, key_map={'G': 1})
    assert np.array_equal(seen['w_dec'], np.eye(4)[[1, 1]]) and seen['w_enc'] is w
    V.transfer_key(_Model(), src, w[::-1], w=w)
    assert np.array_equal(seen['w_dec'], w[::-1])
    with pytest.raises(ValueError):
        V.transfer_key(_Model(), src, None, w=w)
    with pytest.raises(ValueError):
        V.vary(_Model(), src[0], w)
    # w=None infers the label from windows of seq_length = 8 frames: 7 frames are refused, 8 reach the w-encoder
    with pytest.raises(ValueError, match='seq_length'):
        V.vary(_Model(), np.zeros((2, 7, D)))
    monkeypatch.setattr(V, 'infer_labels', lambda model, sources: w)
    V.vary(_Model(), np.zeros((2, 8, D)), to_key=0)
    assert seen['w_enc'] is w and np.array_equal(seen['w_dec'], np.eye(4)[[0, 0]])


# ------------------------------------------------------------------------------------------------- the sample tools
@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_flag_rules(which, capsys):
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    assert [f.names[0] for f in cli.VARY_FLAGS] == ['--vary', '--to_key', '--vary_history']
    # the reference's own tables stay verbatim: the flags are this implementation's list
    assert not any(f.names[0] in ('--vary', '--to_key', '--vary_history') for t in cli.TABLES.values() for f in t)
    assert not hasattr(S.build_parser().parse_args(['r']), 'vary')
    parser = cli.parser_for('%s.sample' % which, cli.DEVICE_LOOP_FLAGS + cli.HARMONIZE_FLAGS + cli.TEMPERATURE_FLAGS
                            + cli.VARY_FLAGS)
    a = parser.parse_args(['r'])
    assert a.vary is False and a.to_key is None and a.vary_history == 'own'
    a = parser.parse_args(['r', '--vary', '--to_key', 'G', '--vary_history', 'source', '--temperature', '0.8'])
    assert a.vary and a.to_key == 'G' and a.vary_history == 'source'
    for bad in (['--vary', '--harmonize', 'top'], ['--vary', '--host_loop'], ['--to_key', 'G'], ['--vary_history', 'source'],
                ['--vary', '--vary_history', 'lagged'], ['--vary', '--harmonize', 'bottom', '--particles', '4']):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(['r'] + bad)
        assert e.value.code == 2
    capsys.readouterr()
    if which == 'cl_vae':           # --vary implies the device loop, as --harmonize does
        assert S.on_device(parser.parse_args(['r', '--vary'])) and not S.on_device(parser.parse_args(['r']))
    src = open(S.__file__).read()
    assert 'VARY_FLAGS' in src.split("if __name__ == '__main__':")[1]


# ------------------------------------------------------------------------------ cl_vae: frames are read as on / off
class _VaeHost(VaeGenerate):
    """the cl_vae sampling mixin without a device: its refusals come before its first launch"""
    cfg = dict(D=D, C=4, L=2, H=88, T=8, use_x_prev=True)
    device = 'cpu'


def test_cl_vae_vary_refuses_frames_that_are_not_binary():
    from clvae_amd.engine_generate import binary_frames
    w = np.eye(4)[[0, 1]]
    for entry in (0.5, 2.0, -1.0, float('nan')):
        src, x0 = np.zeros((2, 3, D)), np.zeros((2, D))
        src[1, 2, 64] = entry
        with pytest.raises(ValueError, match='on/off'):
            _VaeHost().vary(src, w)
        with pytest.raises(ValueError, match='on/off'):
            _VaeHost().vary(src, w, persistent=False)
        x0[0, 87] = entry
        with pytest.raises(ValueError, match='on/off'):
            _VaeHost().vary(np.zeros((2, 3, D)), w, x0=x0, history='source')
    binary_frames(sources=torch.tensor([[0.0, 1.0, 1.0]]), x0=None)              # 0 and 1 pass, an absent frame passes
