"""Host side of the sampling temperatures, no GPU: the refused arguments, the rules between the sample
tools' flags, and the new bindings."""
import importlib
import inspect
import os
import re

import numpy as np
import pytest

pytest.importorskip("torch")

import clvae_amd  # noqa: F401
from clvae_amd import _lib, cli, ops
from clvae_amd.engine_generate import VaeGenerate, VrnnGenerate, temper_args

BAD_T = [0, 0.0, -1.0, float('nan'), float('inf'), -float('inf'), 1e-39, 1e46, True, False, np.bool_(True), None, 'x']
BAD_TZ = [-1e-9, -1.0, float('nan'), float('inf'), 1e39, True, False, None]


@pytest.mark.parametrize("T", BAD_T, ids=repr)
def test_refused_temperatures(T):
    """not finite, <= 0, a float32(1 / T) that is zero (T = 1e46) or not finite (T = 1e-39), bools"""
    with pytest.raises(ValueError):
        temper_args(T, 1.0)


@pytest.mark.parametrize("Tz", BAD_TZ, ids=repr)
def test_refused_z_temperatures(Tz):
    with pytest.raises(ValueError):
        temper_args(1.0, Tz)


def test_accepted_values_and_the_neutral_case():
    assert temper_args(1.0, 1.0) is None and temper_args(1, 1) is None and temper_args(np.float32(1), np.float64(1)) is None
    assert temper_args(0.8, 1.0) == (float(np.float32(1.0 / 0.8)), 1.0)
    assert temper_args(1.0, 0) == (1.0, 0.0)
    inv_T, Tz = temper_args(1e-3, 0.3)
    assert inv_T == float(np.float32(1000.0)) and Tz == float(np.float32(0.3))
    assert np.float32(inv_T) == inv_T and np.float32(Tz) == Tz          # already float32 values: the C call rounds nothing


def test_keyword_arguments_with_neutral_defaults():
    from clvae_amd import harmonize as HZ
    from clvae_amd.cl_vae import model as MV
    from clvae_amd.cl_vrnn import model as MR
    for f in (VrnnGenerate.generate, VrnnGenerate.generate_smc, VaeGenerate.generate, VaeGenerate.generate_smc,
              MV.generate_samples_device, MR.generate_samples_device, HZ.harmonize):
        sig = inspect.signature(f).parameters
        assert sig['temperature'].default == 1.0 and sig['z_temperature'].default == 1.0, f


def test_public_calls_refuse_before_touching_the_device():
    from clvae_amd.cl_vae import model as MV
    from clvae_amd.cl_vrnn import model as MR

    class NoEngine:
        @property
        def engine(self):
            raise AssertionError("the arguments are checked first")
    for gen, seeds in ((MR.generate_samples_device, np.zeros((1, 2, 88))), (MV.generate_samples_device, np.zeros((1, 88)))):
        with pytest.raises(ValueError):
            gen(NoEngine(), seeds, 4, np.eye(3)[[0]], temperature=0.0)
        with pytest.raises(ValueError):
            gen(NoEngine(), seeds, 4, np.eye(3)[[0]], z_temperature=-1.0)


def test_bindings():
    for name in ('clv_vrnn_generate', 'clv_vae_generate', 'clv_sigmoid_temper', 'clv_scale_temper'):
        assert name in _lib.SIGNATURES
    C = _lib.C
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'clvae.h')).read()
    # the roll, the flag and the two factors follow the weights: clamp, tempered, inv_temperature, z_temperature
    for name, n_args, at in (('clv_vrnn_generate', 35, 25), ('clv_vae_generate', 29, 19)):
        argtypes = _lib.SIGNATURES[name][1]
        assert len(argtypes) == n_args and argtypes[at:at + 4] == [C.c_void_p, C.c_int, C.c_float, C.c_float], name
        assert argtypes.count(C.c_float) == 2 and all(a is C.c_void_p for a in argtypes[at - 4:at]), name
        params = [p.strip() for p in re.search(r'\bint %s\(([^;]*?)\);' % name, hdr, re.S).group(1).split(',')]
        assert len(params) == n_args, name
        assert params[at:at + 4] == ['const uint8_t* clamp', 'int tempered', 'float inv_temperature', 'float z_temperature'], name
    for fam in ('vrnn', 'vae'):                                # ABI 610: the base name took the variants over
        for gone in ('clv_%s_generate_clamped' % fam, 'clv_%s_generate_tempered' % fam):
            assert gone not in _lib.SIGNATURES and gone not in hdr
    assert callable(ops.sigmoid_temper) and callable(ops.scale_temper)
    assert 'temper' in inspect.signature(ops.vrnn_generate).parameters and 'temper' in inspect.signature(ops.vae_generate).parameters
    assert _lib.ABI_VERSION == 610


@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_flag_rules(which, capsys):
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    parser = cli.parser_for('%s.sample' % which, cli.DEVICE_LOOP_FLAGS + cli.HARMONIZE_FLAGS + cli.TEMPERATURE_FLAGS)
    a = parser.parse_args(['r'])
    assert a.temperature == 1.0 and a.z_temperature == 1.0 and cli.temperature_kwargs(a) == {}
    a = parser.parse_args(['r', '--temperature', '0.7', '--z_temperature', '0.5'])
    assert cli.temperature_kwargs(a) == dict(temperature=0.7, z_temperature=0.5)
    for bad in (['--host_loop', '--temperature', '0.7'], ['--host_loop', '--z_temperature', '0'], ['--temperature', '0'],
                ['--temperature', '-1'], ['--temperature', 'nan'], ['--z_temperature', '-0.5'], ['--z_temperature', 'inf']):
        with pytest.raises(SystemExit) as e:
            parser.parse_args(['r'] + bad)
        assert e.value.code == 2
    capsys.readouterr()
    parser.parse_args(['r', '--host_loop', '--temperature', '1.0'])            # neutral values change nothing
    # the reference's own tables stay verbatim: the flags are this implementation's list
    assert not any(f.names[0] in ('--temperature', '--z_temperature') for t in cli.TABLES.values() for f in t)
    ns = cli.parser_for('%s.sample' % which).parse_args(['r'])
    assert cli.temperature_kwargs(ns) == {}
    if which == 'cl_vae':           # a non-default value implies the device loop, as --harmonize does
        assert S.on_device(parser.parse_args(['r', '--temperature', '0.7']))
        assert S.on_device(parser.parse_args(['r', '--z_temperature', '0.5']))
        assert not S.on_device(parser.parse_args(['r']))
