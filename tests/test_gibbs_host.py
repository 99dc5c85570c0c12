"""No GPU: particle Gibbs on the host side -- the four new entries in the header, _lib.SIGNATURES and ops, their
refusals on host pointers, the reserved Philox stream, the ValueErrors of every layer and the --sweeps flag."""
import ctypes
import inspect
import os
import re
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import clvae_amd  # noqa: F401
import gibbs_reference as GR
from clvae_amd import _lib, cli, ops, trainer
from clvae_amd import engine_generate as EG
from clvae_amd.harmonize import harmonize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('clv_smc_pin_z', 'clv_smc_pin_frame', 'clv_smc_resample_conditional', 'clv_smc_backtrack_path')
EINVAL = -1
D = 88


def test_header_signatures_and_ops_agree():
    hdr = open(os.path.join(ROOT, 'include', 'clvae.h')).read()
    protos = dict(re.findall(r"\b(clv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))
    i, p = ctypes.c_int, ctypes.c_void_p
    want = {'clv_smc_pin_z': [i] * 4 + [p] * 4,
            'clv_smc_pin_frame': [i] * 5 + [p] * 6,
            'clv_smc_resample_conditional': [i] * 4 + [ctypes.c_uint64, ctypes.c_int64, ctypes.c_double] + [p] * 9,
            'clv_smc_backtrack_path': [i] * 6 + [p] * 10}
    for name in NEW:
        assert name in protos, name
        assert _lib.SIGNATURES[name] == (i, want[name]), name
        assert len(protos[name].split(',')) == len(want[name]), name
        assert hasattr(_lib.lib(), name)
        assert callable(getattr(ops, name[len('clv_'):]))
    # the conditional resampling takes clv_smc_resample's argument list, name for name
    args = lambda n: [a.split()[-1].lstrip('*') for a in protos[n].split(',')]
    assert args('clv_smc_resample_conditional') == args('clv_smc_resample')
    assert _lib.SIGNATURES['clv_smc_resample_conditional'] == _lib.SIGNATURES['clv_smc_resample']
    assert list(inspect.signature(ops.smc_resample_conditional).parameters) == \
        list(inspect.signature(ops.smc_resample).parameters)
    assert _lib.ABI_VERSION == 610 and _lib.lib().clv_version() == 610


def _changed(args, **at):
    a = list(args)
    for k, v in at.items():
        a[int(k[1:])] = v
    return a


def test_refused_argument_lists_return_einval():
    L = _lib.lib()
    p = 1 << 20                     # looks like device memory; a refused call never dereferences it
    ok = [3, 5, 2, 6, p, p, p, None]                                        # G, P, L, T, z_ref, step_dev, z
    for a in [_changed(ok, **{'_%d' % j: 0}) for j in range(4)] + [_changed(ok, **{'_%d' % j: None}) for j in (4, 5, 6)] \
            + [_changed(ok, _0=-1), _changed(ok, _0=2 ** 20, _1=2 ** 20)]:
        assert L.clv_smc_pin_z(*a) == EINVAL, a
    ok = [3, 5, D, 4, 2, p, None, p, p, p, None]                            # G, P, D, nsteps, S, x_ref, bridge, step, x, hist
    for a in [_changed(ok, **{'_%d' % j: 0}) for j in range(4)] + [_changed(ok, **{'_%d' % j: None}) for j in (5, 7, 8, 9)] \
            + [_changed(ok, _4=-1), _changed(ok, _0=2 ** 20, _1=2 ** 20)]:
        assert L.clv_smc_pin_frame(*a) == EINVAL, a
    ok = [3, 5, 4, 2, 7, 0, 0.5] + [p] * 8 + [None]
    for a in [_changed(ok, _0=0), _changed(ok, _1=0), _changed(ok, _1=1025), _changed(ok, _2=0), _changed(ok, _3=-1),
              _changed(ok, _5=-1), _changed(ok, _6=1.5), _changed(ok, _6=-0.1), _changed(ok, _6=float('nan')),
              _changed(ok, _0=2 ** 22, _1=1024)] + [_changed(ok, **{'_%d' % j: None}) for j in range(7, 15)]:
        assert L.clv_smc_resample_conditional(*a) == EINVAL, a
    ok = [3, 5, 4, 2, D, 2] + [p] * 9 + [None]      # G, P, nsteps, S, D, L, picks, anc, hist, zhist, brows, x, z, b, renewed
    for a in [_changed(ok, **{'_%d' % j: 0}) for j in (0, 1, 2, 4, 5)] + [_changed(ok, _3=-1), _changed(ok, _10=None),
              _changed(ok, _13=None), _changed(ok, _0=2 ** 20, _1=2 ** 20)] \
            + [_changed(ok, **{'_%d' % j: None}) for j in (6, 7, 8, 9, 11, 12, 14)]:
        assert L.clv_smc_backtrack_path(*a) == EINVAL, a


def test_the_reserved_stream_and_the_seed_rule():
    assert trainer.GIBBS_STREAM == 0xFFFFFFFA == GR.GIBBS_STREAM
    streams = [trainer.IW_STREAM_W, trainer.IW_STREAM_Z, trainer.SMC_STREAM, trainer.SMC_W_STREAM, trainer.KEY_STREAM,
               trainer.GIBBS_STREAM]
    assert len(set(streams)) == 6
    src = open(os.path.join(ROOT, 'classifying-vae-lstm_amd', 'csrc', 'smc.hip')).read()
    assert re.search(r"GIBBS_STREAM\s*=\s*0xFFFFFFFAu", src)
    assert EG.GIBBS_SEED_STEP == GR.SEED_STEP == 0x9E3779B97F4A7C15
    for seed, s in ((0, 0), (5, 1), (2 ** 64 - 1, 3), (123456789, 40)):
        assert EG.gibbs_seed(seed, s) == GR.sweep_seed(seed, s) < 2 ** 64
    assert EG.gibbs_seed(9, 0) == 9


def test_the_public_surface():
    want = ['self', 'x_seed', 'w', 'nsteps', 'clamp', 'particles', 'sweeps', 'resample_threshold', 'seed', 'use_graph',
            'z_prior', 'chunk', 'temperature', 'z_temperature']
    sig = inspect.signature(EG._Generate.generate_gibbs).parameters
    assert list(sig) == want
    assert [sig[k].default for k in want[7:]] == [0.5, 0, True, False, None, 1.0, 1.0]
    assert EG.VaeGenerate.generate_gibbs is EG.VrnnGenerate.generate_gibbs is EG._Generate.generate_gibbs
    assert 'generate_gibbs' not in vars(EG.VaeGenerate) and 'generate_gibbs' not in vars(EG.VrnnGenerate)
    assert EG.GibbsResult._fields == ('Xs', 'log_evidence', 'renewed', 'z')
    assert 'unbiased' in EG.GibbsResult.__doc__ and 'unbiased' in EG._Generate.generate_gibbs.__doc__
    from clvae_amd.cl_vae import model as MV
    from clvae_amd.cl_vrnn import model as MR
    for f in (MV.generate_samples_device, MR.generate_samples_device, harmonize):
        par = inspect.signature(f).parameters
        assert par['sweeps'].default is None and par['return_renewed'].default is False
        assert list(par)[-2:] == ['sweeps', 'return_renewed']            # trailing keywords: what was there keeps its place


def test_value_errors_before_anything_runs():
    from clvae_amd.cl_vae import model as MV
    from clvae_amd.cl_vrnn import model as MR
    N, nsteps = 2, 4
    roll = np.full((N, nsteps, D), 255, np.uint8)
    w = np.eye(3)[[0, 1]]
    prior = EG.WPrior.uniform(N, 3)
    model = types.SimpleNamespace(engine=None)           # every refusal comes before the engine is touched
    for gen, seeds in ((MR.generate_samples_device, np.zeros((N, 2, D))), (MV.generate_samples_device, np.zeros((N, D)))):
        for kw, msg in ((dict(sweeps=2), 'sweeps needs particles'),
                        (dict(sweeps=2, particles=4, return_key=True), 'return_key'),
                        (dict(sweeps=0, particles=4), 'sweeps must be'),
                        (dict(sweeps=-1, particles=4), 'sweeps must be'),
                        (dict(sweeps=2.5, particles=4), 'sweeps must be'),
                        (dict(sweeps=True, particles=4), 'sweeps must be'),
                        (dict(sweeps=2, particles=4, state=object()), 'state'),
                        (dict(sweeps=2, particles=4, return_state=True), 'state'),
                        (dict(particles=4, return_renewed=True), 'return_renewed needs sweeps')):
            with pytest.raises(ValueError, match=msg):
                gen(model, seeds, nsteps, w, clamp=roll, **kw)
        with pytest.raises(ValueError, match='w_prior'):
            gen(model, seeds, nsteps, None, clamp=roll, particles=4, sweeps=2, w_prior=prior)
    src = np.zeros((N, nsteps, D))
    with pytest.raises(ValueError, match='sweeps needs particles'):
        harmonize(model, np.zeros((N, 2, D)), src, w, sweeps=2)
    with pytest.raises(ValueError, match='infer_key'):
        harmonize(model, np.zeros((N, 2, D)), src, None, particles=4, sweeps=2, infer_key='discrete')
    with pytest.raises(ValueError, match='infer_key'):
        harmonize(model, np.zeros((N, 2, D)), src, w, particles=4, sweeps=2, w_prior=prior)
    # the engine's own call: sweeps, then the filter's arguments, before any buffer is asked for
    eng = EG.VrnnGenerate()
    eng.cfg, eng.device = dict(D=D, H=D, L=2, C=3, T=8, use_x_prev=True), torch.device('cpu')
    xs, wt = torch.zeros(N, 2, D), torch.as_tensor(w, dtype=torch.float32)
    for args in ((roll, 4, 0), (roll, 4, 1.5), (roll, 4, False), (roll, 0, 2), (roll, 2000, 2), (None, 4, 2)):
        with pytest.raises(ValueError):
            eng.generate_gibbs(xs, wt, nsteps, *args)
    with pytest.raises(ValueError):
        eng.generate_gibbs(xs, wt, nsteps, roll, 4, 2, resample_threshold=1.5)
    with pytest.raises(ValueError):
        eng.generate_gibbs(xs, wt, nsteps, roll, 4, 2, temperature=0.0)
    with pytest.raises(ValueError):
        eng.generate_gibbs(xs, wt, nsteps, roll, 4, 2, chunk=0)
    assert EG.gibbs_args(3) == 3 and EG.gibbs_args(np.int64(2)) == 2


def test_gibbs_flags():
    assert [f.names[0] for f in cli.GIBBS_FLAGS] == ['--sweeps']
    assert cli.GIBBS_FLAGS[0].default is None and cli.GIBBS_FLAGS[0].kind is int
    for tool in ('cl_vae.sample', 'cl_vrnn.sample'):
        p = cli.parser_for(tool, cli.DEVICE_LOOP_FLAGS + cli.HARMONIZE_FLAGS + cli.GIBBS_FLAGS)
        ns = p.parse_args(['r', '--harmonize', 'top', '--particles', '8', '--sweeps', '3'])
        assert ns.sweeps == 3 and cli.gibbs_kwargs(ns) == dict(sweeps=3, return_renewed=True)
        ns = p.parse_args(['r', '--harmonize', 'top', '--particles', '8'])
        assert ns.sweeps is None and cli.gibbs_kwargs(ns) == {}
        for bad in (['--sweeps', '3'], ['--harmonize', 'top', '--sweeps', '3'],
                    ['--harmonize', 'top', '--particles', '8', '--sweeps', '0'],
                    ['--harmonize', 'top', '--particles', '8', '--sweeps', '2', '--infer_key', 'discrete']):
            with pytest.raises(SystemExit):
                p.parse_args(['r'] + bad)
        # a parser without the group knows no sweeps
        assert cli.gibbs_kwargs(cli.parser_for(tool, cli.HARMONIZE_FLAGS).parse_args(['r'])) == {}
    import importlib
    for which in ('cl_vae', 'cl_vrnn'):
        S = importlib.import_module('clvae_amd.%s.sample' % which)
        assert S.GIBBS_FLAGS is cli.GIBBS_FLAGS
