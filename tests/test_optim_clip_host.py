"""CPU: the host side of gradient clipping and learning-rate decay -- the optimizer objects, the three C entry
points' bindings and their argument checks (which answer before anything touches a device), the CLI flags."""
import ctypes as C
import math
import os
import re
import types

import pytest

from clvae_amd import _lib, cli
from clvae_amd.keras_like import OptimizerSpec
from clvae_amd.utils.weightnorm import AdamWithWeightnorm
from helpers import ROOT

EINVAL, EWORKSPACE = -1, -2
NEW = ('clv_grad_norm_workspace_bytes', 'clv_grad_norm_scale', 'clv_adam_wn_step_clipped')


def test_optimizer_objects_take_keras_clip_and_decay_arguments():
    o = OptimizerSpec(clipnorm=1.0)
    assert (o.clipnorm, o.clipvalue, o.decay) == (1.0, 0.0, 0.0) and o.name == 'adam-wn'
    a = AdamWithWeightnorm(decay=1e-4)
    assert a.decay == 1e-4 and a.name == 'adam-wn' and (a.clipnorm, a.clipvalue) == (0.0, 0.0)
    b = AdamWithWeightnorm(lr=2e-3, clipnorm=5.0, clipvalue=0.5)
    assert (b.lr, b.clipnorm, b.clipvalue, b.decay) == (2e-3, 5.0, 0.5, 0.0)
    assert OptimizerSpec(clipnorm=math.inf).clipnorm == math.inf          # report the norm, clip nothing
    for key in ('decay', 'clipnorm', 'clipvalue'):
        for bad in (-1.0, float('nan')):
            with pytest.raises(ValueError):
                OptimizerSpec(**{key: bad})
            with pytest.raises(ValueError):
                AdamWithWeightnorm(**{key: bad})
    with pytest.raises(ValueError):
        OptimizerSpec(decay=math.inf)
    r = OptimizerSpec.resolve('rmsprop', clipvalue=0.25, decay=1e-3)
    assert (r.name, r.beta_2, r.clipvalue, r.decay, r.clipnorm) == ('rmsprop', 0.9, 0.25, 1e-3, 0.0)
    assert OptimizerSpec.resolve('adam', clipnorm=2.0).clipnorm == 2.0
    assert OptimizerSpec.resolve(a) is a
    with pytest.raises(ValueError):
        OptimizerSpec.resolve(a, clipnorm=1.0)
    plain = OptimizerSpec.resolve('adam-wn')
    assert (plain.clipnorm, plain.clipvalue, plain.decay) == (0.0, 0.0, 0.0)


def test_the_three_entry_points_are_bound_and_declared():
    hdr = open(os.path.join(ROOT, "include", "clvae.h")).read()
    assert int(re.search(r"#define\s+CLV_ABI_VERSION\s+(\d+)", hdr).group(1)) == 610 == _lib.ABI_VERSION
    flat = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = dict(re.findall(r"\b(clv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", flat))
    for name in NEW:
        assert name in _lib.SIGNATURES and name in protos, name
        assert hasattr(_lib.lib(), name)
    # the 21 arguments of clv_adam_wn_step, unchanged, then grad_scale, clipvalue, decay
    base, clipped = _lib.SIGNATURES['clv_adam_wn_step'], _lib.SIGNATURES['clv_adam_wn_step_clipped']
    assert len(base[1]) == 21 and clipped[1][:21] == base[1] and clipped[1][21:] == [C.c_void_p, C.c_float, C.c_float]
    strip = lambda s: [re.sub(r"\s+", " ", a.strip()) for a in s.split(",")]
    assert strip(protos['clv_adam_wn_step_clipped'])[:21] == strip(protos['clv_adam_wn_step'])
    assert strip(protos['clv_adam_wn_step_clipped'])[21:] == ['const float* grad_scale', 'float clipvalue', 'float decay']


def _table(shapes):
    import optim_reference as R
    descs, n, n_cols = R.layout(shapes)
    return (_lib.ParamDesc * len(descs))(*[_lib.ParamDesc(d.offset, d.rows, d.cols, d.col_offset, d.is_matrix, 0) for d in descs]), len(descs)


def test_norm_workspace_is_one_float_per_plan_unit():
    L = _lib.lib()
    assert L.clv_grad_norm_workspace_bytes(None, 0) == 0
    tb, k = _table([('a/kernel', (17, 3)), ('a/bias', (3,)), ('t/kernel', (160, 8))])       # 2 + 1 + 10 units of <= 16 rows
    assert L.clv_grad_norm_workspace_bytes(tb, k) == 13 * 4 + 12
    tb, k = _table([('t/kernel', (11264, 88))])
    assert L.clv_grad_norm_workspace_bytes(tb, k) == 704 * 4


def test_refusals_answer_before_anything_is_launched():
    """every refused value, with non-NULL stand-ins for the device pointers: the checks come first, nothing dereferences them"""
    L = _lib.lib()
    tb, k = _table([('a/kernel', (16, 3)), ('t/kernel', (160, 8))])
    need = L.clv_grad_norm_workspace_bytes(tb, k)
    p = C.c_void_p(4096)
    norm = lambda clipnorm=1.0, table=tb, plan=p, grads=p, stats=p, ws=p, nbytes=need: \
        L.clv_grad_norm_scale(table, k, plan, grads, clipnorm, stats, ws, nbytes, None)
    for bad in (0.0, -1.0, float('nan'), -math.inf):
        assert norm(clipnorm=bad) == EINVAL, bad
    for null in ('table', 'plan', 'grads', 'stats', 'ws'):
        assert norm(**{null: None}) == EINVAL, null
    assert norm(nbytes=need - 1) == EINVAL and norm(nbytes=0) == EINVAL
    ws_bytes = L.clv_adam_wn_workspace_bytes(tb, k)
    known = _lib.AdamKnownSums(1, 1, p, p)

    def step(grad_scale=None, clipvalue=0.0, decay=0.0, kn=None, nbytes=ws_bytes, table=tb):
        return L.clv_adam_wn_step_clipped(table, k, p, p, p, p, p, p, p, p, p, 0, 1e-3, 0.9, 0.999, 1e-8, 1,
                                          C.byref(kn) if kn is not None else None, p, nbytes, None, grad_scale, clipvalue, decay)
    for bad in (-1.0, float('nan'), -math.inf):
        assert step(clipvalue=bad) == EINVAL, bad
    for bad in (-1.0, float('nan'), math.inf, -math.inf):
        assert step(decay=bad) == EINVAL, bad
    assert step(clipvalue=0.5, kn=known) == EINVAL                  # a clamped gradient's sum g.V is not the backward pass's
    assert step(grad_scale=p, clipvalue=0.5, decay=0.1, table=None) == EINVAL
    assert step(grad_scale=p, decay=0.1, nbytes=ws_bytes - 1) == EWORKSPACE     # as clv_adam_wn_step


def test_cli_flags_are_extras_and_reach_the_optimizer():
    from clvae_amd.cl_vae import train as vt
    from clvae_amd.cl_vrnn import train as rt
    assert [f.names[0] for f in cli.OPTIMIZER_FLAGS] == ['--clipnorm', '--clipvalue', '--lr_decay']
    for tool, mod in (('cl_vrnn.train', rt), ('cl_vae.train', vt)):
        ns = cli.parser_for(tool, cli.OPTIMIZER_FLAGS).parse_args(['r', '--clipnorm', '2.5', '--clipvalue', '0.1', '--lr_decay', '1e-4'])
        assert (ns.clipnorm, ns.clipvalue, ns.lr_decay) == (2.5, 0.1, 1e-4)
        off = cli.parser_for(tool, cli.OPTIMIZER_FLAGS).parse_args(['r'])
        assert (off.clipnorm, off.clipvalue, off.lr_decay) == (0.0, 0.0, 0.0)
        # the reference's surface is what build_parser() keeps
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(['r', '--clipnorm', '2.5'])
        src = open(mod.__file__).read()
        assert 'OPTIMIZER_FLAGS' in src.split("if __name__ == '__main__':")[1]

    def spec(**kw):
        plan = object.__new__(cli.TrainPlan)
        plan.args = types.SimpleNamespace(**kw)
        return plan.optimizer()
    o = spec(optimizer='adam-wn', clipnorm=2.5, clipvalue=0.1, lr_decay=1e-4)
    assert isinstance(o, AdamWithWeightnorm) and (o.clipnorm, o.clipvalue, o.decay, o.lr, o.epsilon) == (2.5, 0.1, 1e-4, 0.001, 1e-8)
    for name in ('adam', 'rmsprop'):
        o = spec(optimizer=name, clipnorm=0.0, clipvalue=0.0, lr_decay=0.5)
        assert isinstance(o, OptimizerSpec) and (o.name, o.decay, o.clipnorm) == (name, 0.5, 0.0)
    assert OptimizerSpec.resolve(spec(optimizer='rmsprop', clipnorm=1.0, clipvalue=0.0, lr_decay=0.0)).beta_2 == 0.9
    # without the flags (build_parser(): the reference's surface) nothing changes
    assert spec(optimizer='adam') == 'adam' and spec(optimizer='adam', clipnorm=0.0, clipvalue=0.0, lr_decay=0.0) == 'adam'
    d = spec(optimizer='adam-wn')
    assert isinstance(d, AdamWithWeightnorm) and (d.clipnorm, d.clipvalue, d.decay) == (0.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        spec(optimizer='adam', clipnorm=-1.0, clipvalue=0.0, lr_decay=0.0)
