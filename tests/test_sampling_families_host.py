"""No GPU: the two sampling mixins share one body each of vary, decode_latents and generate_smc (engine_generate._Generate),
and what a family states about itself is what the kernels and the frame chains need of it."""
import inspect

import pytest

torch = pytest.importorskip("torch")

import clvae_amd  # noqa: F401
from clvae_amd import engine_generate as EG
from clvae_amd import ops
from clvae_amd.engine_generate import VaeGenerate, VrnnGenerate

SHARED = ('vary', 'decode_latents', 'generate_smc')
PUBLIC = {'generate': ['x_seed', 'w', 'nsteps', 'seed', 'use_graph', 'z_prior', 'persistent', 'xhat_out', 'clamp',
                       'temperature', 'z_temperature', 'state', 'return_state'],
          'vary': ['sources', 'w_enc', 'w_dec', 'x0', 'history', 'seed', 'clamp', 'temperature', 'z_temperature', 'persistent',
                   'use_graph', 'xhat_out', 'zout'],
          'decode_latents': ['z', 'w_dec', 'x0', 'history', 'seed', 'clamp', 'temperature', 'noise_rows', 'persistent',
                             'use_graph', 'xhat_out'],
          'generate_smc': ['x_seed', 'w', 'nsteps', 'clamp', 'particles', 'resample_threshold', 'n_out', 'seed', 'use_graph',
                           'z_prior', 'chunk', 'w_prior', 'temperature', 'z_temperature'],
          '_weights': ['encoder']}
VRNN_ONLY = {'new_state': ['B'], 'encode_w': ['X', 'B'], 'enc_step': ['x', 'w', 'st', 'rec_name'],
             'dec_step': ['z', 'xp', 'w', 'st', 'act']}


def test_the_shared_calls_are_one_function():
    for name in SHARED:
        assert getattr(VaeGenerate, name) is getattr(VrnnGenerate, name) is getattr(EG._Generate, name), name
        assert name not in vars(VaeGenerate) and name not in vars(VrnnGenerate), name


def test_both_families_resolve_every_public_method():
    for cls, names in ((VaeGenerate, PUBLIC), (VrnnGenerate, dict(PUBLIC, **VRNN_ONLY))):
        for name, params in names.items():
            assert list(inspect.signature(getattr(cls, name)).parameters) == ['self'] + params, (cls.__name__, name)


class _Numel:
    def __init__(self, n):
        self.n = n

    def numel(self):
        return self.n


def test_each_family_states_its_own_particulars(monkeypatch):
    asked = []
    monkeypatch.setattr(ops, 'vae_generate_supported', lambda *a: asked.append(('vae',) + a) or True)
    monkeypatch.setattr(ops, 'vrnn_generate_supported', lambda *a: asked.append(('vrnn',) + a) or True)
    cfg = dict(D=88, H=88, L=3, C=4, T=8, use_x_prev=True)
    vae, vrnn = VaeGenerate(), VrnnGenerate()
    vae.cfg, vae.B = cfg, 8
    vrnn.cfg, vrnn.gate_act = cfg, 7
    # the rows of a chain; the most rows of one chunk of the filter
    assert VaeGenerate.ROWS is EG._VaeRows and VrnnGenerate.ROWS is EG._VrnnRows
    assert vae._smc_cap() == 8 and vrnn._smc_cap() is None
    with pytest.raises(ValueError, match="exceed the engine's batch size"):
        EG._VaeRows(vae, 9)
    # persistent usable: the family's own predicate on (D, H, L, C); cl_vae never without its hidden layer
    assert vae._persistent_ok() is True and vrnn._persistent_ok() is True
    assert asked == [('vae', 88, 88, 3, 4), ('vrnn', 88, 88, 3, 4)]
    vae.cfg = dict(cfg, H=0)
    assert not vae._persistent_ok() and len(asked) == 2
    vae.cfg = cfg
    # the int after C in every entry
    assert vae._family_flag() is True and vrnn._family_flag() == 7
    # frames: cl_vae on / off, cl_vrnn any float
    assert VaeGenerate._check_frames is EG.binary_frames
    half = torch.full((2, 88), 0.5)
    with pytest.raises(ValueError, match="x0 has an entry other than 0 and 1"):
        vae._check_frames(sources=torch.zeros(2, 3, 88), x0=half)
    assert vrnn._check_frames(sources=half, x0=half, history=None) is None
    # 32-bit addressing of a re-decoding: cl_vae never leaves the persistent route
    big = 2 ** 32
    assert vae._vary_fits(_Numel(big), big, _Numel(3 * big)) is True
    assert vrnn._vary_fits(None, 5, None) and vrnn._vary_fits(_Numel(big - 1), big // (88 * 4), _Numel(3 * big - 1))
    assert not vrnn._vary_fits(_Numel(big), 5, None)
    assert not vrnn._vary_fits(None, big // (88 * 4) + 1, None)
    assert not vrnn._vary_fits(None, 5, _Numel(3 * big))
    # the filter's chain: S, and where the seed rows go
    xs2, xs3 = torch.zeros(4, 88), torch.zeros(4, 2, 88)
    assert EG.seed_steps('cl_vae', xs2) == 0 and EG.seed_steps('cl_vrnn', xs3) == 2
    sv = vae._smc_seed(xs2)
    assert sorted(sv) == ['dec_prev', 'x_dec', 'x_enc'] and sv['dec_prev'] == 'enc_input' and sv['x_enc'] is xs2
    assert sv['x_dec'] is not xs2 and torch.equal(sv['x_dec'], xs2)
    sr = vrnn._smc_seed(xs3)
    assert sorted(sr) == ['dec_prev', 'seed_frames'] and sr['dec_prev'] == 'shared' and sr['seed_frames'] is xs3
    # the entry points (vary stores the latents where it gets a zout) and the state layout
    assert VaeGenerate._vary_op is ops.vae_vary and VaeGenerate._decode_op is ops.vae_decode
    assert VrnnGenerate._vary_op is ops.vrnn_vary and VrnnGenerate._decode_op is ops.vrnn_decode
    assert (VaeGenerate.STATE_KIND, VrnnGenerate.STATE_KIND) == ('cl_vae', 'cl_vrnn')
    assert EG.STATE_FIELDS == {'cl_vrnn': ('h_enc', 'c_enc', 'h_dec', 'c_dec', 'x'), 'cl_vae': ('x_in', 'hist')}
    assert EG.SEED_RANK == {'cl_vrnn': 3, 'cl_vae': 2}
    assert EG.LSTM_FIELDS == {'cl_vrnn': ('h_enc', 'c_enc', 'h_dec', 'c_dec'), 'cl_vae': ()}
    assert EG.state_widths('cl_vrnn', dict(D=88, H=40)) == dict(h_enc=40, c_enc=40, h_dec=40, c_dec=40, x=88)
    assert EG.state_widths('cl_vae', dict(D=88, H=40)) == dict(x_in=88, hist=88)
