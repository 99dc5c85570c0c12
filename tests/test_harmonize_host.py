"""CPU checks of clamped generation's host side: voice_constraints, the constraint-roll validation, the --harmonize flag
and the C ABI of the clamped entry points (header, ctypes binding, argument checks before any device work)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import clvae_amd  # noqa: E402,F401
from clvae_amd.harmonize import FREE, voice_constraints  # noqa: E402

# the roll is an argument of the two generate entry points (ABI 610: _clamped took over the base name)
NEW = ('clv_vrnn_generate', 'clv_vae_generate', 'clv_bernoulli_sample_clamped')
GONE = ('clv_vrnn_generate_clamped', 'clv_vae_generate_clamped')


def _roll(*frames):
    r = np.zeros((len(frames), 88))
    for t, notes in enumerate(frames):
        r[t, list(notes)] = 1.0
    return r


def test_voice_constraints_top_with_fence():
    c = voice_constraints(_roll([40, 52, 64], [], [7]), 'top')
    assert c.dtype == np.uint8 and c.shape == (3, 88)
    assert c[0, 64] == 1 and np.all(c[0, 65:] == 0) and np.all(c[0, :64] == FREE)
    assert np.all(c[1] == FREE)                                   # a rest is entirely free
    assert c[2, 7] == 1 and np.all(c[2, 8:] == 0) and np.all(c[2, :7] == FREE)


def test_voice_constraints_bottom_with_fence():
    c = voice_constraints(_roll([40, 52, 64], [], [87]), 'bottom')
    assert c[0, 40] == 1 and np.all(c[0, :40] == 0) and np.all(c[0, 41:] == FREE)
    assert np.all(c[1] == FREE)
    assert c[2, 87] == 1 and np.all(c[2, :87] == 0)


@pytest.mark.parametrize('voice,note', [('top', 64), ('bottom', 40)])
def test_voice_constraints_without_fence(voice, note):
    c = voice_constraints(_roll([40, 52, 64], [0]), voice, fence=False)
    assert c[0, note] == 1 and (c[0] != FREE).sum() == 1
    assert c[1, 0] == 1 and (c[1] != FREE).sum() == 1


def test_voice_constraints_extreme_notes_and_batch_shape():
    r = np.zeros((2, 4, 88))
    r[0, 0, 87] = r[1, 3, 0] = 1
    top, bot = voice_constraints(r, 'top'), voice_constraints(r, 'bottom')
    assert top.shape == (2, 4, 88)
    assert top[0, 0, 87] == 1 and np.all(top[0, 0, :87] == FREE)
    assert bot[1, 3, 0] == 1 and np.all(bot[1, 3, 1:] == FREE)
    assert np.all(top[0, 1:] == FREE) and np.all(top[1, :3] == FREE)
    with pytest.raises(ValueError):
        voice_constraints(r, 'middle')


def test_clamp_roll_validation():
    torch = pytest.importorskip("torch")
    from clvae_amd.engine_generate import clamp_roll
    cpu = torch.device('cpu')
    good = np.full((2, 3, 88), FREE, np.uint8)
    assert clamp_roll(None, 2, 3, 88, cpu) is None
    out = clamp_roll(good, 2, 3, 88, cpu)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 3, 88) and out.is_contiguous()
    assert torch.equal(clamp_roll(torch.from_numpy(good), 2, 3, 88, cpu), out)
    for bad in (good.astype(np.float32), good.astype(np.int64), good.astype(bool), torch.zeros(2, 3, 88)):
        with pytest.raises(ValueError):
            clamp_roll(bad, 2, 3, 88, cpu)
    for shape in ((2, 4, 88), (3, 3, 88), (2, 3, 87), (2, 3 * 88)):
        with pytest.raises(ValueError):
            clamp_roll(np.zeros(shape, np.uint8), 2, 3, 88, cpu)


@pytest.mark.parametrize('tool', ['cl_vae.sample', 'cl_vrnn.sample'])
def test_harmonize_flag_parsing(tool):
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, HARMONIZE_FLAGS, parser_for
    p = parser_for(tool, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS)
    assert p.parse_args(['r']).harmonize is None
    assert p.parse_args(['r', '--harmonize', 'top']).harmonize == 'top'
    assert p.parse_args(['r', '--harmonize', 'bottom', '--seed', '3']).harmonize == 'bottom'
    with pytest.raises(SystemExit):
        p.parse_args(['r', '--harmonize', 'alto'])


@pytest.mark.parametrize('tool', ['cl_vae.sample', 'cl_vrnn.sample'])
def test_device_loop_parser_is_unchanged(tool):
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, parser_for
    a = parser_for(tool, DEVICE_LOOP_FLAGS).parse_args(['r', '--device_loop'])
    assert not hasattr(a, 'harmonize')
    dests = sorted(x.dest for x in parser_for(tool, DEVICE_LOOP_FLAGS)._actions)
    assert 'harmonize' not in dests and {'device_loop', 'host_loop', 'seed'} <= set(dests)


def test_sample_tools_decide_the_route_without_the_flag():
    import argparse
    from clvae_amd.cl_vae.sample import on_device, voice_of
    a = argparse.Namespace(device_loop=False, host_loop=False)
    assert voice_of(a) is None and not on_device(a)
    assert on_device(argparse.Namespace(device_loop=False, host_loop=False, harmonize='top'))


def test_clamped_entry_points_are_declared_and_bound():
    from clvae_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'clvae.h')).read()
    for n in NEW:
        assert re.search(r'\bint %s\(' % n, hdr), n
        assert n in _lib.SIGNATURES, n
    for n in GONE:
        assert n not in hdr and n not in _lib.SIGNATURES, n
    C = _lib.C
    for n, n_args, at in (('clv_vrnn_generate', 35, 25), ('clv_vae_generate', 29, 19)):      # the roll follows the weights
        params = [a.strip() for a in re.search(r'\bint %s\(([^;]*?)\);' % n, hdr, re.S).group(1).split(',')]
        assert len(params) == len(_lib.SIGNATURES[n][1]) == n_args and params[at] == 'const uint8_t* clamp', n
        assert _lib.SIGNATURES[n][1][at] is C.c_void_p, n
    assert 'FREE = 255' in hdr and 'BRIDGE RULE' in hdr
    assert _lib.ABI_VERSION == 610


def test_clamped_entry_points_refuse_null_and_zero_arguments():
    """Every new entry point answers CLV_EINVAL before it touches the device when a roll has no frame to constrain, its step
    counter is missing, or a size is zero, even with all other arguments valid-looking.  (A generate call without a roll is
    the plain call since ABI 610, and accepted: tests/test_sampling_refusals.py.)"""
    import ctypes as C
    from clvae_amd import _lib
    L = _lib.lib()
    tail = [0, 1.0, 1.0, 0, None, None]                # tempered, the two factors, t0, no states
    einval = L.clv_vrnn_generate(*([0] * 9 + [0] + [None] * 16 + tail + [None] * 3))
    assert einval < 0
    dummy = (C.c_float * 64)()
    p = C.cast(dummy, C.c_void_p)
    # a supported shape with every pointer set, the roll too, and no frame for it to constrain
    assert L.clv_vrnn_generate(1, 0, 0, 88, 88, 2, 10, 0, 0, 0, *([p] * 15), p, *tail, p, None, None) == einval
    assert L.clv_vrnn_generate(1, 1, 0, 88, 88, 2, 10, 0, 0, 0, *([p] * 15), p, *tail, p, None, None) == einval
    assert L.clv_vae_generate(1, 0, 88, 88, 2, 10, 1, 0, 0, *([p] * 10), p, *tail, p, None, None) == einval
    args = [88, 88, 1, 0, p, p, p, p, p, None]         # (never called as it is: every variant below has one bad argument)
    for i, bad in ((0, 0), (1, 0), (2, 0), (3, -1), (0, 87), (4, None), (5, None), (6, None), (7, None), (8, None)):
        a = list(args)
        a[i] = bad
        assert L.clv_bernoulli_sample_clamped(*a) == einval, i
