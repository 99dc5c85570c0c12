"""CPU tests of the novelty audit: the C ABI surface of clv_roll_nearest, the library's and nearest()'s
refusals, Novelty's bookkeeping on hand-built fields, and the argument surfaces of the tools."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import clvae_amd  # noqa: F401
from clvae_amd import _lib
from helpers import ROOT


def _protos():
    hdr = open(os.path.join(ROOT, "include", "clvae.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    return dict(re.findall(r"\b(clv_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr))


def test_the_entries_are_declared_bound_and_exported():
    protos = _protos()
    for name, nargs, res in (('clv_roll_nearest', 21, ctypes.c_int), ('clv_roll_nearest_workspace_bytes', 3, ctypes.c_size_t)):
        assert name in protos, name
        assert len(protos[name].split(',')) == nargs
        r, args = _lib.SIGNATURES[name]
        assert r is res and len(args) == nargs
        assert hasattr(_lib.lib(), name)
    a = _lib.SIGNATURES['clv_roll_nearest'][1]
    assert all(t is ctypes.c_int for t in a[:6]) and all(t is ctypes.c_int64 for t in a[6:9]) and a[16] is ctypes.c_size_t
    assert _lib.ABI_VERSION == 610 and _lib.lib().clv_version() == 610
    from clvae_amd import ops
    assert callable(ops.roll_nearest) and callable(ops.roll_nearest_workspace_bytes)
    src = open(os.path.join(ROOT, "classifying-vae-lstm_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bnovelty\.hip\b", src, flags=re.M)


def test_workspace_size():
    f = _lib.lib().clv_roll_nearest_workspace_bytes
    assert f(0, 0, 0) >= 0
    assert f(100, 1000, 50) >= 16 * 1100 + 4 * 1000 + 8 * 50
    assert f(101, 1000, 50) - f(100, 1000, 50) == 16 and f(100, 1000, 51) - f(100, 1000, 50) == 8
    assert f(-1, 0, 0) == 0 and f(0, 1 << 31, 0) == 0


ORDER = ('Nq', 'Nc', 'W', 'hop', 'S', 'D', 'Fq', 'Fc', 'Wq', 'q_roll', 'q_off', 'c_roll', 'c_off', 'qwin_off', 'exclude',
         'workspace', 'workspace_bytes', 'dist', 'shift', 'cframe', 'stream')


def _args(**kw):
    """a well-formed argument list (pointers: any non-NULL, 16-byte aligned value; the entry refuses before it reads them)"""
    p = ctypes.c_void_p(4096)
    a = dict(Nq=1, Nc=1, W=16, hop=1, S=2, D=88, Fq=32, Fc=64, Wq=17, q_roll=p, q_off=p, c_roll=p, c_off=p, qwin_off=p,
             exclude=p, workspace=p, workspace_bytes=1 << 20, dist=p, shift=p, cframe=p, stream=None)
    a.update(kw)
    return [a[k] for k in ORDER]


@pytest.mark.parametrize("bad", [dict(q_roll=None), dict(q_off=None), dict(c_roll=None), dict(c_off=None), dict(qwin_off=None),
                                 dict(workspace=None), dict(dist=None), dict(shift=None), dict(cframe=None),
                                 dict(D=0), dict(D=117), dict(D=-1), dict(W=0), dict(W=1025), dict(hop=0), dict(hop=-3),
                                 dict(S=-1), dict(S=13), dict(Nq=0), dict(Nc=0), dict(Nq=-1),
                                 dict(Fq=-1), dict(Fc=-1), dict(Wq=-1), dict(Fq=1 << 31), dict(Fc=1 << 31), dict(Wq=1 << 31),
                                 dict(workspace_bytes=16 * 96 + 4 * 64 + 8 * 17 - 1), dict(workspace=ctypes.c_void_p(4104))])
def test_the_entry_refuses_before_the_device(bad):
    """CLV_EINVAL (-1) on a machine without a GPU: nothing was launched"""
    assert _lib.lib().clv_roll_nearest(*_args(**bad)) == -1


def test_no_query_window_is_ok_and_launches_nothing():
    assert _lib.lib().clv_roll_nearest(*_args(Wq=0)) == 0
    assert _lib.lib().clv_roll_nearest(*_args(Wq=0, exclude=None)) == 0


# ------------------------------------------------------------------------------------------------------------ nearest()
def test_nearest_refuses_with_value_errors_before_the_device():
    """every refusal is raised from the host-side checks: no GPU is needed, and torch's device runtime stays untouched
    (keytrack.pack_pieces is reused for the packing, and its module imports torch, so torch itself is loaded)"""
    import torch
    from clvae_amd.novelty import nearest
    ok = np.zeros((20, 88))
    bad_calls = [
        dict(queries=[np.full((20, 88), 2.0)], corpus=[ok]),                         # not binary
        dict(queries=[ok], corpus=[np.full((20, 88), 0.5)]),
        dict(queries=[ok], corpus=[np.zeros((20, 87))]),                             # the widths differ
        dict(queries=[np.zeros((20, 87))], corpus=[ok]),
        dict(queries=[np.zeros((20, 117))], corpus=[np.zeros((20, 117))]),           # wider than 116
        dict(queries=np.zeros((2, 20, 120)), corpus=np.zeros((2, 20, 120))),
        dict(queries=[np.zeros(88)], corpus=[ok]),
        dict(queries=[], corpus=[ok]), dict(queries=[ok], corpus=[]),
        dict(queries=[ok], corpus=[ok], window=0), dict(queries=[ok], corpus=[ok], window=1025),
        dict(queries=[ok], corpus=[ok], window=4.0), dict(queries=[ok], corpus=[ok], window=True),
        dict(queries=[ok], corpus=[ok], hop=0), dict(queries=[ok], corpus=[ok], hop=-1), dict(queries=[ok], corpus=[ok], hop=1.5),
        dict(queries=[ok], corpus=[ok], semitones=-1), dict(queries=[ok], corpus=[ok], semitones=13),
        dict(queries=[ok], corpus=[ok], semitones=1.0),
        dict(queries=[ok], corpus=[ok], exclude=[0, 0]),                             # the wrong length
        dict(queries=[ok, ok], corpus=[ok], exclude=[0]),
        dict(queries=[ok], corpus=[ok], exclude=[1]), dict(queries=[ok], corpus=[ok], exclude=[-2]),       # out of range
        dict(queries=[ok], corpus=[ok], exclude=[0.5]),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            nearest(device='cuda:0', **kw)
    assert not torch.cuda.is_initialized()


def _nov(window, hop, dists):
    from clvae_amd.novelty import Novelty
    z = [np.zeros(len(d), np.int64) for d in dists]
    return Novelty(window, hop, 0, [max(0, (len(d) - 1) * hop + window) if len(d) else 0 for d in dists],
                   [np.asarray(d, np.int32) for d in dists], z, [np.where(np.asarray(d) < 0, -1, 3) for d in dists], z,
                   [np.arange(len(d)) * hop for d in dists], z)


def test_copied_longest_copy_and_quantiles():
    nov = _nov(4, 1, [[0, 0, 5, 0, 0, 0, 2], [3, 1, 7], [], [-1, -1], [0, -1, 0]])
    np.testing.assert_allclose(nov.copied(), [5 / 7, 0, 0, 0, 2 / 3])
    np.testing.assert_allclose(nov.copied(max_dist=2), [6 / 7, 1 / 3, 0, 0, 2 / 3])       # -1 is no copy at any bound
    assert [nov.longest_copy(n) for n in range(5)] == [3 - 1 + 4, 0, 0, 0, 4]
    assert nov.longest_copy(0, max_dist=2) == 4 - 1 + 4 and nov.longest_copy(1, max_dist=7) == 2 + 4
    np.testing.assert_allclose(nov.quantiles((0, .5, 1)), [0, 0, 7])                    # over the 12 windows with a candidate
    np.testing.assert_allclose(nov.quantiles((.75,)), [2.25])
    assert len(nov.quantiles()) == 5
    assert np.isnan(_nov(4, 1, [[-1], []]).quantiles()).all()
    hop3 = _nov(4, 3, [[0, 0, 0, 9, 0]])
    assert hop3.longest_copy(0) == 2 * 3 + 4
    with pytest.raises(ValueError):
        _nov(2, 3, [[0, 0]]).longest_copy(0)                                             # windows that do not touch
    assert nov.closest(0)[0] == 0 and nov.closest(1) == (1, 0, 3, 0, 1) and nov.closest(3) is None
    s = nov.summary(1)
    assert (s['min_dist'], s['median_dist'], s['windows'], s['longest_copy']) == (1, 3.0, 3, 0)
    assert nov.summary(3)['min_dist'] == -1 and nov.summary(3)['nearest_song'] == -1
    import json
    j = json.loads(json.dumps(nov.to_json()))
    assert j['dist'][0] == [0, 0, 5, 0, 0, 0, 2] and j['window'] == 4 and len(j['copied']) == 5 and j['song'][3] == [-1, -1]


# ----------------------------------------------------------------------------------------------------------- the tools
FLAG_LISTS = ('DEVICE_LOOP_FLAGS', 'HARMONIZE_FLAGS', 'TEMPERATURE_FLAGS', 'VARY_FLAGS', 'MORPH_FLAGS', 'RESUME_FLAGS',
              'VOICES_FLAGS', 'GIBBS_FLAGS', 'NOVELTY_FLAGS')


@pytest.mark.parametrize("tool", ['cl_vae.sample', 'cl_vrnn.sample'])
def test_parser_rules_of_the_two_flags(tool, capsys):
    from clvae_amd import cli
    p = cli.parser_for(tool, sum((getattr(cli, n) for n in FLAG_LISTS), []))
    ns = p.parse_args(['run'])
    assert ns.novelty is None and ns.novelty_transpose == 0
    ns = p.parse_args(['run', '--novelty', '8', '--novelty_transpose', '12', '--vary'])
    assert ns.novelty == 8 and ns.novelty_transpose == 12
    assert p.parse_args(['run', '--novelty', '1', '--host_loop']).novelty == 1           # a post-process: any route
    for bad in (['--novelty', '0'], ['--novelty', '-4'], ['--novelty_transpose', '3'], ['--novelty', '8', '--novelty_transpose', '13'],
                ['--novelty', '8', '--novelty_transpose', '-1'], ['--novelty', 'x']):
        with pytest.raises(SystemExit):
            p.parse_args(['run'] + bad)
    capsys.readouterr()
    # a parser without the flags is not touched by their rules
    assert not hasattr(cli.parser_for(tool).parse_args(['run']), 'novelty')
    import types
    cli.novelty_check(types.SimpleNamespace(novelty=None), 40)
    cli.novelty_check(types.SimpleNamespace(novelty=8), 88)
    with pytest.raises(SystemExit):
        cli.novelty_check(types.SimpleNamespace(novelty=8), 40)                          # cl_vae's flattened windows


def test_the_tools_print_their_help():
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'clvae_amd.novelty', '--help'], capture_output=True, text=True, timeout=120,
                       stdin=subprocess.DEVNULL, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ('--train_file', '--split', '--against', '-w', '--hop', '--transpose', '--rolls', '--out'):
        assert flag in r.stdout, flag
    for which in ('cl_vae', 'cl_vrnn'):
        script = os.path.join(ROOT, 'classifying-vae-lstm_amd', which, 'sample.py')
        r = subprocess.run([sys.executable, script, '--help'], capture_output=True, text=True, timeout=120, stdin=subprocess.DEVNULL)
        assert r.returncode == 0, r.stderr[-2000:]
        assert '--novelty' in r.stdout and '--novelty_transpose' in r.stdout
