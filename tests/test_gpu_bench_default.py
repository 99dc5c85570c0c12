"""-m gpu: `python bench.py` as the driver runs it (no flags but a short --steps / --warmup), plain and with `--full`.

A plain run prints ONE JSON line with the contract's keys and nothing it did not measure in its timed region.  `--full` adds
`roofline` (traffic measured in the run), `cpu_baseline`, and the `also` list from its child process -- every piece of that
path, so that a slip in any of them (round 6: a NameError behind the headline, in the `also` child's timeout) fails here and
not in a later run.  Both dump the same arrays: nothing `--full` adds runs between the warm-up and the dump."""
import json
import os
import subprocess
import sys

import pytest

from helpers import ROOT

pytestmark = pytest.mark.gpu


def test_default_bench_line_is_whole():
    pytest.importorskip("torch")
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    env = dict(os.environ)
    env.pop('CLV_LIB', None)
    pr = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '10', '--warmup', '3', '--full'], cwd=ROOT,
                        env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [l for l in pr.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, pr.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
              'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['n_gpus'] == 1 and d['steps'] == 10 and d['warmup'] == 3 and d['dtype'] == 'f32' and d['vs_baseline'] is None
    assert abs(d['value'] - 256 * 128 / (d['ms_per_step'] * 1e-3)) < 1e-3 * d['value']
    r = d['roofline']
    assert r['bound'] == 'mfma' and 0.05 < r['frac'] < 1.0 and r['peak'] == 157.3 and abs(r['frac'] - r['achieved'] / r['peak']) < 1e-3
    assert r['traffic'] is None or r['traffic'] > 1e6
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['value'] > 0 and c['cores'] >= 1
    also = d.get('also')
    assert isinstance(also, list) and len(also) >= 6, also
    assert not [a for a in also if 'error' in a], also


def test_plain_bench_line_is_the_headline_alone():
    """`python bench.py` without --full: the contract's keys with what they meant before, and none of the extras -- no PMC
    child passes, no per-kernel times, no CPU baseline, no host-issue steps, no `also` child."""
    pytest.importorskip("torch")
    import numpy as np
    import time
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    env = dict(os.environ)
    env.pop('CLV_LIB', None)
    t0 = time.perf_counter()
    pr = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '10', '--warmup', '3'], cwd=ROOT, env=env,
                        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert pr.returncode == 0, pr.stderr[-2000:]
    lines = [l for l in pr.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, pr.stdout[-2000:]
    d = json.loads(lines[0])
    assert d['metric'] == 'piano-roll timesteps/sec (train)' and d['unit'] == 'timesteps/s' and d['higher_is_better'] is True
    assert d['n_gpus'] == 1 and d['steps'] == 10 and d['warmup'] == 3 and d['dtype'] == 'f32' and d['vs_baseline'] is None
    assert abs(d['value'] - 256 * 128 / (d['ms_per_step'] * 1e-3)) < 1e-3 * d['value']
    assert np.isfinite(d['final_loss'])
    for k in ('roofline', 'cpu_baseline', 'host_issue_us_per_step', 'allreduce_alone'):
        assert k in d and d[k] is None, (k, d.get(k))
    assert 'also' not in d
    assert 'pmc traffic passes' not in pr.stderr and 'headline (repeated' not in pr.stderr
    print("plain run: %.1f s in all, %.1f s outside the warm-up and timed steps" % (wall, wall - 13 * d['ms_per_step'] * 1e-3))


def test_a_plain_and_a_full_run_dump_the_same_outputs(tmp_path):
    """--full times the set-up's kernel-time pass (whose steps put the state back) and measures its other extras after the
    dump: a plain run and a --full run of the same arguments dump the same arrays, bit for bit."""
    pytest.importorskip("torch")
    import numpy as np
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    env = dict(os.environ)
    env.pop('CLV_LIB', None)
    dirs = {}
    for mode, extra in (('plain', []), ('full', ['--full', '--no-cpu-baseline', '--no-pmc-traffic', '--no-also'])):
        dirs[mode] = str(tmp_path / mode)
        pr = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '4', '--warmup', '2', '--dump-outputs',
                             dirs[mode]] + extra, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                            timeout=600)
        assert pr.returncode == 0, pr.stderr[-2000:]
        d = json.loads(pr.stdout.strip().splitlines()[-1])
        assert (d['roofline'] is not None) == (mode == 'full'), mode
    names = sorted(os.listdir(dirs['plain']))
    assert names == sorted(os.listdir(dirs['full'])) and 'losses.npy' in names
    for n in names:
        a, b = (np.load(os.path.join(dirs[m], n)) for m in ('plain', 'full'))
        np.testing.assert_array_equal(a, b, err_msg=n)


def test_dump_outputs_are_the_same_in_two_runs(tmp_path):
    """`bench.py --dump-outputs DIR`: the last timed step's loss terms, updated weights and gradients (one file per Keras
    layer tensor), finite, and bit for bit the same in two runs with the same arguments (seeded inputs, deterministic step)."""
    pytest.importorskip("torch")
    import numpy as np
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    env = dict(os.environ)
    env.pop('CLV_LIB', None)
    dirs = [str(tmp_path / d) for d in ('a', 'b')]
    for d in dirs:
        pr = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '4', '--warmup', '2', '--no-cpu-baseline',
                             '--no-pmc-traffic', '--no-also', '--dump-outputs', d], cwd=ROOT, env=env,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
        assert pr.returncode == 0, pr.stderr[-2000:]
        assert json.loads(pr.stdout.strip().splitlines()[-1])['steps'] == 4
    names = sorted(os.listdir(dirs[0]))
    assert names == sorted(os.listdir(dirs[1]))
    assert 'losses.npy' in names and 'weights.hW.kernel.npy' in names and 'grads.hW.kernel.npy' in names
    assert len([n for n in names if n.startswith('weights.')]) == len([n for n in names if n.startswith('grads.')]) > 10
    for n in names:
        a, b = (np.load(os.path.join(d, n)) for d in dirs)
        assert a.dtype == (np.float64 if n == 'losses.npy' else np.float32), n
        assert np.isfinite(a).all(), n
        np.testing.assert_array_equal(a, b, err_msg=n)
