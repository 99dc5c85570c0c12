"""CPU: the particle-filter entry points are declared, bound and refuse bad arguments before touching a device; the
argument checks of generate_smc and the sample CLIs' --particles flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from clvae_amd import _lib
from helpers import ROOT

NEW = ('clv_smc_sample', 'clv_smc_resample', 'clv_smc_gather', 'clv_smc_backtrack')


def test_smc_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'clvae.h')).read()
    for n in NEW:
        assert re.search(r'\bint %s\(' % n, hdr), n
        assert n in _lib.SIGNATURES, n
    assert _lib.ABI_VERSION == 610


def test_smc_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    dummy = (C.c_double * 64)()
    p = C.cast(dummy, C.c_void_p)
    einval = L.clv_smc_sample(0, 88, 1, 1, 0, *([p] * 7), None)
    assert einval < 0
    good = [6, 88, 3, 2, 0] + [p] * 7
    for i, bad in ((0, 0), (1, 0), (2, 0), (2, 4), (3, 0), (4, -1), (5, None), (7, None), (8, None), (10, None), (11, None)):
        a = list(good)
        a[i] = bad
        assert L.clv_smc_sample(*a, None) == einval, i
    good = [2, 3, 4, 0, 0, 0, 0.5] + [p] * 8
    for i, bad in ((0, 0), (1, 0), (1, 1025), (2, 0), (3, -1), (5, -1), (6, -0.1), (6, 1.5), (6, float('nan')), (7, None),
                   (13, None), (14, None)):
        a = list(good)
        a[i] = bad
        assert L.clv_smc_resample(*a, None) == einval, i
    ptrs, widths = (C.c_void_p * 2)(p, p), (C.c_int * 2)(88, 0)
    assert L.clv_smc_gather(6, 3, 2, 0, 2, C.cast(ptrs, C.c_void_p), C.cast(widths, C.c_void_p), p, p, p, p, None) == einval
    assert L.clv_smc_gather(6, 3, 2, 0, 9, C.cast(ptrs, C.c_void_p), C.cast(widths, C.c_void_p), p, p, p, p, None) == einval
    assert L.clv_smc_gather(6, 4, 2, 0, 1, C.cast(ptrs, C.c_void_p), C.cast(widths, C.c_void_p), p, p, p, p, None) == einval
    good = [2, 3, 4, 88, 1, 0, 0, 4] + [p] * 4 + [None]
    for i, bad in ((0, 0), (1, 2000), (2, 0), (3, 0), (4, 0), (6, -1), (7, -1), (8, None), (9, None), (10, None), (11, None)):
        a = list(good)
        a[i] = bad
        assert L.clv_smc_backtrack(*a, None) == einval, i


def test_generate_smc_argument_checks():
    from clvae_amd.engine_generate import smc_args
    cpu = torch.device('cpu')
    roll = np.full((2, 3, 88), 255, np.uint8)
    assert smc_args(roll, 4, 0.5, 1, 2, 3, 88, cpu).shape == (2, 3, 88)
    for kw in (dict(clamp=None), dict(particles=0), dict(particles=1025), dict(particles=2.5), dict(particles=True),
               dict(tau=-0.01), dict(tau=1.01), dict(tau=float('nan')), dict(n_out=0), dict(nsteps=0)):
        a = dict(clamp=roll, particles=4, tau=0.5, n_out=1, nsteps=3)
        a.update(kw)
        with pytest.raises(ValueError):
            smc_args(a['clamp'], a['particles'], a['tau'], a['n_out'], 2, a['nsteps'], 88, cpu)


@pytest.mark.parametrize('tool', ['cl_vae.sample', 'cl_vrnn.sample'])
def test_particles_flag_needs_harmonize(tool):
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, HARMONIZE_FLAGS, parser_for
    p = parser_for(tool, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS)
    assert p.parse_args(['r']).particles is None
    assert p.parse_args(['r', '--harmonize', 'top', '--particles', '16']).particles == 16
    for bad in (['r', '--particles', '8'], ['r', '--harmonize', 'top', '--particles', '0'],
                ['r', '--device_loop', '--particles', '2']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
