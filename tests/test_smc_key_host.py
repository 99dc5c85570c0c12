"""CPU: the key-inference entry points of the particle filter are declared, bound and refuse bad arguments
before touching a device; WPrior's validation; the argument rules of generate_smc, harmonize and the sample CLIs'
--infer_key flag."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from clvae_amd import _lib
from helpers import ROOT

NEW = ('clv_smc_init_w', 'clv_smc_w_posterior', 'clv_smc_take_w')


def test_key_entry_points_are_declared_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'clvae.h')).read()
    for n in NEW:
        assert re.search(r'\bint %s\(' % n, hdr), n
        assert n in _lib.SIGNATURES, n
        assert hasattr(_lib.lib(), n), n
    assert _lib.ABI_VERSION == 610
    from clvae_amd import trainer
    assert trainer.SMC_W_STREAM == 0xFFFFFFFC and trainer.SMC_W_STREAM == trainer.SMC_STREAM - 1
    src = open(os.path.join(ROOT, 'classifying-vae-lstm_amd', 'csrc', 'smc.hip')).read()
    assert re.search(r'SMC_W_STREAM\s*=\s*0xFFFFFFFCu', src)


def test_key_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    dummy = (C.c_double * 64)()
    p = C.cast(dummy, C.c_void_p)
    einval = L.clv_smc_sample(0, 88, 1, 1, 0, *([p] * 7), None)
    assert einval < 0
    # clv_smc_init_w(G, P, C, mode, seed, m0, probs, mean, log_var, wr, stream)
    good = [2, 3, 4, 0, 0, 0, p, None, None, p]
    for i, bad in ((0, 0), (1, 0), (1, 1025), (2, 1), (2, 33), (3, 2), (3, -1), (5, -1), (6, None), (9, None)):
        a = list(good)
        a[i] = bad
        assert L.clv_smc_init_w(*a, None) == einval, i
    good = [2, 3, 4, 1, 0, 0, None, p, p, p]
    for i, bad in ((7, None), (8, None), (9, None), (2, 1)):
        a = list(good)
        a[i] = bad
        assert L.clv_smc_init_w(*a, None) == einval, i
    # clv_smc_w_posterior(G, P, C, nsteps, S, logW, wr, step_dev, out, stream)
    good = [2, 3, 4, 5, 0] + [p] * 4
    for i, bad in ((0, 0), (1, 0), (1, 1025), (2, 1), (2, 33), (3, 0), (4, -1), (5, None), (6, None), (7, None), (8, None)):
        a = list(good)
        a[i] = bad
        assert L.clv_smc_w_posterior(*a, None) == einval, i
    # clv_smc_take_w(G, P, C, n_out, picks, wr, w_out, stream)
    good = [2, 3, 4, 1] + [p] * 3
    for i, bad in ((0, 0), (1, 0), (1, 1025), (2, 1), (2, 33), (3, 0), (4, None), (5, None), (6, None)):
        a = list(good)
        a[i] = bad
        assert L.clv_smc_take_w(*a, None) == einval, i


def test_w_prior_validation():
    from clvae_amd.engine_generate import WPrior, smc_label_args
    cpu = torch.device('cpu')
    pr = WPrior.categorical([[0.25, 0.75, 0.0], [0.0, 0.0, 1.0]])
    assert (pr.kind, pr.N, pr.C) == ('categorical', 2, 3) and pr.probs.dtype == np.float64
    assert np.array_equal(pr.probs, [[0.25, 0.75, 0.0], [0.0, 0.0, 1.0]])
    assert WPrior.categorical([0.5, 0.5]).N == 1                      # one row
    near = WPrior.categorical([[0.3, 0.7 + 5e-7]])                    # within 1e-6: accepted and renormalised
    assert abs(near.probs.sum() - 1) < 1e-15
    u = WPrior.uniform(3, 10)
    assert u.probs.shape == (3, 10) and np.all(u.probs == 0.1)
    for bad in ([[0.5, 0.6]], [[0.5, 0.4]], [[1.5, -0.5]], [[np.nan, 1.0]], [[np.inf, 0.0]], [[1.0]], np.ones((2, 2, 2)) / 2,
                np.full((1, 33), 1 / 33.0), np.zeros((0, 3))):
        with pytest.raises(ValueError):
            WPrior.categorical(bad)
    ln = WPrior.logistic_normal(np.zeros((4, 9)), np.full((4, 9), -1.0))
    assert (ln.kind, ln.N, ln.C) == ('logistic_normal', 4, 10) and ln.mean.dtype == np.float32 == ln.log_var.dtype
    for m, lv in ((np.zeros((4, 9)), np.zeros((4, 8))), (np.zeros((4, 9)), np.full((4, 9), np.nan)),
                  (np.full((4, 9), np.inf), np.zeros((4, 9))), (np.zeros((2, 32)), np.zeros((2, 32))),
                  (np.zeros((2, 2, 3)), np.zeros((2, 2, 3)))):
        with pytest.raises(ValueError):
            WPrior.logistic_normal(m, lv)
    # exactly one of w and w_prior; the prior's shape is the call's
    w = torch.zeros(2, 3)
    assert smc_label_args(w, None, 2, 3, cpu)[1] is None
    got = smc_label_args(None, pr, 2, 3, cpu)
    assert got[0] is None and got[1].probs.dtype == torch.float64 and tuple(got[1].probs.shape) == (2, 3)
    for a in ((None, None, 2, 3), (w, pr, 2, 3), (None, pr, 3, 3), (None, pr, 2, 4), (None, pr.probs, 2, 3)):
        with pytest.raises(ValueError):
            smc_label_args(*a, cpu)


def test_smc_results_keep_their_fields():
    from clvae_amd.engine_generate import SmcKeyResult, SmcResult
    assert SmcResult._fields == ('Xs', 'log_evidence', 'ess', 'resamples')          # callers iterate over all of them
    assert SmcKeyResult._fields == SmcResult._fields + ('w_posterior', 'w_out')


class _Model:
    class engine:
        cfg = dict(C=5, w_log_var_prior=-0.5)


def test_harmonize_key_argument_rules():
    from clvae_amd.harmonize import default_w_prior, harmonize
    d = default_w_prior(_Model, 3, 'discrete')
    assert d.kind == 'categorical' and np.all(d.probs == 0.2) and d.probs.shape == (3, 5)
    c = default_w_prior(_Model, 3, 'continuous')
    assert c.kind == 'logistic_normal' and np.all(c.mean == 0) and np.all(c.log_var == np.float32(-0.5))
    assert c.mean.shape == (3, 4)
    seeds, rolls, w = np.zeros((2, 88)), np.zeros((2, 4, 88)), np.eye(5)[[0, 1]]
    for kw in (dict(infer_key='discrete'),                                   # a single path cannot weigh keys
               dict(infer_key='discrete', particles=4, w_vals=w),            # both
               dict(infer_key='modal', particles=4),
               dict(w_prior=d, particles=4, w_vals=w),                       # a prior without infer_key
               dict(particles=4)):                                           # neither
        with pytest.raises(ValueError):
            harmonize(_Model, seeds, rolls, **kw)


@pytest.mark.parametrize('tool', ['cl_vae.sample', 'cl_vrnn.sample'])
def test_infer_key_flag_needs_particles(tool, capsys):
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, HARMONIZE_FLAGS, parser_for
    p = parser_for(tool, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS)
    assert p.parse_args(['r']).infer_key is None
    assert p.parse_args(['r', '--harmonize', 'top', '--particles', '8']).infer_key is None
    for mode in ('discrete', 'continuous'):
        a = p.parse_args(['r', '--harmonize', 'top', '--particles', '8', '--infer_key', mode])
        assert a.infer_key == mode and a.particles == 8 and not a.infer_w
    capsys.readouterr()
    for bad, msg in ((['r', '--infer_key', 'discrete'], '--infer_key needs --particles'),
                     (['r', '--harmonize', 'top', '--infer_key', 'discrete'], '--infer_key needs --particles'),
                     (['r', '--particles', '8', '--infer_key', 'discrete'], '--particles needs --harmonize'),
                     (['r', '--harmonize', 'top', '--particles', '8', '--infer_key', 'modal'], 'invalid choice')):
        with pytest.raises(SystemExit) as e:
            p.parse_args(bad)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err
