"""Tiny engines and inputs for the filter-stream tests (the builders of tests/test_gpu_smc.py, kept here so that a test file
does not import another), and the one-call filter with its ancestor table kept."""
import types

import numpy as np
import torch

from oracle import clvae_oracle as O

FREE = 255
D = 88


def roll(rng, N, nsteps, frac=0.3, on=0.3):
    """about `frac` of the notes clamped, `on` of those forced on"""
    r = rng.random((N, nsteps, D))
    return np.where(r < frac, (r < frac * on).astype(np.uint8), np.uint8(FREE)).astype(np.uint8)


def vrnn(dev, L=2, B=4, seed=5):
    from clvae_amd.engine import VrnnEngine
    cfg = O.vrnn_config(latent_dim=L, seq_length=8, n_classes=10, use_x_prev=True, gate_act='hard_sigmoid')
    rng = np.random.default_rng(L)
    p = {k: np.asarray(v, np.float32) for k, v in O.vrnn_init_params(cfg, seed=seed).items()}
    for k in p:
        if not k.startswith('hW'):
            p[k] = (p[k] + 0.15 * rng.standard_normal(p[k].shape)).astype(np.float32)
    eng = VrnnEngine(cfg, B, dev)
    eng.P.set_weights(p)
    return eng


def vae(dev, L=3, C=4, B=32):
    from clvae_amd.engine import VaeEngine
    cfg = O.vae_config(latent_dim=L, n_classes=C, use_x_prev=True)
    rng = np.random.default_rng(L + C)
    p = {k: np.asarray(v, np.float32) for k, v in O.vae_init_params(cfg, seed=6).items()}
    for k in p:
        p[k] = (p[k] + 0.1 * rng.standard_normal(p[k].shape)).astype(np.float32)
    p['x_decoded_mean/bias'] = (p['x_decoded_mean/bias'] - 2.0).astype(np.float32)
    eng = VaeEngine(cfg, B, dev)
    eng.P.set_weights(p)
    return eng


def inputs(N, S, C, seed):
    """host seeds [N, S, 88] (S None: [N, 88]) and one-hot labels [N, C]"""
    rng = np.random.default_rng(seed)
    shape = (N, S, D) if S is not None else (N, D)
    return (rng.random(shape) < 0.06).astype(np.float32), np.eye(C, dtype=np.float32)[rng.integers(0, C, N)]


def model_of(eng):
    """what stream.Stream / FilterStream need of a model: its engine"""
    return types.SimpleNamespace(engine=eng)


def one_call(eng, x_seed, w, nsteps, clamp, particles, **kw):
    """eng.generate_smc(...) on host inputs, and the chunk objects (_Smc: anc, hist, logW) its driver ran"""
    from clvae_amd import engine_generate as EG
    kept, real = [], EG._smc_drive

    def drive(chunks, run_chunk, *a, **k):
        def keep(m0, m1):
            kept.append(run_chunk(m0, m1))
            return kept[-1]
        return real(chunks, keep, *a, **k)
    EG._smc_drive = drive
    try:
        t = lambda a: torch.as_tensor(a, device=eng.device)
        res = eng.generate_smc(t(x_seed), t(w), nsteps, clamp, particles, **kw)
    finally:
        EG._smc_drive = real
    torch.cuda.synchronize()
    return res, kept
