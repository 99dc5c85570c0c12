"""Particle-filter sampling throughput at the cl_vrnn default shape: G melodies x P particles x nsteps
frames through VrnnEngine.generate_smc, against the clamped frame chain (generate(persistent=False, clamp=...)) on the same
G * P rows, which runs the same frame launches without the filter.  Runs alternate; medians are printed as one JSON line.

    python tools/smc_bench.py [--melodies 64] [--particles 128] [--nsteps 64] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clvae_amd  # noqa: E402,F401
from clvae_amd.engine import VrnnEngine  # noqa: E402
from clvae_amd.harmonize import FREE  # noqa: E402
from clvae_amd.initializers import init_weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--melodies', type=int, default=64)
ap.add_argument('--particles', type=int, default=128)
ap.add_argument('--nsteps', type=int, default=64)
ap.add_argument('--seed_frames', type=int, default=1)
ap.add_argument('--tau', type=float, default=0.5)
ap.add_argument('--reps', type=int, default=5)
args = ap.parse_args()
dev = torch.device('cuda:0')
G, P, T, S = args.melodies, args.particles, args.nsteps, args.seed_frames
cfg = dict(D=88, H=88, L=2, T=16, C=10, use_x_prev=True, class_weight=1.0, kl_weight=1.0, w_kl_weight=1.0,
           w_log_var_prior=0.0, gate_act='hard_sigmoid')
eng = VrnnEngine(cfg, 1, dev)
wts = init_weights(eng.P.logical, cfg, seed=0)
wts['X_decoded_mean/bias'] = np.full_like(wts['X_decoded_mean/bias'], -3.07)     # logit(0.0443): piano-roll note density
eng.P.set_weights(wts)
rng = np.random.default_rng(0)
seeds = torch.as_tensor((rng.random((G, S, 88)) < 0.0443).astype(np.float32), device=dev)
wv = torch.as_tensor(np.eye(10, dtype=np.float32)[rng.integers(0, 10, G)], device=dev)
# a melody voice: one note forced on per frame and every note above it forced off (harmonize --harmonize top)
top = rng.integers(50, 80, (G, T))
roll = np.full((G, T, 88), FREE, np.uint8)
idx = np.arange(88)
roll[idx[None, None, :] > top[..., None]] = 0
np.put_along_axis(roll, top[..., None], 1, axis=2)
clamp = torch.as_tensor(roll, device=dev)
clamp_rows = clamp.repeat_interleave(P, 0)
seeds_rows, wv_rows = seeds.repeat_interleave(P, 0), wv.repeat_interleave(P, 0)


def smc():
    return eng.generate_smc(seeds, wv, T, clamp, P, resample_threshold=args.tau, seed=2)


def chain():
    return eng.generate(seeds_rows, wv_rows, T, seed=2, persistent=False, clamp=clamp_rows)


smc(); chain(); torch.cuda.synchronize()
t = {'smc': [], 'chain': []}
for rep in range(args.reps):
    for name in (('smc', 'chain') if rep % 2 == 0 else ('chain', 'smc')):
        t0 = time.perf_counter()
        out = smc() if name == 'smc' else chain()
        if name == 'smc':
            r = out
        torch.cuda.synchronize()
        t[name].append(time.perf_counter() - t0)
med = {k: float(np.median(v)) for k, v in t.items()}
frames = S + T
print(json.dumps({
    'tool': 'smc_bench', 'melodies': G, 'particles': P, 'nsteps': T, 'seed_frames': S, 'tau': args.tau, 'reps': args.reps,
    'smc_s': med['smc'], 'chain_s': med['chain'],
    'smc_us_per_frame': 1e6 * med['smc'] / frames, 'chain_us_per_frame': 1e6 * med['chain'] / frames,
    'smc_overhead_pct': 100 * (med['smc'] / med['chain'] - 1),
    'particle_frames_per_s': G * P * T / med['smc'],
    'resamples_per_melody': float(r.resamples.float().mean()), 'mean_log_evidence_per_frame': float(r.log_evidence.mean()) / T,
}))
