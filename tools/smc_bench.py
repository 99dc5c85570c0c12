"""Particle-filter sampling throughput at the cl_vrnn default shape: G melodies x P particles x nsteps
frames through VrnnEngine.generate_smc, against the clamped frame chain (generate(persistent=False, clamp=...)) on the same
G * P rows, which runs the same frame launches without the filter.  Runs alternate; medians are printed as one JSON line.
--infer_key adds the filter with a label per particle on the same rows, in the same alternation: a uniform
categorical prior over the keys and / or the model's own logistic-normal prior, each against the fixed-label filter.
--voices LO[:HI] adds the filter and the clamped chain under that voice count per frame, the top-voice roll
kept, in the same alternation: clv_smc_sample_voices / clv_bernoulli_sample_voices in place of their twins.
--sweeps K adds particle Gibbs on the same melodies and particles, in the same alternation: generate_gibbs with
K sweeps and with one (the filter plus the bookkeeping of a retained path); a conditional sweep costs (t_K - t_1) / (K - 1).

    python tools/smc_bench.py [--melodies 64] [--particles 128] [--nsteps 64] [--reps 5] [--infer_key both] [--voices 4] [--sweeps 4]
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
from clvae_amd.cli import parse_voices  # noqa: E402
from clvae_amd.engine_generate import Constraints, WPrior  # noqa: E402
from clvae_amd.harmonize import FREE  # noqa: E402
from clvae_amd.initializers import init_weights  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--melodies', type=int, default=64)
ap.add_argument('--particles', type=int, default=128)
ap.add_argument('--nsteps', type=int, default=64)
ap.add_argument('--seed_frames', type=int, default=1)
ap.add_argument('--tau', type=float, default=0.5)
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--infer_key', choices=('categorical', 'logistic_normal', 'both'), default=None)
ap.add_argument('--voices', default=None, help='LO[:HI]: also run both samplers under this voice count per frame')
ap.add_argument('--sweeps', type=int, default=None, help='K >= 2: also run particle Gibbs with K sweeps and with one')
args = ap.parse_args()
if args.sweeps is not None and args.sweeps < 2:
    ap.error('--sweeps must be >= 2')
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


priors = {'categorical': WPrior.uniform(G, 10),
          'logistic_normal': WPrior.logistic_normal(np.zeros((G, 9)), np.full((G, 9), cfg['w_log_var_prior']))}
key_modes = [] if args.infer_key is None else list(priors) if args.infer_key == 'both' else [args.infer_key]


def smc(prior=None):
    if prior is None:
        return eng.generate_smc(seeds, wv, T, clamp, P, resample_threshold=args.tau, seed=2)
    return eng.generate_smc(seeds, None, T, clamp, P, resample_threshold=args.tau, seed=2, w_prior=priors[prior])


def chain():
    return eng.generate(seeds_rows, wv_rows, T, seed=2, persistent=False, clamp=clamp_rows)


voice_modes = []
if args.voices is not None:
    lo, hi = parse_voices(args.voices)
    counted = Constraints.between(lo, hi, roll=clamp).resolve(G, T, 88, dev)
    counted_rows = Constraints.between(lo, hi, roll=clamp_rows).resolve(G * P, T, 88, dev)
    voice_modes = ['smc_voices', 'chain_voices']

gibbs_modes = [] if args.sweeps is None else ['gibbs', 'gibbs1']
names = ['smc', 'chain'] + key_modes + voice_modes + gibbs_modes
run = {'smc': smc, 'chain': chain,
       'gibbs': lambda: eng.generate_gibbs(seeds, wv, T, clamp, P, args.sweeps, resample_threshold=args.tau, seed=2),
       'gibbs1': lambda: eng.generate_gibbs(seeds, wv, T, clamp, P, 1, resample_threshold=args.tau, seed=2),
       'smc_voices': lambda: eng.generate_smc(seeds, wv, T, counted, P, resample_threshold=args.tau, seed=2),
       'chain_voices': lambda: eng.generate(seeds_rows, wv_rows, T, seed=2, persistent=False, clamp=counted_rows), 'categorical': lambda: smc('categorical'), 'logistic_normal': lambda: smc('logistic_normal')}
for name in names:
    run[name]()
torch.cuda.synchronize()
t, last = {name: [] for name in names}, {}
for rep in range(args.reps):
    for name in (names if rep % 2 == 0 else names[::-1]):
        t0 = time.perf_counter()
        last[name] = run[name]()
        torch.cuda.synchronize()
        t[name].append(time.perf_counter() - t0)
med = {k: float(np.median(v)) for k, v in t.items()}
frames = S + T
r = last['smc']
res = {
    'tool': 'smc_bench', 'melodies': G, 'particles': P, 'nsteps': T, 'seed_frames': S, 'tau': args.tau, 'reps': args.reps,
    'smc_s': med['smc'], 'chain_s': med['chain'],
    'smc_us_per_frame': 1e6 * med['smc'] / frames, 'chain_us_per_frame': 1e6 * med['chain'] / frames,
    'smc_overhead_pct': 100 * (med['smc'] / med['chain'] - 1),
    'particle_frames_per_s': G * P * T / med['smc'],
    'resamples_per_melody': float(r.resamples.float().mean()), 'mean_log_evidence_per_frame': float(r.log_evidence.mean()) / T,
}
for mode in key_modes:
    k = last[mode]
    res['key_' + mode] = {
        's': med[mode], 'us_per_frame': 1e6 * med[mode] / frames, 'over_fixed_w_smc_pct': 100 * (med[mode] / med['smc'] - 1),
        'all_s': t[mode], 'resamples_per_melody': float(k.resamples.float().mean()),
        'mean_log_evidence_per_frame': float(k.log_evidence.mean()) / T,
        'mean_max_key_posterior': float(k.w_posterior[:, -1].max(dim=1).values.mean()),
    }
if voice_modes:
    k = last['smc_voices']
    res['voices'] = {
        'range': [lo, hi], 'smc_s': med['smc_voices'], 'chain_s': med['chain_voices'],
        'smc_over_roll_only_pct': 100 * (med['smc_voices'] / med['smc'] - 1),
        'chain_over_roll_only_pct': 100 * (med['chain_voices'] / med['chain'] - 1),
        'smc_all_s': t['smc_voices'], 'chain_all_s': t['chain_voices'], 'roll_only_chain_all_s': t['chain'],
        'resamples_per_melody': float(k.resamples.float().mean()),
        'mean_log_evidence_per_frame': float(k.log_evidence.mean()) / T,
        'counts_in_range': bool(((k.Xs.sum(-1) >= lo) & (k.Xs.sum(-1) <= hi)).all()),
    }
if gibbs_modes:
    k, K = last['gibbs'], args.sweeps
    per = (med['gibbs'] - med['gibbs1']) / (K - 1)
    res['gibbs'] = {
        'sweeps': K, 's': med['gibbs'], 'one_sweep_s': med['gibbs1'], 'conditional_sweep_s': per,
        'conditional_sweep_us_per_frame': 1e6 * per / frames, 'conditional_sweep_over_smc_pct': 100 * (per / med['smc'] - 1),
        'one_sweep_over_smc_pct': 100 * (med['gibbs1'] / med['smc'] - 1), 'all_s': t['gibbs'], 'one_sweep_all_s': t['gibbs1'],
        'sweep0_is_the_filter': bool(torch.equal(k.Xs[:, 0], r.Xs[:, 0]) and torch.equal(k.log_evidence[:, 0], r.log_evidence)),
        'renewed_per_sweep': [float(v) for v in k.renewed.float().mean(dim=(0, 2))],
        'mean_log_z_per_frame_per_sweep': [float(v) / T for v in k.log_evidence.mean(dim=0)],
    }
if key_modes or voice_modes or gibbs_modes:
    res['smc_all_s'] = t['smc']
print(json.dumps(res))
