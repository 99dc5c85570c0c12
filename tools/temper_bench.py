"""Cost of a sampling temperature.

Default: the persistent generation kernels at the shapes bench.py uses for gen1, gen1024, gen_vae1 and gen_vae1024, tempered
(--temperature 0.8 --z_temperature 0.9) against untempered in one process, alternating; medians of --reps runs each with
the spread of the untempered runs next to the difference; one JSON line.  These kernels' time follows the number of notes
that sound (a frame's projection is a gather of the rows of its notes), and a temperature changes that number; the third
variant, `near_one` (T = 1.0000001, Tz = 0.9999999: the tempered instances on all but the same frames), isolates what the
two multiplies cost.  The note density of each variant is printed next to its time.

    python tools/temper_bench.py [--steps 240] [--reps 7]

--smc: one particle-filter run at DESIGN.md 11's shape (64 melodies x 128 particles x 64 frames), untempered or, with
--tempered, at the temperatures above, for a kernel trace with statistics in a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/temper_bench.py --smc [--tempered]
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
from clvae_amd.engine import VaeEngine, VrnnEngine  # noqa: E402
from clvae_amd.harmonize import FREE  # noqa: E402
from clvae_amd.initializers import init_weights  # noqa: E402

NOTE_DENSITY = 0.0443
ap = argparse.ArgumentParser()
ap.add_argument('--steps', type=int, default=240)
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--temperature', type=float, default=0.8)
ap.add_argument('--z_temperature', type=float, default=0.9)
ap.add_argument('--smc', action='store_true')
ap.add_argument('--tempered', action='store_true')
args = ap.parse_args()
dev = torch.device('cuda:0')
TEMPER = dict(temperature=args.temperature, z_temperature=args.z_temperature)
BIAS = float(np.log(NOTE_DENSITY / (1 - NOTE_DENSITY)))


def vrnn(N, L, C, S=16):
    cfg = dict(D=88, H=88, L=L, T=16, C=C, use_x_prev=True, class_weight=1.0, kl_weight=1.0, w_kl_weight=1.0,
               w_log_var_prior=0.0, gate_act='hard_sigmoid')
    eng = VrnnEngine(cfg, 1, dev)
    wts = init_weights(eng.P.logical, cfg, seed=0)
    wts['X_decoded_mean/bias'] = np.full_like(wts['X_decoded_mean/bias'], BIAS)
    eng.P.set_weights(wts)
    rng = np.random.default_rng(1234)
    seeds = torch.as_tensor((rng.random((N, S, 88)) < NOTE_DENSITY).astype(np.float32), device=dev)
    wv = torch.as_tensor(np.eye(C, dtype=np.float32)[rng.integers(0, C, N)], device=dev)
    return eng, seeds, wv


def vae(N, L, C):
    cfg = dict(D=88, H=88, L=L, Hc=88, C=C, use_x_prev=True, class_weight=1.0, kl_weight=1.0, w_kl_weight=1.0,
               w_log_var_prior=0.0)
    eng = VaeEngine(cfg, 4, dev)
    wts = init_weights(eng.P.logical, cfg, seed=0)
    wts['x_decoded_mean/bias'] = np.full_like(wts['x_decoded_mean/bias'], BIAS)
    eng.P.set_weights(wts)
    rng = np.random.default_rng(1234)
    seeds = torch.as_tensor((rng.random((N, 88)) < NOTE_DENSITY).astype(np.float32), device=dev)
    wv = torch.as_tensor(np.eye(C, dtype=np.float32)[rng.integers(0, C, N)], device=dev)
    return eng, seeds, wv


def smc_run():
    G, P, T = 64, 128, 64
    eng, seeds, wv = vrnn(G, 2, 10, S=1)
    rng = np.random.default_rng(0)
    top = rng.integers(50, 80, (G, T))
    roll = np.full((G, T, 88), FREE, np.uint8)
    roll[np.arange(88)[None, None, :] > top[..., None]] = 0
    np.put_along_axis(roll, top[..., None], 1, axis=2)
    kw = TEMPER if args.tempered else {}
    t0 = time.perf_counter()
    r = eng.generate_smc(seeds, wv, T, torch.as_tensor(roll, device=dev), P, seed=2, **kw)
    torch.cuda.synchronize()
    print(json.dumps({'tool': 'temper_bench --smc', 'tempered': bool(args.tempered), **(kw or {}), 'melodies': G, 'particles': P,
                      'nsteps': T, 'wall_s': time.perf_counter() - t0,
                      'mean_log_evidence_per_frame': float(r.log_evidence.mean()) / T}))


def compare(name, eng, seeds, wv, frames_per_run):
    run = {'plain': lambda: eng.generate(seeds, wv, args.steps, seed=2),
           'tempered': lambda: eng.generate(seeds, wv, args.steps, seed=2, **TEMPER),
           'near_one': lambda: eng.generate(seeds, wv, args.steps, seed=2, temperature=1.0000001, z_temperature=0.9999999)}
    density = {k: float(f().mean()) for k, f in run.items()}
    torch.cuda.synchronize()
    t = {k: [] for k in run}
    for rep in range(args.reps):
        for k in (list(run) if rep % 2 == 0 else list(run)[::-1]):
            t0 = time.perf_counter()
            run[k]()
            torch.cuda.synchronize()
            t[k].append(time.perf_counter() - t0)
    med = {k: float(np.median(v)) for k, v in t.items()}
    return {'workload': name, 'plain_ms': 1e3 * med['plain'], 'tempered_ms': 1e3 * med['tempered'],
            'near_one_ms': 1e3 * med['near_one'], 'difference_pct': 100 * (med['tempered'] / med['plain'] - 1),
            'near_one_difference_pct': 100 * (med['near_one'] / med['plain'] - 1), 'note_density': density,
            'plain_spread_pct': 100 * (max(t['plain']) - min(t['plain'])) / med['plain'],
            'plain_frames_per_s': frames_per_run / med['plain'], 'tempered_frames_per_s': frames_per_run / med['tempered'],
            'plain_all_ms': [1e3 * v for v in t['plain']], 'tempered_all_ms': [1e3 * v for v in t['tempered']],
            'near_one_all_ms': [1e3 * v for v in t['near_one']]}


if args.smc:
    smc_run()
else:
    out = []
    for name, N in (('gen1', 1), ('gen1024', 1024)):
        eng, seeds, wv = vrnn(N, 32, 10)
        out.append(compare(name, eng, seeds, wv, N * (args.steps + 16)))
    for name, N in (('gen_vae1', 1), ('gen_vae1024', 1024)):
        eng, seeds, wv = vae(N, 4, 2)
        out.append(compare(name, eng, seeds, wv, N * args.steps))
    print(json.dumps({'tool': 'temper_bench', 'steps': args.steps, 'reps': args.reps, **TEMPER, 'workloads': out}))
