"""Cost of decoding a given latent path against generation under the prior.

For both families at their default shapes (cl_vrnn: latent 2, 10 classes, 88 units, use_x_prev; cl_vae: latent 4, 2 classes,
use_x_prev) and N = 1 and N = 1024 sequences of --frames frames: decoding on the persistent kernel (the ZG instances: no
encoder cell, no latent head), decoding on the frame chain, and generate(persistent=True, z_prior=True) with S = 0 / one seed
frame at the same N and length (the yardstick: the cheapest loop the project had).  Every configuration runs in a fresh
process under its own time limit (a failing one ends the run); a warm-up, then the median of --reps runs.  Prints one JSON
line; --out FILE also writes a table.

    python tools/latent_path_bench.py [--frames 256] [--reps 7] [--out profiles/latent_bench.txt]

--one FAMILY N ROUTE runs a single configuration in this process (ROUTE: decode_persistent, decode_chain, generate, or
encode: vary with its latents stored), also for a kernel trace with statistics in a run of its own:

    rocprofv3 --kernel-trace --stats -d DIR -o p --output-format csv -- python tools/latent_path_bench.py --one cl_vrnn 1024 decode_persistent
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {'cl_vrnn': dict(L=2, C=10), 'cl_vae': dict(L=4, C=2)}
ROUTES = ('decode_persistent', 'decode_chain', 'generate')
NOTE_DENSITY = 0.0443

ap = argparse.ArgumentParser()
ap.add_argument('--frames', type=int, default=256)
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--limit', type=int, default=120, help='seconds allowed to one configuration')
ap.add_argument('--out', default='')
ap.add_argument('--one', nargs=3, metavar=('FAMILY', 'N', 'ROUTE'))
args = ap.parse_args()


def one(family, N, route):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import clvae_amd  # noqa: F401
    from clvae_amd.engine import VaeEngine, VrnnEngine
    from clvae_amd.initializers import init_weights
    dev = torch.device('cuda:0')
    L, C, T = FAMILIES[family]['L'], FAMILIES[family]['C'], args.frames
    base = dict(D=88, H=88, L=L, C=C, use_x_prev=True, class_weight=1.0, kl_weight=1.0, w_kl_weight=1.0, w_log_var_prior=0.0)
    if family == 'cl_vrnn':
        cfg = dict(base, T=16, gate_act='hard_sigmoid')
        eng, head = VrnnEngine(cfg, 1, dev), 'X_decoded_mean/bias'
    else:
        cfg = dict(base, Hc=88)
        eng, head = VaeEngine(cfg, N, dev), 'x_decoded_mean/bias'
    wts = init_weights(eng.P.logical, cfg, seed=0)
    wts[head] = np.full_like(wts[head], float(np.log(NOTE_DENSITY / (1 - NOTE_DENSITY))))        # piano-roll densities
    eng.P.set_weights(wts)
    rng = np.random.default_rng(1234)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
    sources = t(rng.random((N, T, 88)) < NOTE_DENSITY)
    x0 = t(rng.random((N, 88)) < NOTE_DENSITY)
    k = rng.integers(0, C, N)
    w_enc, w_dec = t(np.eye(C)[k]), t(np.eye(C)[(k + 1) % C])
    z = t(rng.standard_normal((N, T, L)))
    if route == 'generate':
        seed_frames = torch.zeros(N, 0, 88, device=dev) if family == 'cl_vrnn' else x0
        run = lambda: eng.generate(seed_frames, w_enc, T, seed=2, z_prior=True)
    elif route == 'encode':
        zout = torch.zeros(3, N, T, L, device=dev)
        run = lambda: eng.vary(sources, w_enc, w_dec, x0=x0, seed=2, zout=zout)
    else:
        run = lambda: eng.decode_latents(z, w_dec, x0=x0, seed=2, persistent=route == 'decode_persistent')
    density = float(run().mean())
    torch.cuda.synchronize()
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    med = float(np.median(times))
    print(json.dumps({'family': family, 'N': N, 'route': route, 'frames': T, 'reps': args.reps, 'median_ms': 1e3 * med,
                      'us_per_frame': 1e6 * med / T, 'frames_per_s': N * T / med, 'note_density': density,
                      'spread_pct': 100 * (max(times) - min(times)) / med, 'all_ms': [1e3 * v for v in times]}))


def drive():
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5")
    rows = []
    for family in FAMILIES:
        for N in (1, 1024):
            for route in ROUTES:
                cmd = ['timeout', '-k', '10', str(args.limit), sys.executable, os.path.abspath(__file__), '--one', family, str(N),
                       route, '--frames', str(args.frames), '--reps', str(args.reps)]
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
                if r.returncode != 0:       # a fault, an abort or the time limit: nothing more is started on the device
                    raise SystemExit("%s N=%d %s ended with status %d" % (family, N, route, r.returncode))
                rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    by = {(r['family'], r['N'], r['route']): r for r in rows}
    cases = []
    for family in FAMILIES:
        for N in (1, 1024):
            p, c, g = (by[family, N, route] for route in ROUTES)
            cases.append({'family': family, 'N': N, 'frames': args.frames,
                          'decode_persistent_us_per_frame': p['us_per_frame'], 'decode_chain_us_per_frame': c['us_per_frame'],
                          'generate_us_per_frame': g['us_per_frame'], 'decode_persistent_frames_per_s': p['frames_per_s'],
                          'decode_chain_frames_per_s': c['frames_per_s'], 'generate_frames_per_s': g['frames_per_s'],
                          'persistent_over_generate': p['median_ms'] / g['median_ms'],
                          'chain_over_persistent': c['median_ms'] / p['median_ms'],
                          'generate_spread_pct': g['spread_pct'], 'decode_persistent_spread_pct': p['spread_pct'],
                          'note_density': {route: by[family, N, route]['note_density'] for route in ROUTES}})
    print(json.dumps({'tool': 'latent_path_bench', 'frames': args.frames, 'reps': args.reps, 'cases': cases}))
    if args.out:
        with open(args.out, 'w') as f:
            f.write("decoding a latent path against generation under the prior: %d frames, median of %d runs after a warm-up, a process per cell\n"
                    % (args.frames, args.reps))
            f.write("%-8s %5s | %-28s | %-28s | %-28s | %-10s\n" % ('family', 'N', 'decode persistent us/frame (fr/s)',
                                                                  'decode chain us/frame (fr/s)', 'generate us/frame (fr/s)',
                                                                  'dec/gen'))
            for c in cases:
                cell = lambda k: "%10.2f (%12.0f)" % (c[k + '_us_per_frame'], c[k + '_frames_per_s'])
                f.write("%-8s %5d | %-28s | %-28s | %-28s | %.3f (yardstick spread %.1f %%)\n"
                        % (c['family'], c['N'], cell('decode_persistent'), cell('decode_chain'), cell('generate'),
                           c['persistent_over_generate'], c['generate_spread_pct']))
            f.write("note density of the frames: %s\n" % json.dumps({"%s/%d" % (c['family'], c['N']): c['note_density']
                                                                     for c in cases}))


if args.one:
    one(args.one[0], int(args.one[1]), args.one[2])
else:
    drive()
