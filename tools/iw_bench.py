"""Throughput of the importance-weighted likelihood (Model.log_likelihood) at the configuration-3 shape: cl_vrnn,
256 windows x 128 frames, latent 2, 10 classes, history frames on (the pair path).

  python tools/iw_bench.py [--windows 256] [-k 100] [--reps 3]          windows * samples / s, one JSON line
  python tools/iw_bench.py --rocprof DIR                                 the same under rocprofv3 --kernel-trace --stats
                                                                         (a child process), then each kernel's share of a
                                                                         sample pass from DIR/iw_kernel_stats.csv

Weights are the oracle's initialisation and the frames sparse random binary ones: the forward pass costs the same for any
values, so the number is the cost of the estimate on trained models too."""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(args):
    import torch
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    from clvae_amd.cl_vrnn.model import get_model
    _lib.require_gpu()
    dev = torch.device('cuda:0')
    B, T, L, C = 256, 128, 2, 10
    model, _ = get_model(B, 88, 88, L, T, C, True, 'adam', seed=0, device=dev)
    rng = np.random.default_rng(0)
    win = (rng.random((args.windows, T + 1, 88)) < 0.0443).astype(np.uint8)
    X, Xp = win[:, 1:], win[:, :-1]
    wt = np.eye(C)[rng.integers(0, C, args.windows)]
    x, y = [X, Xp], [X, wt, wt, X]
    model.log_likelihood(x, y, k=2, seed=1)            # warm-up: workspaces, first capture
    times = []
    for r in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = model.log_likelihood(x, y, k=args.k, seed=1)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    best = min(times)
    out = {'metric': 'iw_windows_samples_per_s', 'value': round(args.windows * args.k / best, 1),
           'config': 'cl_vrnn %d windows x %d frames, latent %d, %d classes, use_x_prev, K = %d, batch %d'
                     % (args.windows, T, L, C, args.k, B),
           'seconds': [round(t, 4) for t in times], 'ms_per_sample_pass': round(1e3 * best / args.k / -(-args.windows // B), 4),
           'log_likelihood_per_frame': res['log_likelihood_per_frame'], 'ess': res['ess']}
    print(json.dumps(out))
    return out


def profile(args):
    d = os.path.abspath(args.rocprof)
    os.makedirs(d, exist_ok=True)
    cmd = ['rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'iw', '--output-format', 'csv', '--',
           sys.executable, os.path.abspath(__file__), '--windows', str(args.windows), '-k', str(args.k), '--reps', '1']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.timeout)
    print(r.stdout.strip().splitlines()[-1] if r.stdout.strip() else '')
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-4000:])
        raise SystemExit(r.returncode)
    stats = [os.path.join(root, f) for root, _, files in os.walk(d) for f in files if f.endswith('kernel_stats.csv')]
    rows = list(csv.DictReader(open(stats[0])))
    acc = [x for x in rows if 'iw_accumulate' in x['Name']]
    passes = int(acc[0]['Calls'])                 # one accumulate launch per sample pass (warm-up + timed run)
    total = sum(float(x['TotalDurationNs']) for x in rows)
    print("sample passes profiled: %d" % passes)
    for x in sorted(rows, key=lambda x: -float(x['TotalDurationNs'])):
        per = float(x['TotalDurationNs']) / passes / 1e3
        print("%-64s calls %6s  avg %8.2f us  per pass %8.2f us  share %5.1f %%"
              % (x['Name'][:64], x['Calls'], float(x['AverageNs']) / 1e3, per, 100 * float(x['TotalDurationNs']) / total))
    print("accumulate kernel: %.2f us per pass, %.2f %% of the kernel time of a pass (%.1f us)"
          % (float(acc[0]['AverageNs']) / 1e3, 100 * float(acc[0]['TotalDurationNs']) / total, total / passes / 1e3))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--windows', type=int, default=256)
    ap.add_argument('-k', type=int, default=100)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rocprof', default='', help='profile a run under rocprofv3 into this directory')
    ap.add_argument('--timeout', type=int, default=600)
    a = ap.parse_args()
    profile(a) if a.rocprof else run(a)
