"""Time of a filter stream against the one generate_smc call, in one run.

cl_vrnn at BASELINE configuration 3's shape (88 notes, 88 units, latent 2, 10 classes, history frames), 16 melodies x 64
particles, 8 teacher-forced seed frames and 128 harmonized frames under the top voice of a random source (note density
0.0443):

  one_call   engine.generate_smc over the 128 frames;
  stream     stream.FilterStream fed 16 frames at a time, then finish() (exact mode);
  lag16      the same with max_lag=16.

Each cell is a host clock around the whole call, ended by a device synchronise (the stream's own host reads included: they
are part of what a caller waits for).  The cells alternate; a warm-up of each, then --reps rounds, medians and spreads.
The share of clv_smc_commit: device events around every commit launch of the stream cell, summed, over the cell's time.
Prints one JSON line; --out FILE also writes it there.

    python tools/stream_filter_time.py [--reps 5] [--out profiles/stream_filter_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()


def main():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib, ops
    from clvae_amd.cl_vrnn.model import get_model
    from clvae_amd.harmonize import voice_constraints
    from clvae_amd.stream import FilterStream
    _lib.require_gpu()
    dev = torch.device('cuda:0')
    N, P, S, T, K, D, C = 16, 64, 8, 128, 16, 88, 10
    rng = np.random.default_rng(0)
    model, _ = get_model(256, D, 88, 2, 128, C, True, 'adam-wn', seed=0, device=dev)
    seeds = (rng.random((N, S, D)) < 0.0443).astype(np.float32)
    roll = voice_constraints(rng.random((N, T, D)) < 0.0443)
    w = np.eye(C, dtype=np.float32)[rng.integers(0, C, N)]
    d_seeds, d_w = torch.as_tensor(seeds, device=dev), torch.as_tensor(w, device=dev)
    commit_events, real_commit = [], ops.smc_commit

    def timed_commit(*a):
        e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e[0].record()
        real_commit(*a)
        e[1].record()
        commit_events.append(e)
    ops.smc_commit = timed_commit
    stats = {}

    def one_call():
        return model.engine.generate_smc(d_seeds, d_w, T, roll, P, seed=3).Xs[:, 0].cpu().numpy().astype(np.float64)

    def stream(max_lag=None):
        s = FilterStream(model, seeds, w, P, seed=3, max_lag=max_lag)
        for a in range(0, T, K):
            s.advance(roll[:, a:a + K])
        before = np.array([len(e) for e in s.emitted])
        s.finish()
        stats['lag16' if max_lag else 'stream'] = dict(emitted_before_finish=before.tolist(), collapses=s.collapses.tolist())
        return np.stack(s.emitted)

    cells = dict(one_call=one_call, stream=stream, lag16=lambda: stream(16))

    def timed(f):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t), out

    outs = {k: timed(f)[1] for k, f in cells.items()}           # warm-up
    times, share = {k: [] for k in cells}, []
    for _ in range(args.reps):                                  # alternating
        for k, f in cells.items():
            del commit_events[:]
            times[k].append(timed(f)[0])
            if k == 'stream':
                share.append(sum(a.elapsed_time(b) for a, b in commit_events) / times[k][-1])
    res = dict(tool='stream_filter_time', N=N, P=P, seed_frames=S, frames=T, chunk=K, reps=args.reps,
               stream_equals_one_call=bool(np.array_equal(outs['stream'], outs['one_call'])), **stats)
    for k, v in times.items():
        res[k + '_ms'] = round(float(np.median(v)), 3)
        res[k + '_spread_pct'] = round(float(100 * (max(v) - min(v)) / np.median(v)), 1)
    res['commit_share_of_stream_pct'] = round(float(100 * np.median(share)), 3)
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + "\n")


main()
