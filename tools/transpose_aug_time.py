"""Time of the transposition augmentation against the plain mini-batch assembly, in one run.

At BASELINE configuration 3 (256 windows x 128 frames, latent 2) and configuration 5 (1024 x 256, latent 32), cl_vrnn with
history frames, a uint8 frame store with one window per row of the data set (4 batches), note density 0.0443 in the notes
15..65 so that most shifts are allowed:

  launch   clv_gather_transposed against clv_gather_rows_multi on IDENTICAL segments (the step's own: what
           TrainStep._stage_bound passes, note lists and batch cursor included), device events around --launches launches;
  step     the captured training step with a TransposePlan bound against the step without one (which assembles its batch
           inside its first launch where it can), device events around --steps replays.

The cells alternate; a warm-up of each, then --reps rounds, medians and spreads.  Prints one JSON line; --out FILE also writes
it there.

    python tools/transpose_aug_time.py [--reps 7] [--out profiles/transpose_aug_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTE_DENSITY = 0.0443
SHAPES = {'cfg3': dict(B=256, T=128, L=2, C=10), 'cfg5': dict(B=1024, T=256, L=32, C=10)}
KEYS = {'A': 0, 'A-': 1, 'B-': 2, 'C': 3, 'D': 4, 'D-': 5, 'E': 6, 'E-': 7, 'F': 8, 'G': 9}      # JSB Chorales_all

ap = argparse.ArgumentParser()
ap.add_argument('--semitones', type=int, default=6)
ap.add_argument('--launches', type=int, default=2000, help='launches inside one timed window of the launch cells')
ap.add_argument('--steps', type=int, default=100, help='replays inside one timed window of the step cells')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--only', default='', help='cfg3 or cfg5')
ap.add_argument('--out', default='')
args = ap.parse_args()


def main():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib, ops
    from clvae_amd.augment import TransposePlan
    from clvae_amd.cl_vrnn.model import get_model
    from clvae_amd.trainer import DevWindows, TrainStep
    from clvae_amd.utils.pianoroll import Windows
    _lib.require_gpu()
    dev = torch.device('cuda:0')
    D, K = 88, args.semitones
    res = dict(tool='transpose_aug_time', semitones=K, launches=args.launches, steps=args.steps, reps=args.reps)

    def timed(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / n                 # us per call

    for name, sh in SHAPES.items():
        if args.only and name != args.only:
            continue
        B, T, L, C = sh['B'], sh['T'], sh['L'], sh['C']
        rng = np.random.default_rng(B)
        n = 4 * B
        store = np.zeros((n + T + 1, D), np.uint8)
        store[:, 15:66] = rng.random((n + T + 1, 51)) < NOTE_DENSITY * D / 51
        starts = rng.permutation(n).astype(np.int64)
        lab = rng.integers(0, C, n)
        plan_h = TransposePlan.build([Windows(store, starts, 1, T), Windows(store, starts, 0, T)], lab, KEYS, semitones=K)
        plan = plan_h.to(dev)
        d_store = torch.as_tensor(store, device=dev)
        d_starts = torch.as_tensor(starts, device=dev)
        cur, hist = DevWindows(d_store, d_starts, 1), DevWindows(d_store, d_starts, 0)
        w = torch.as_tensor(np.eye(C, dtype=np.float32)[lab], device=dev)
        idx = torch.as_tensor(rng.permutation(n).astype(np.int64), device=dev)

        def step_of(augment):
            model, _ = get_model(B, D, 88, L, T, C, True, 'adam-wn', seed=0, device=dev)
            ts = TrainStep(model.engine, seed=1)
            ts.bind_batches(cur, hist, w, idx=idx, period=4, stride=B, augment=augment)
            for _ in range(4):                              # eager, capture, replays
                ts.step()
            torch.cuda.synchronize()
            return ts
        ts_aug, ts_plain = step_of(plan), step_of(None)

        # the launch alone, on the segments of the augmented step (the plain step may assemble inside its label launch)
        b = ts_aug._bound
        segs = ts_aug._segments(b['cur'], b['hist'], b['w'], None, bytes_out=ts_aug._f8)
        notes = ts_aug._note_outputs(b['cur'], b['hist'], len(segs))
        cursor = (ts_aug.eng.P.iterations, b['step0'], b['period'], b['stride'], b['offset'])

        def plain_launch():
            ops.gather_rows_multi(B, idx, segs, notes=notes, cursor=cursor)

        def aug_launch():
            ops.gather_transposed(B, idx, segs, plan.allowed, plan.class_map, K, D, 1, step_dev=ts_aug.eng.P.iterations,
                                  shift_out=ts_aug.shifts, label_seg=len(segs) - 1, notes=notes, cursor=cursor)

        cells = dict(gather_plain_us=lambda: timed(plain_launch, args.launches), gather_transposed_us=lambda: timed(aug_launch, args.launches),
                     step_plain_us=lambda: timed(ts_plain.step, args.steps), step_transposed_us=lambda: timed(ts_aug.step, args.steps))
        for f in cells.values():
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in cells}
        for _ in range(args.reps):                          # alternating
            for k, f in cells.items():
                times[k].append(f())
        out = dict(B=B, T=T, L=L, bytes_batch=ts_aug._f8 is not None, note_lists=notes is not None,
                   plain_step_assembles_in_its_first_launch=ts_plain._label_stage() is not None,
                   shifts_allowed_min=int(plan_h.counts().min()), shifts_allowed_max=int(plan_h.counts().max()))
        for k, v in times.items():
            out[k] = round(float(np.median(v)), 3)
            out[k.replace('_us', '_spread_pct')] = round(float(100 * (max(v) - min(v)) / np.median(v)), 1)
        out['launch_ratio'] = round(out['gather_transposed_us'] / out['gather_plain_us'], 3)
        out['step_extra_us'] = round(out['step_transposed_us'] - out['step_plain_us'], 3)
        res[name] = out
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + "\n")


main()
