"""Time of key tracking against the route the project had for the same windows.

256 pieces x 512 frames (note density 0.0443), hop 1, cl_vrnn's label head at T = 32: every window of every piece, once
through keytrack.track (clv_key_track_windows straight from the byte roll + clv_key_track_smooth), once the earlier way:
the windows materialised as float rows [rows, T * 88] on the device and pushed through VrnnGenerate.encode_w (two dense
GEMMs) in chunks of engine.B rows.  The two routes alternate; a warm-up of both, then --reps runs each, device events
around the device work (the windows launch, the smoothing launch, the earlier route with and without its gather) and a
host clock around the whole of track() (packing, copies to and from the device included).  Also compares the wargs of both
routes.  Prints one JSON line; --out FILE also writes it there.

    python tools/keytrack_time.py [--pieces 256] [--frames 512] [--reps 7] [--out profiles/keytrack_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTE_DENSITY = 0.0443

ap = argparse.ArgumentParser()
ap.add_argument('--pieces', type=int, default=256)
ap.add_argument('--frames', type=int, default=512)
ap.add_argument('--seq_length', type=int, default=32)
ap.add_argument('--classes', type=int, default=10)
ap.add_argument('--batch', type=int, default=1024, help='engine.B: rows per encode_w call of the earlier route')
ap.add_argument('--reps', type=int, default=7)
ap.add_argument('--out', default='')
args = ap.parse_args()


def main():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib, keytrack, ops
    from clvae_amd.cl_vrnn.model import get_model
    _lib.require_gpu()
    dev = torch.device('cuda:0')
    N, P, T, C, D = args.pieces, args.frames, args.seq_length, args.classes, 88
    model, _ = get_model(args.batch, D, 88, 2, T, C, True, 'adam-wn', seed=0, device=dev)
    eng = model.engine
    rng = np.random.default_rng(1234)
    pieces = (rng.random((N, P, D)) < NOTE_DENSITY).astype(np.uint8)
    J = P - T + 1
    rows = N * J

    # ---- the device work of track(), launch by launch ----
    roll = torch.as_tensor(pieces.reshape(N * P, D), device=dev)
    po = torch.arange(N + 1, dtype=torch.int64, device=dev) * P
    wo = torch.arange(N + 1, dtype=torch.int64, device=dev) * J
    wargs = torch.empty(rows, 2 * (C - 1), dtype=torch.float32, device=dev)
    logp = torch.empty(rows, C, dtype=torch.float32, device=dev)
    post = torch.empty(rows, C, dtype=torch.float64, device=dev)
    path = torch.empty(rows, dtype=torch.int32, device=dev)
    ev = torch.empty(N, dtype=torch.float64, device=dev)
    pp = torch.empty(N, C, dtype=torch.float64, device=dev)
    lt = torch.as_tensor(np.log(keytrack.sticky_transitions(C, 1, 64)), device=dev)
    Pm = eng.P
    head = [Pm.p(n) for n in ('hW/kernel', 'hW/bias', 'Wargs/kernel', 'Wargs/bias')]

    def windows():
        ops.key_track_windows(N, T, D, D, C, 1, 0, roll, po, wo, *head, 0, 0, wargs, logp)

    def smooth():
        ops.key_track_smooth(N, C, wo, logp, None, lt, 1.0 / T, post, path, ev, pp)

    # ---- the earlier route: float windows, materialised chunk by chunk, through encode_w ----
    roll_f = roll.to(torch.float32)
    starts = (torch.arange(N, device=dev)[:, None] * P + torch.arange(J, device=dev)[None, :]).reshape(-1)
    frame = torch.arange(T, device=dev)[None, :]
    old_wargs = torch.empty(rows, 2 * (C - 1), dtype=torch.float32, device=dev)
    B = eng.B

    def gather(r0, nb):
        return roll_f[starts[r0:r0 + nb, None] + frame].reshape(nb, T * D)

    def old_route():
        for r0 in range(0, rows, B):
            nb = min(B, rows - r0)
            eng.encode_w(gather(r0, nb), nb)
            old_wargs[r0:r0 + nb] = eng.wargs[:nb]

    X_one = gather(0, B)

    def old_gemms_only():
        for r0 in range(0, rows, B):
            eng.encode_w(X_one, min(B, rows - r0))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def track_wall():
        t0 = time.perf_counter()
        keytrack.track(model, pieces, hop=1)
        return 1e3 * (time.perf_counter() - t0)        # (track ends in copies to the host: the device work is done)

    cells = dict(windows_ms=lambda: timed(windows), smooth_ms=lambda: timed(smooth), old_route_ms=lambda: timed(old_route),
                 old_gemms_only_ms=lambda: timed(old_gemms_only), track_wall_ms=track_wall)
    for f in cells.values():            # warm-up of every shape
        f()
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in cells}
    for _ in range(args.reps):          # alternating
        for k, f in cells.items():
            times[k].append(f())
    diff = float((wargs - old_wargs).abs().max())
    res = dict(tool='keytrack_time', pieces=N, frames=P, seq_length=T, classes=C, hop=1, windows=rows, engine_B=B, reps=args.reps,
               wargs_max_abs_diff_between_routes=diff)
    for k, v in times.items():
        res[k] = float(np.median(v))
        res[k.replace('_ms', '_spread_pct')] = float(100 * (max(v) - min(v)) / np.median(v))
    res['windows_us_per_window'] = 1e3 * res['windows_ms'] / rows
    res['old_route_us_per_window'] = 1e3 * res['old_route_ms'] / rows
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + "\n")


main()
