"""Time of the novelty audit against the route the project had for the same question.

1024 query pieces x 32 frames against a corpus of 256 pieces x 256 frames (note density 0.0443), windows of 16 frames at
hop 1, without transposition (S = 0) and with up to 6 semitones (S = 6): every query window against every corpus window,
once through clv_roll_nearest (packing, the sliding-sum search, unpacking: what novelty.nearest launches), once with torch
on the same device tensors: per shift the frame distances |q| + |c| - 2 q.c as a matrix product over a chunk of query
pieces, 16 shifted slices added for the window distances, a masked minimum per query window, the shifts folded in rank
order.  Both routes are checked against each other first (dist and shift exactly; cframe where torch.min names the first
minimum), then alternate: a warm-up of both, --reps runs each, device events around the device work.  Prints one JSON line;
--out FILE also writes it there.

    python tools/novelty_time.py [--queries 1024] [--corpus 256] [--reps 5] [--out profiles/novelty_time.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTE_DENSITY = 0.0443

ap = argparse.ArgumentParser()
ap.add_argument('--queries', type=int, default=1024)
ap.add_argument('--query_frames', type=int, default=32)
ap.add_argument('--corpus', type=int, default=256)
ap.add_argument('--corpus_frames', type=int, default=256)
ap.add_argument('--window', type=int, default=16)
ap.add_argument('--chunk', type=int, default=32, help='query pieces per matrix product of the torch route')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()


def main():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib, ops
    _lib.require_gpu()
    dev = torch.device('cuda:0')
    Nq, P, Nc, L, W, D = args.queries, args.query_frames, args.corpus, args.corpus_frames, args.window, 88
    rng = np.random.default_rng(4321)
    q = (rng.random((Nq, P, D)) < NOTE_DENSITY).astype(np.uint8)
    c = (rng.random((Nc, L, D)) < NOTE_DENSITY).astype(np.uint8)
    for n in range(0, Nq, 8):                              # every eighth query holds a corpus passage, some transposed
        m, b, s = int(rng.integers(Nc)), int(rng.integers(L - P + 1)), int(rng.integers(-3, 4))
        src = c[m, b:b + P]
        q[n] = 0
        if s >= 0:
            q[n][:, s:] = src[:, :D - s]
        else:
            q[n][:, :D + s] = src[:, -s:]
    J, B = P - W + 1, L - W + 1
    Wq = Nq * J
    q_roll, c_roll = torch.as_tensor(q.reshape(Nq * P, D), device=dev), torch.as_tensor(c.reshape(Nc * L, D), device=dev)
    q_off = torch.arange(Nq + 1, dtype=torch.int64, device=dev) * P
    c_off = torch.arange(Nc + 1, dtype=torch.int64, device=dev) * L
    w_off = torch.arange(Nq + 1, dtype=torch.int64, device=dev) * J
    dist = torch.empty(Wq, dtype=torch.int32, device=dev)
    shift = torch.empty(Wq, dtype=torch.int32, device=dev)
    cframe = torch.empty(Wq, dtype=torch.int64, device=dev)
    ws = torch.empty(ops.roll_nearest_workspace_bytes(Nq * P, Nc * L, Wq), dtype=torch.uint8, device=dev)

    def kernel(S):
        ops.roll_nearest(Nq, Nc, W, 1, S, D, Nq * P, Nc * L, Wq, q_roll, q_off, c_roll, c_off, w_off, None, dist, shift, cframe,
                         workspace=ws)

    # ---- the torch route on the same tensors ----
    qf, cf = q_roll.to(torch.float32).view(Nq, P, D), c_roll.to(torch.float32)
    csum = cf.sum(1)
    t_dist = torch.empty(Nq, J, dtype=torch.int32, device=dev)
    t_shift = torch.empty(Nq, J, dtype=torch.int32, device=dev)
    t_g = torch.empty(Nq, J, dtype=torch.int64, device=dev)
    # the shifts a window allows, from the lowest and highest sounding note of the window (host side, not timed)
    on = q.any(axis=2)
    lo = np.where(on, q.argmax(axis=2), D)
    hi = np.where(on, D - 1 - q[:, :, ::-1].argmax(axis=2), -1)
    wlo = np.stack([lo[:, a:a + W].min(1) for a in range(J)], 1)
    whi = np.stack([hi[:, a:a + W].max(1) for a in range(J)], 1)
    BIG = 1 << 24

    def torch_route(S):
        order = sorted(range(-S, S + 1), key=lambda s: 0 if s == 0 else (-2 * s - 1 if s < 0 else 2 * s))
        ok = {s: torch.as_tensor((wlo + s >= 0) & (whi + s < D), device=dev) for s in order}
        for n0 in range(0, Nq, args.chunk):
            n1 = min(Nq, n0 + args.chunk)
            best = torch.full((n1 - n0, J), BIG, dtype=torch.float32, device=dev)
            bs = torch.zeros(n1 - n0, J, dtype=torch.int32, device=dev)
            bg = torch.full((n1 - n0, J), -1, dtype=torch.int64, device=dev)
            for s in order:
                Q = torch.zeros(n1 - n0, P, D, dtype=torch.float32, device=dev)
                if s >= 0:
                    Q[:, :, s:] = qf[n0:n1, :, :D - s]
                else:
                    Q[:, :, :D + s] = qf[n0:n1, :, -s:]
                F = (Q.sum(2)[:, :, None] + csum[None, None, :] - 2.0 * (Q.view(-1, D) @ cf.t()).view(n1 - n0, P, Nc * L))
                F = F.view(n1 - n0, P, Nc, L)
                Wd = F[:, 0:J, :, 0:B].clone()
                for t in range(1, W):
                    Wd += F[:, t:t + J, :, t:t + B]
                v, i = Wd.view(n1 - n0, J, Nc * B).min(dim=2)
                v = torch.where(ok[s][n0:n1], v, torch.full_like(v, BIG))
                take = v < best
                best = torch.where(take, v, best)
                bs = torch.where(take, torch.full_like(bs, s), bs)
                bg = torch.where(take, (i // B) * L + i % B, bg)
            t_dist[n0:n1], t_shift[n0:n1], t_g[n0:n1] = best.to(torch.int32), bs, bg

    def timed(fn, S):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(S)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    res = dict(tool='novelty_time', queries=Nq, query_frames=P, corpus=Nc, corpus_frames=L, window=W, hop=1, reps=args.reps,
               torch_chunk=args.chunk, query_windows=Wq, corpus_windows=Nc * B)
    for S in (0, 6):
        kernel(S)                                          # both routes agree before either is timed (also the warm-up)
        torch_route(S)
        torch.cuda.synchronize()
        same_d = bool((dist.view(Nq, J) == t_dist).all())
        same_s = bool((shift.view(Nq, J) == t_shift).all())
        res['S%d_routes_agree_on_dist_and_shift' % S] = same_d and same_s
        res['S%d_cframe_equal_share' % S] = float((cframe.view(Nq, J) == t_g).float().mean())
        res['S%d_windows_at_dist_0' % S] = int((dist == 0).sum())
        if not (same_d and same_s):
            raise SystemExit("the two routes disagree at S = %d: %s" % (S, json.dumps(res)))
        times = dict(kernel=[], torch=[])
        for _ in range(args.reps):                         # alternating
            times['kernel'].append(timed(kernel, S))
            times['torch'].append(timed(torch_route, S))
        pairs = float(Wq) * Nc * B * (2 * S + 1)           # (query window, corpus window, shift) triples
        for k, v in times.items():
            res['S%d_%s_ms' % (S, k)] = float(np.median(v))
            res['S%d_%s_spread_pct' % (S, k)] = float(100 * (max(v) - min(v)) / np.median(v))
        res['S%d_window_pairs' % S] = pairs
        res['S%d_kernel_window_pairs_per_s' % S] = pairs / (1e-3 * res['S%d_kernel_ms' % S])
        res['S%d_kernel_frame_pairs_per_s' % S] = pairs * W / (1e-3 * res['S%d_kernel_ms' % S])
        res['S%d_torch_over_kernel' % S] = res['S%d_torch_ms' % S] / res['S%d_kernel_ms' % S]
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + "\n")


main()
