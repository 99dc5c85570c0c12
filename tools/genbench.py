import argparse, os, sys, time, numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import clvae_amd
from clvae_amd.engine import VrnnEngine
from clvae_amd.harmonize import FREE
from clvae_amd.initializers import init_weights
ap = argparse.ArgumentParser()
ap.add_argument('--clamped', action='store_true', help='time clamped against unclamped generation (persistent kernel), '
                'alternating in this process; the constraint roll clamps ~30%% of the notes')
ap.add_argument('--steps', type=int, default=2000)
ap.add_argument('--reps', type=int, default=5, help='--clamped: alternating pairs per shape')
ap.add_argument('--shapes', default='', help='N:L,N:L,... (default: all six, or 1:2,1024:2,1:32,1024:32 with --clamped)')
args = ap.parse_args()
dev = torch.device('cuda:0')
if args.shapes:
    shapes = [tuple(int(v) for v in s.split(':')) for s in args.shapes.split(',')]
else:
    shapes = ((1, 2), (1024, 2), (1, 32), (1024, 32)) if args.clamped else ((1, 2), (256, 2), (1024, 2), (1, 32), (256, 32), (1024, 32))
# --clamped: both gate activations (each compiles to kernel instances of its own); otherwise hard_sigmoid as before
gates = ('hard_sigmoid', 'sigmoid') if args.clamped else ('hard_sigmoid',)
for (N, L), gate in [(s, g) for s in shapes for g in gates]:
    cfg = dict(D=88, H=88, L=L, T=16, C=10, use_x_prev=True, class_weight=1.0, kl_weight=1.0, w_kl_weight=1.0, w_log_var_prior=0.0, gate_act=gate)
    eng = VrnnEngine(cfg, 1, dev)
    wts = init_weights(eng.P.logical, cfg, seed=0)
    wts['X_decoded_mean/bias'] = np.full_like(wts['X_decoded_mean/bias'], -3.07)   # logit(0.0443): piano-roll note density
    eng.P.set_weights(wts)
    rng = np.random.default_rng(0)
    seeds = torch.as_tensor((rng.random((N, 16, 88)) < 0.0443).astype(np.float32), device=dev)
    wv = torch.as_tensor(np.eye(10, dtype=np.float32)[rng.integers(0, 10, N)], device=dev)
    if args.clamped:
        steps = args.steps
        r = rng.random((N, steps, 88))
        roll = np.where(r < 0.3, (r < 0.02).astype(np.uint8), np.uint8(FREE)).astype(np.uint8)
        clamp = torch.as_tensor(roll, device=dev)
        t = {False: [], True: []}
        eng.generate(seeds, wv, 8, seed=1); eng.generate(seeds, wv, steps, seed=1, clamp=clamp); torch.cuda.synchronize()
        for rep in range(args.reps):
            for cl in ((False, True) if rep % 2 == 0 else (True, False)):
                t0 = time.perf_counter()
                eng.generate(seeds, wv, steps, seed=2, clamp=clamp if cl else None)
                torch.cuda.synchronize()
                t[cl].append(time.perf_counter() - t0)
        us = {k: 1e6 * np.median(v) / (steps + 16) for k, v in t.items()}
        print("N=%d L=%d %s: unclamped %.3f us/frame, clamped %.3f us/frame (%+.2f %%), medians of %d alternating runs"
              % (N, L, gate, us[False], us[True], 100 * (us[True] / us[False] - 1), args.reps))
        continue
    for persistent in (True, True, True, False):
        steps = args.steps if persistent else 300
        eng.generate(seeds, wv, 8, seed=1, persistent=persistent); torch.cuda.synchronize()
        t0 = time.perf_counter(); out = eng.generate(seeds, wv, steps, seed=2, persistent=persistent); torch.cuda.synchronize(); dt = time.perf_counter() - t0
        print("N=%d L=%d persistent=%s: %.3f us/frame, %.0f frames/s, density %.3f" % (N, L, persistent, 1e6 * dt / (steps + 16), N * (steps + 16) / dt, float(out.mean())))
