"""What gradient clipping costs a training step: ms per step of the captured single-GPU step of a workload
  plain     : no clipping (clv_adam_wn_step)
  clipnorm  : clipnorm set (two norm launches and one more read of the gradient buffer, then clv_adam_wn_step_clipped)
  all       : clipnorm, clipvalue and decay (clipvalue takes the five-launch Adam-WN for the tall matrix)
alternating, --reps rounds of --steps steps; the last step's norm and scale next to it.  clipnorm is set far below the
gradient's norm so that the clip is taken, though what the kernels do does not depend on it.
Run on the GPU box: python tools/clip_overhead.py --workload cfg3 ; python tools/clip_overhead.py --workload cfg5"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=300)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--workload', default='cfg3')
    args = ap.parse_args()
    import torch
    import bench
    import clvae_amd  # noqa: F401
    from clvae_amd.trainer import TrainStep
    dev = torch.device('cuda:0')
    torch.cuda.set_device(0)
    w = bench.WORKLOADS[args.workload]
    B = w['B']
    modes = {'plain': {}, 'clipnorm': dict(clipnorm=1e-3), 'all': dict(clipnorm=1e-3, clipvalue=1e-5, decay=1e-4)}
    steps = {}
    for name, clip in modes.items():
        eng, cfg = bench.make_engine(w, dev)
        X_all, Xp_all, w_all = bench.synthetic_windows(w, 4 * B, 1234, dev)
        ts = TrainStep(eng, seed=1234, use_graph=True, **clip)
        ts.bind_batches(X_all, Xp_all, w_all, idx=None, period=4, stride=B)
        for _ in range(5):
            ts.step()
        torch.cuda.synchronize()
        steps[name] = ts
    for r in range(args.reps):
        line = []
        for name, ts in steps.items():
            for _ in range(20):
                ts.step()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                ts.step()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            st = ts.grad_stats.cpu().numpy()
            line.append("%s %.4f ms (norm %.4g scale %.4g)" % (name, 1e3 * dt / args.steps, st[0], st[1]))
        print("%s round %d: " % (args.workload, r) + " | ".join(line), flush=True)


if __name__ == '__main__':
    main()
