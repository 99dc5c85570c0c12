"""Importance-weighted log-likelihood of held-out windows, for both engines.

The reference scores nothing but the training objective; the standard figure for a polyphonic-music model is the test-set
log-likelihood per time step, estimated by importance sampling with the model's own encoder as the proposal (the K-sample
IWAE estimate).  Sample k of a window draws eps_W, eps_Z, runs the unchanged inference forward pass (no dropout, no
gradients) and hands what the pass leaves -- rownll, zargs, wargs and the eps -- to csrc/iw_eval.hip, which forms the
sample's log weight and folds it into a running log-sum-exp per window.  The K samples of a chunk of windows are replays
of one captured graph; a device counter advanced by the accumulate launch keys the draw of the next replay.

Noise: the Philox stream pair IW_STREAM_W / IW_STREAM_Z of trainer.py, step = k, first index from the GLOBAL window index,
so the estimate does not depend on the batch size, the chunking or the number of ranks.

Nothing of the training state changes: the estimate stages its windows through a TrainStep of its own (the model's step,
its bound batches and its graphs are not touched), uses its own sample counter (not `iterations`), and puts back the
engine buffers a forward pass shares with training (the loss means, the [Xp | Z] history columns, the note lists) and the
engine's per-data-set flags.
"""
import math

import numpy as np
import torch
import torch.distributed as dist

from . import ops
from .parallel import eps_first_index
from .trainer import IW_STREAM_W, IW_STREAM_Z, TrainStep


def _dp():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def _iw_step(model):
    """The estimate's own TrainStep (staging buffers and eps), kept on the model between calls."""
    ts = getattr(model, '_iw_ts', None)
    if ts is None or ts.eng is not model.engine:
        ts = TrainStep(model.engine, seed=model.seed, rank=0, world=1, optimizer=model.optimizer.name,
                       lr=model.optimizer.lr, use_graph=False)
        model._iw_ts = ts
    return ts


class _SharedEngineState:
    """What a forward pass writes into the engine that a training step may still read: saved on entry, put back on exit."""

    FLAGS = ('frames_exact_bf16', 'notes_valid')
    BUFFERS = ('scal', 'XZ', 'notes_enc', 'notes_dec')      # (cl_vae has no XZ; the note lists exist only with fuse_notes)

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        e = self.eng
        self.flags = {f: getattr(e, f) for f in self.FLAGS}
        self.bufs = {b: t.clone() for b, t in ((b, getattr(e, b, None)) for b in self.BUFFERS) if t is not None}
        return self

    def __exit__(self, *exc):
        e = self.eng
        for f, v in self.flags.items():
            setattr(e, f, v)
        for b, v in self.bufs.items():
            getattr(e, b).copy_(v)
        return False


def estimate_device(model, d_cur, d_hist, d_w, n, k=100, seed=0, d_target=None, use_graph=True):
    """Per-window (log_p, elbo, ess) as a float64 [3, n] device tensor for the n windows of the device-resident data set
    (the structures Model.fit stages: whole rows or DevWindows).  Chunks of the engine's batch, dealt round-robin to the
    ranks under torch.distributed and summed, so every rank returns the whole result."""
    eng = model.engine
    cfg, B, dev = eng.cfg, eng.B, eng.device
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1, got %d" % k)
    if n < 1:
        raise ValueError("no windows to score")
    T = cfg['T'] if 'T' in cfg else 1
    L, C1 = cfg['L'], cfg['C'] - 1
    prior = float(cfg['w_log_var_prior'])
    seed = int(seed)
    rank, world = _dp()
    ts = _iw_step(model)
    out = torch.zeros(3, n, dtype=torch.float64, device=dev)
    state = torch.empty(B, 4, dtype=torch.float64, device=dev)
    res = torch.empty(3, B, dtype=torch.float64, device=dev)
    k_dev = torch.zeros(1, dtype=torch.int32, device=dev)
    rows = torch.arange(B, dtype=torch.int64, device=dev)

    def draw(w0):
        fw, fz = eps_first_index(w0, C1), eps_first_index(w0, T * L)
        if C1 > 0:
            ops.philox_normal2(ts.eps_w, B * C1, IW_STREAM_W, fw, ts.eps_z, B * T * L, IW_STREAM_Z, fz, seed, 0, step_dev=k_dev)
        else:
            ops.philox_normal(ts.eps_z, B * T * L, seed, 0, IW_STREAM_Z, fz, step_dev=k_dev)

    def forward():
        eng.loss_and_grads(ts.X, ts.Xp, ts.w_true, ts.eps_w, ts.eps_z, need_grads=False, target=ts.Y)

    def sample(w0, nvalid):
        draw(w0)
        forward()
        ops.iw_accumulate(B, T, L, C1, eng.rownll, eng.zargs, ts.eps_z, eng.wargs, ts.eps_w, prior, nvalid, state, k_dev)

    graphs = []          # kept until the call's work is done: a graph is not destroyed under its pending replays
    with _SharedEngineState(eng):
        warm = False
        for j, w0 in enumerate(range(0, n, B)):
            if j % world != rank:
                continue
            nvalid = min(B, n - w0)
            # the last chunk is padded with copies of the last window; only rows < nvalid are scored
            ib = torch.clamp(rows + w0, max=n - 1)
            ts.gather_batch(d_cur, d_hist, d_w, ib, d_target=d_target)
            if use_graph and not warm:      # one eager pass sizes every workspace before anything is captured
                k_dev.zero_()
                draw(w0)
                forward()
                warm = True
            state[:, 0].fill_(-math.inf)
            state[:, 1:].zero_()
            k_dev.zero_()
            if use_graph:
                with ops.Graph() as g:
                    sample(w0, nvalid)
                for _ in range(k):
                    g.launch()
                graphs.append(g)
            else:
                for _ in range(k):
                    sample(w0, nvalid)
            ops.iw_finish(B, nvalid, k, state, res[0], res[1], res[2])
            out[:, w0:w0 + nvalid].copy_(res[:, :nvalid])
    if world > 1:
        dist.all_reduce(out)        # every window is written by exactly one rank, zeros elsewhere
    torch.cuda.current_stream(dev).synchronize()
    del graphs
    return out


def summarize(per_window, T, k, per_window_arrays=False):
    """The data-set figures of a per-window [3, n] result (means over windows; log_p / T per frame)."""
    a = per_window.detach().cpu().numpy().astype(np.float64)
    lp, el, es = a
    out = {'log_likelihood': float(lp.mean()), 'log_likelihood_per_frame': float(lp.mean() / T),
           'elbo': float(el.mean()), 'ess': float(es.mean()), 'n_windows': int(a.shape[1]), 'k': int(k)}
    if per_window_arrays:
        out['windows'] = {'log_p': lp, 'elbo': el, 'ess': es}
    return out
