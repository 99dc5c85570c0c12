"""Time of the roll statistics audit against the same tables formed with torch ops on the device.

Two workloads: the training songs of the JSB Chorales_all data set as the test suite stores it (tests/golden, 209 songs of
uneven length), and a [1024, 4096, 88] uint8 roll that lies on the device (note density 0.0443, every fifth frame repeats
the one before it so that notes last).  Each is profiled once through clv_roll_stats (a memset and one launch: what
stats.profile runs) and once with torch on the same device tensors: sums for pitch and degree, scatter-adds for voices,
change, the outer voices' steps and the span, the diagonals of x^T x per piece for the intervals, and the note lengths from
the sorted onsets and ends (torch.nonzero).  The torch route takes pieces of one length per call, so the songs go through it
one by one -- what a user without the kernel would write.  Both routes are compared first, every section in exact equality
(the run stops if they differ), then alternate: a warm-up of both, --reps runs each, device events around the device work;
for the songs also the wall time of one stats.profile call from host arrays (packing and copies included).  Reporting only:
prints one JSON line; --out FILE also writes it there.

    python tools/stats_time.py [--pieces 1024] [--frames 4096] [--reps 5] [--out profiles/stats_time.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOTE_DENSITY = 0.0443

ap = argparse.ArgumentParser()
ap.add_argument('--pieces', type=int, default=1024)
ap.add_argument('--frames', type=int, default=4096)
ap.add_argument('--max_duration', type=int, default=32)
ap.add_argument('--chunk', type=int, default=64, help='pieces per call of the torch route on the device roll')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()


def main():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib, ops, stats
    from clvae_amd.keytrack import split_songs
    from helpers import write_jsb_pickle
    _lib.require_gpu()
    dev = torch.device('cuda:0')
    D, Lmax, low = 88, args.max_duration, 21
    V, C, M = stats.VOICES, stats.CHANGE, stats.STEP
    S = ops.roll_stats_columns(D, Lmax)

    def kernel_route(roll, off, tonic, table):
        ops.roll_stats(off.numel() - 1, D, Lmax, low, roll.shape[0], roll, off, tonic, table)

    def counts(idx, n, bins, weight=None):
        """[n, bins]: per row the number of entries of idx [n, k] per bin (entries with weight 0 left out)"""
        out = torch.zeros(n, bins, dtype=torch.int64, device=dev)
        if idx.shape[1]:
            out.scatter_add_(1, idx, torch.ones_like(idx) if weight is None else weight.to(torch.int64))
        return out

    def torch_route(x, tonic):
        """the table [n, S] of a block x [n, P, D] (uint8, non-zero: the note sounds) with torch ops"""
        n, P, _ = x.shape
        b = x != 0
        i64 = b.to(torch.int64)
        pitch = i64.sum(1)
        deg_of = (torch.arange(D, device=dev)[None, :] + low - tonic.clamp(min=0).to(torch.int64)[:, None]) % 12
        degree = torch.zeros(n, 12, dtype=torch.int64, device=dev).scatter_add_(1, deg_of, pitch)
        nn = i64.sum(2)
        voices = counts(nn.clamp(max=V), n, V + 1)
        f = b.to(torch.float32)
        G = f.transpose(1, 2) @ f                          # [n, D, D]: frames in which notes d and e both sound (< 2^24: exact)
        interval = torch.zeros(n, D, dtype=torch.int64, device=dev)
        for k in range(1, D):
            interval[:, k] = G.diagonal(offset=k, dim1=1, dim2=2).sum(-1).to(torch.int64)
        bt = b.transpose(1, 2)                             # [n, D, P]: a note's frames are contiguous in the sorted index
        pad = torch.zeros(n, D, 1, dtype=torch.bool, device=dev)
        starts = torch.nonzero(bt & ~torch.cat([pad, bt[:, :, :-1]], 2))
        ends = torch.nonzero(bt & ~torch.cat([bt[:, :, 1:], pad], 2))
        length = ends[:, 2] - starts[:, 2] + 1
        duration = torch.bincount(starts[:, 0] * Lmax + length.clamp(max=Lmax) - 1, minlength=n * Lmax).view(n, Lmax)
        change = counts((b[:, 1:] != b[:, :-1]).sum(2).clamp(max=C), n, C + 1)
        some = nn > 0
        ar = torch.arange(D, device=dev)
        hi = torch.where(b, ar, torch.full_like(ar, -1)).amax(2)
        lo = torch.where(b, ar, torch.full_like(ar, D)).amin(2)
        both = some[:, 1:] & some[:, :-1]
        top = counts((hi[:, 1:] - hi[:, :-1]).clamp(-M, M) + M, n, 2 * M + 1, both)
        bottom = counts((lo[:, 1:] - lo[:, :-1]).clamp(-M, M) + M, n, 2 * M + 1, both)
        span = counts((hi - lo).clamp(min=0), n, D, some)
        return torch.cat([pitch, degree, voices, interval, duration, change, top, bottom, span], 1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def measure(name, kernel, torch_fn, res):
        got, want = kernel(), torch_fn()                   # both routes agree before either is timed (also the warm-up)
        torch.cuda.synchronize()
        res[name + '_routes_agree'] = bool(torch.equal(got, want))
        if not res[name + '_routes_agree']:
            at, bad = 0, []
            for sec, nb in stats.section_bins(D, Lmax).items():
                if not torch.equal(got[:, at:at + nb], want[:, at:at + nb]):
                    bad.append(sec)
                at += nb
            raise SystemExit("the two routes disagree on %s in %s: %s" % (name, ", ".join(bad), json.dumps(res)))
        times = dict(kernel=[], torch=[])
        for _ in range(args.reps):                         # alternating
            times['kernel'].append(timed(kernel))
            times['torch'].append(timed(torch_fn))
        for k, v in times.items():
            res['%s_%s_ms' % (name, k)] = float(np.median(v))
            res['%s_%s_spread_pct' % (name, k)] = float(100 * (max(v) - min(v)) / np.median(v))
        res[name + '_torch_over_kernel'] = res[name + '_torch_ms'] / res[name + '_kernel_ms']

    res = dict(tool='stats_time', width=D, max_duration=Lmax, columns=S, reps=args.reps, torch_chunk=args.chunk)

    # ---- the training songs of JSB Chorales_all ----
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        songs, keys, key_map = split_songs(write_jsb_pickle('all', os.path.join(tmp, 'jsb.pickle')), 'train')
    tonics = [stats.tonic_of(key_map, k) for k in keys]
    lengths = [s.shape[0] for s in songs]
    s_roll = torch.as_tensor(np.concatenate(songs, 0), device=dev)
    s_off = torch.as_tensor(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), device=dev)
    s_ton = torch.as_tensor(np.asarray(tonics, np.int32), device=dev)
    s_table = torch.empty(len(songs), S, dtype=torch.int64, device=dev)
    s_blocks = [s_roll[a:a + p][None] for a, p in zip(np.cumsum([0] + lengths[:-1]), lengths)]

    def songs_kernel():
        kernel_route(s_roll, s_off, s_ton, s_table)
        return s_table

    def songs_torch():
        return torch.cat([torch_route(x, s_ton[n:n + 1]) for n, x in enumerate(s_blocks)], 0)

    res.update(songs=len(songs), songs_frames=int(sum(lengths)))
    measure('songs', songs_kernel, songs_torch, res)
    walls = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        st = stats.profile(songs, tonics, max_duration=Lmax)
        walls.append(1e3 * (time.perf_counter() - t0))
    res['songs_profile_call_wall_ms'] = float(np.median(walls))
    res['songs_profile_equals_kernel'] = bool(np.array_equal(st.table, s_table.cpu().numpy()))

    # ---- a roll that lies on the device ----
    N, P = args.pieces, args.frames
    g = torch.Generator(device=dev)
    g.manual_seed(4321)
    roll = (torch.rand(N, P, D, device=dev, generator=g) < NOTE_DENSITY).to(torch.uint8)
    roll[:, 4::5] = roll[:, 3::5][:, :roll[:, 4::5].shape[1]]
    r_ton = (torch.arange(N, device=dev) % 13 - 1).to(torch.int32)
    r_off = torch.arange(N + 1, dtype=torch.int64, device=dev) * P
    r_table = torch.empty(N, S, dtype=torch.int64, device=dev)
    flat = roll.view(N * P, D)

    def roll_kernel():
        kernel_route(flat, r_off, r_ton, r_table)
        return r_table

    def roll_torch():
        return torch.cat([torch_route(roll[a:a + args.chunk], r_ton[a:a + args.chunk]) for a in range(0, N, args.chunk)], 0)

    res.update(roll_pieces=N, roll_frames=P)
    measure('roll', roll_kernel, roll_torch, res)
    res['roll_kernel_frames_per_s'] = N * P / (1e-3 * res['roll_kernel_ms'])
    res['roll_kernel_roll_GB_per_s'] = N * P * D / (1e6 * res['roll_kernel_ms'])
    t0 = time.perf_counter()
    st = stats.profile(roll, r_ton.tolist(), max_duration=Lmax)
    res['roll_profile_call_wall_ms'] = 1e3 * (time.perf_counter() - t0)
    res['roll_profile_equals_kernel'] = bool(np.array_equal(st.table, r_table.cpu().numpy()))
    line = json.dumps(res, sort_keys=True)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + "\n")


main()
