"""-m gpu: transposition augmentation.  clv_gather_transposed (csrc/transpose_aug.hip) against the numpy reference
of tests/transpose_reference.py, bit for bit -- everything it computes is exact -- over sources, row lists, cursor positions,
output forms and segment sets; the frame edges; a launch split in two; then the captured TrainStep, Model.fit and train.py."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import transpose_reference as TR
from helpers import Bufs, make_synthetic_pickle
from oracle import clvae_oracle as O
from oracle import philox as OP

pytestmark = pytest.mark.gpu
D = 88
JSB_KEYS = {'A': 0, 'A-': 1, 'B-': 2, 'C': 3, 'D': 4, 'D-': 5, 'E': 6, 'E-': 7, 'F': 8, 'G': 9}


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def U8(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint8), device=dev)


def F(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def I64(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int64), device=dev)


def _problem(T, rows, K, C, seed):
    """A data set of N source rows in both forms (a frame store with a window table; whole rows), masks with every kind of word
    (empty, bits above 2K, single, full), a random class map with -1 and repeated targets, labels that are not one-hot."""
    rng = np.random.default_rng(seed)
    N = 3 * rows + 7                                            # cursor: period 3, stride rows, offset 2; row0 up to 3
    Fr = N + T + 9
    store = (rng.random((Fr, D)) < 0.08).astype(np.uint8)
    store[rng.integers(0, Fr, 6), rng.integers(0, D, 6)] = 255  # bytes are copied, not tested for being 1
    store[1, 0] = store[2, 87] = store[3, :] = 1
    table = rng.integers(0, Fr - T - 1, N).astype(np.int64)
    table[:2] = (0, Fr - T - 1)                                 # the store's first and last possible window
    cur_rows = np.stack([store[t + 1:t + 1 + T] for t in table]).reshape(N, T * D)
    hist_rows = np.stack([store[t:t + T] for t in table]).reshape(N, T * D)
    allowed = rng.integers(0, 1 << 25, N, dtype=np.int64).astype(np.uint32)
    allowed[rng.integers(0, N, max(N // 8, 1))] = 0
    allowed[rng.integers(0, N, max(N // 8, 1))] = 0xFE000000    # only bits above every 2K + 1
    allowed[rng.integers(0, N, max(N // 8, 1))] = 0xFFFFFFFF
    allowed[0] = 1 << (2 * K)                                   # shift +K
    cmap = rng.integers(-1, C, (2 * K + 1) * C).astype(np.int32)
    w = rng.random((N, C)).astype(np.float32)
    idx = rng.permutation(N).astype(np.int64)
    return dict(N=N, store=store, table=table, cur_rows=cur_rows, hist_rows=hist_rows, allowed=allowed, cmap=cmap, w=w, idx=idx)


def _launch_and_check(dev, pr, dv, T, rows, K, C, windows, use_idx, form, with_hist, with_target, step, seed):
    """one launch in one configuration at one value of the device step counter, against the reference"""
    from clvae_amd import ops
    row = T * D
    period, stride, offset, step0 = 3, rows, 2, 1
    base = TR.cursor_base(step, (step0, period, stride, offset))
    idx = pr['idx'] if use_idx else None
    row0 = 0 if use_idx else 3
    bufs = Bufs(dev)
    ld = D + 8 if form == 'strided' else D
    dt = torch.uint8 if form == 'byte' else torch.float32

    def out():
        return bufs.out(rows * T, ld, pad_cols=ld - D, dtype=dt)

    def src(which):      # (device source, the gather's extras, the reference's segment)
        t0 = {'cur': 1, 'hist': 0, 'target': 0}[which]
        if windows:
            return dv['store'], (D, t0 * D, dv['table']), (pr['store'], row, D, t0 * D, pr['table'])
        a = 'cur_rows' if which == 'cur' else 'hist_rows'
        return dv[a], (), (pr[a], row, row, 0, None)
    names = ['cur'] + (['hist'] if with_hist else []) + ['w'] + (['target'] if with_target else [])
    segs, ref_segs, outs = [], [], {}
    for nm in names:
        if nm == 'w':
            outs['w'] = bufs.out(rows, C)
            segs.append((dv['w'], outs['w'], C, 0, 0))
            continue
        s, ext, rs = src(nm)
        outs[nm] = out()
        # the history frames as TrainStep passes them: chunk D with a leading dimension; the others packed (chunk 0) when they can be
        chunk = D if (form == 'strided' or nm == 'hist') else 0
        segs.append((s, outs[nm], row, chunk, ld if chunk else 0) + ext)
        ref_segs.append(rs)
    notes = [None] * len(segs)
    note_bufs = {}
    for k, nm in enumerate(names):
        if nm in ('cur', 'hist'):
            note_bufs[nm] = notes[k] = bufs.out(rows * T, TR.NOTE_ROW, dtype=torch.uint8)
    shift_raw = torch.full((rows + 8,), -99, dtype=torch.int32, device=dev)
    dv['step'].fill_(step)
    ops.gather_transposed(rows, dv['idx'] if use_idx else None, segs, dv['allowed'], dv['cmap'], K, D, seed, step=12345,
                          step_dev=dv['step'], first_row=40, shift_out=shift_raw[:rows], label_seg=names.index('w'), row0=row0,
                          notes=notes, cursor=(dv['step'], step0, period, stride, offset))
    torch.cuda.synchronize()
    want, w_want, sh = TR.gather_transposed(rows, idx, row0, base, ref_segs, pr['w'], pr['allowed'], pr['cmap'], K, seed, step, 40)
    tag = (T, rows, K, C, windows, use_idx, form, with_hist, with_target, step)
    got_sh = shift_raw.cpu().numpy()
    assert np.array_equal(got_sh[:rows], sh) and (got_sh[rows:] == -99).all(), (tag, got_sh, sh)
    fnames = [nm for nm in names if nm != 'w']
    for nm, wf in zip(fnames, want):
        g = outs[nm].cpu().numpy()[:, :D].reshape(rows, T, D)
        assert g.dtype == (np.uint8 if form == 'byte' else np.float32)
        assert np.array_equal(g, wf.astype(g.dtype)), (tag, nm)
        if nm in note_bufs:
            TR.check_note_rows(note_bufs[nm].cpu().numpy(), wf)
    assert np.array_equal(outs['w'].cpu().numpy(), w_want), (tag, 'w')
    bufs.check_canaries()
    return sh


@pytest.mark.parametrize("C", [2, 10, 12])
@pytest.mark.parametrize("K", [0, 1, 6, 12])
@pytest.mark.parametrize("rows", [1, 6, 70])
@pytest.mark.parametrize("T", [1, 5])
def test_launch_against_the_reference(dev, T, rows, K, C):
    pr = _problem(T, rows, K, C, seed=1000 * T + 10 * rows + K + C)
    dv = dict(store=U8(pr['store'], dev), table=I64(pr['table'], dev), cur_rows=U8(pr['cur_rows'], dev),
              hist_rows=U8(pr['hist_rows'], dev), allowed=torch.as_tensor(pr['allowed'].view(np.int32), device=dev),
              cmap=torch.as_tensor(pr['cmap'], device=dev), w=F(pr['w'], dev), idx=I64(pr['idx'], dev),
              step=torch.zeros(1, dtype=torch.int32, device=dev))
    seen = set()
    for windows in (True, False):
        for use_idx in (False, True):
            for form in ('float', 'byte', 'strided'):
                for with_hist in (True, False):
                    for with_target in (False, True):
                        for step in range(5):                   # counter - step0 = -1, 0, 1, 2, 3: the cursor wraps at both ends
                            sh = _launch_and_check(dev, pr, dv, T, rows, K, C, windows, use_idx, form, with_hist, with_target,
                                                   step, seed=0xABCDEF0123 + K)
                            seen.update(sh.tolist())
    assert seen <= set(range(-K, K + 1))
    if rows == 70:                                              # (210 source rows at 5 steps: fewer rows need not meet all 25)
        assert len(seen) == 2 * K + 1                           # every shift occurred


@pytest.mark.parametrize("form", ['float', 'byte', 'strided'])
@pytest.mark.parametrize("K", [1, 6, 12])
@pytest.mark.parametrize("T", [1, 5])
def test_frame_edges_and_store_ends(dev, T, K, form):
    """A store of exactly T + 1 frames: frame f ends with note 87 on, frame f + 1 begins with note 0 on.  Windows at the
    store's first and last position, shifted by +-1 and +-K: what leaves a frame is gone, what enters is zero."""
    from clvae_amd import ops
    store = np.zeros((T + 1, D), np.uint8)
    for f in range(T + 1):
        store[f, 87 if f % 2 == 0 else 0] = 1
        store[f, 40 + f] = 1
    table = np.array([0, 1, 0, 1, 0, 1, 0, 1], np.int64)
    shifts = np.array([1, 1, -1, -1, K, K, -K, -K])
    allowed = (1 << (shifts + K)).astype(np.uint32)
    d_store, d_table = U8(store, dev), I64(table, dev)
    bufs = Bufs(dev)
    ld = D + 4 if form == 'strided' else D
    out = bufs.out(8 * T, ld, pad_cols=ld - D, dtype=torch.uint8 if form == 'byte' else torch.float32)
    notes = bufs.out(8 * T, TR.NOTE_ROW, dtype=torch.uint8)
    sh = torch.zeros(8, dtype=torch.int32, device=dev)
    cmap = torch.zeros((2 * K + 1) * 2, dtype=torch.int32, device=dev)
    ops.gather_transposed(8, None, [(d_store, out, T * D, D, ld, D, 0, d_table)], torch.as_tensor(allowed.view(np.int32), device=dev),
                          cmap, K, D, seed=3, shift_out=sh, notes=[notes])
    torch.cuda.synchronize()
    assert np.array_equal(sh.cpu().numpy(), shifts)
    got = out.cpu().numpy()[:, :D].reshape(8, T, D)
    want, _, _ = TR.gather_transposed(8, None, 0, 0, [(store, T * D, D, 0, table)], None, allowed, None, K, 3, 0)
    assert np.array_equal(got, want[0].astype(got.dtype))
    TR.check_note_rows(notes.cpu().numpy(), want[0])
    for r in range(8):
        s = int(shifts[r])
        for t in range(T):
            fr = store[table[r] + t]
            g = got[r, t]
            if s > 0:
                assert (g[:s] == 0).all()                       # nothing of the frame before came in
                assert g.sum() == fr[:D - s].sum()              # note 87 left, note 0 moved to s
            else:
                assert (g[D + s:] == 0).all()                   # nothing of the frame behind came in
                assert g.sum() == fr[-s:].sum()
            assert g[40 + table[r] + t + s] == 1
    bufs.check_canaries()


@pytest.mark.parametrize("Dn,form,pad", [(88, 'byte', 4),       # byte rows 92 apart: 4-byte work items
                                         (44, 'byte', 0), (44, 'float', 4),      # a frame size that is no multiple of 8
                                         (48, 'byte', 8), (48, 'float', 0),      # 8-byte work items, frame size not 88
                                         (4, 'byte', 0), (8, 'float', 0)])       # frames of one work item
def test_the_other_work_item_sizes_and_frame_sizes(dev, Dn, form, pad):
    """The launch picks 8-byte work items where every frame segment can store them and divides by a constant where D = 88:
    the three other instances of the kernel, windows and whole rows, with note lists, at a cursor that wraps."""
    from clvae_amd import ops
    T, rows, K, C, seed = 3, 37, min(6, Dn // 4), 5, 91
    rng = np.random.default_rng(Dn)
    N, Fr = 3 * rows, 3 * rows + T + 2
    store = (rng.random((Fr, Dn)) < 0.2).astype(np.uint8)
    table = rng.integers(0, Fr - T, N).astype(np.int64)
    table[:2] = (0, Fr - T)
    allowed = rng.integers(0, 1 << 25, N, dtype=np.int64).astype(np.uint32)
    cmap = rng.integers(-1, C, (2 * K + 1) * C).astype(np.int32)
    w, idx = rng.random((N, C)).astype(np.float32), rng.permutation(N).astype(np.int64)
    d_store, d_table, d_idx, d_w = U8(store, dev), I64(table, dev), I64(idx, dev), F(w, dev)
    d_rows = U8(np.stack([store[t:t + T] for t in table]).reshape(N, T * Dn), dev)
    d_allowed, d_cmap = torch.as_tensor(allowed.view(np.int32), device=dev), torch.as_tensor(cmap, device=dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    ld = Dn + pad
    for windows in (True, False):
        for it in (0, 1, 2, 3):
            bufs = Bufs(dev)
            out = bufs.out(rows * T, ld, pad_cols=pad, dtype=torch.uint8 if form == 'byte' else torch.float32)
            notes, wo = bufs.out(rows * T, TR.NOTE_ROW, dtype=torch.uint8), bufs.out(rows, C)
            sh = torch.zeros(rows, dtype=torch.int32, device=dev)
            seg = (d_store, out, T * Dn, Dn, ld, Dn, 0, d_table) if windows else (d_rows, out, T * Dn, Dn, ld)
            step.fill_(it)
            ops.gather_transposed(rows, d_idx, [seg, (d_w, wo, C, 0, 0)], d_allowed, d_cmap, K, Dn, seed, step_dev=step, first_row=5,
                                  shift_out=sh, label_seg=1, notes=[notes, None], cursor=(step, 0, 3, rows, 0))
            torch.cuda.synchronize()
            want, w_want, sh_want = TR.gather_transposed(rows, idx, 0, (it % 3) * rows, [(store, T * Dn, Dn, 0, table)], w, allowed, cmap,
                                                         K, seed, it, 5, D=Dn)
            assert np.array_equal(sh.cpu().numpy(), sh_want)
            got = out.cpu().numpy()[:, :Dn].reshape(rows, T, Dn)
            assert np.array_equal(got, want[0].astype(got.dtype)), (windows, it)
            assert np.array_equal(wo.cpu().numpy(), w_want)
            TR.check_note_rows(notes.cpu().numpy(), want[0])
            bufs.check_canaries()


@pytest.mark.parametrize("use_idx", [False, True])
def test_two_half_launches_equal_one(dev, use_idx):
    from clvae_amd import ops
    T, rows, K, C = 5, 70, 6, 10
    pr = _problem(T, rows, K, C, seed=77)
    store, table = U8(pr['store'], dev), I64(pr['table'], dev)
    allowed, cmap = torch.as_tensor(pr['allowed'].view(np.int32), device=dev), torch.as_tensor(pr['cmap'], device=dev)
    w, idx = F(pr['w'], dev), I64(pr['idx'], dev)
    step = torch.full((1,), 9, dtype=torch.int32, device=dev)

    def run(parts):
        X, Xh = torch.zeros(rows, T * D, device=dev), torch.zeros(rows, T * D, dtype=torch.uint8, device=dev)
        wo, sh = torch.zeros(rows, C, device=dev), torch.zeros(rows, dtype=torch.int32, device=dev)
        for a, b in parts:
            segs = [(store, X[a:b], T * D, D, D, D, D, table), (store, Xh[a:b], T * D, D, D, D, 0, table), (w, wo[a:b], C, 0, 0)]
            ops.gather_transposed(b - a, idx[a:] if use_idx else None, segs, allowed, cmap, K, D, seed=11, step_dev=step,
                                  first_row=100 + a, shift_out=sh[a:b], label_seg=2, row0=0 if use_idx else a)
        torch.cuda.synchronize()
        return X, Xh, wo, sh
    one, two = run([(0, rows)]), run([(0, rows // 2), (rows // 2, rows)])
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    assert len(set(one[3].cpu().numpy().tolist())) > 3


# ---------------------------------------------------------------- TrainStep --
def _windows_in_range(rng, n, Tn, lo=20, hi=60, density=0.08):
    win = np.zeros((n, Tn + 1, D), bool)
    win[:, :, lo:hi] = rng.random((n, Tn + 1, hi - lo)) < density
    return win


def _reference_batch(plan, win, keys, it, period, B, seed, first_row=0):
    """the transposed batch of step `it` (iterations == it): rows (it mod period) * B .. of the data set"""
    base = (it % period) * B
    sr = np.arange(base, base + B)
    sh = TR.draw_shifts(plan.allowed[sr], plan.K, seed, it, first_row)
    n, T1 = win.shape[0], win.shape[1]
    outs, w_out, sh2 = TR.gather_transposed(B, None, 0, base, [(win.astype(np.uint8), T1 * D, T1 * D, 0, None)], keys.astype(np.float32),
                                            plan.allowed, plan.class_map, plan.K, seed, it, first_row)
    assert np.array_equal(sh, sh2)
    return outs[0], w_out, sh


def test_trainstep_with_a_plan_follows_the_oracle_on_the_transposed_batches(dev):
    from clvae_amd.augment import TransposePlan
    from clvae_amd.engine import VrnnEngine
    from clvae_amd.trainer import TrainStep
    B, Tn, L, Cn, steps, period, seed = 16, 10, 2, 10, 4, 2, 808
    cfg = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=True)
    rng = np.random.default_rng(3)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=9).items()}
    win = _windows_in_range(rng, period * B, Tn)
    lab = rng.integers(0, Cn, period * B)
    keys = np.eye(Cn)[lab]
    cur, hist = win[:, 1:].reshape(period * B, -1), win[:, :-1].reshape(period * B, -1)
    plan = TransposePlan.build([cur.reshape(-1, Tn, D), hist.reshape(-1, Tn, D)], lab, JSB_KEYS, semitones=6)
    assert plan.counts().min() >= 2
    eng = VrnnEngine(cfg, B, dev)
    eng.P.set_weights(p)
    ts = TrainStep(eng, seed=seed)
    ts.bind_batches(U8(cur, dev), U8(hist, dev), F(keys, dev), idx=None, period=period, stride=B, augment=plan.to(dev))
    st = O.adam_wn_init(p)
    seen = []
    for it in range(steps):
        ts.step()
        torch.cuda.synchronize()
        got = eng.losses()
        wt, w_t, sh = _reference_batch(plan, win, keys, it, period, B, seed)
        assert np.array_equal(ts.shifts.cpu().numpy(), sh), (it, ts.shifts.cpu().numpy(), sh)
        assert np.array_equal(ts.w_true.cpu().numpy(), w_t)
        seen.append(sh)
        eW = f32(OP.normal(B * (Cn - 1), seed, step=it, stream_id=0).reshape(B, Cn - 1))
        eZ = f32(OP.normal(B * Tn * L, seed, step=it, stream_id=1).reshape(B, Tn, L))
        ref = O.vrnn_loss_and_grads(p, cfg, wt[:, 1:].astype(np.float64), wt[:, :-1].astype(np.float64), w_t.astype(np.float64), eW, eZ)
        O.adam_wn_step(p, ref['grads'], st)
        for k in ('vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
            assert abs(got[k] - ref[k]) <= 1e-3, (it, k, got[k], ref[k])
    assert int(eng.P.iterations.item()) == steps
    assert not np.array_equal(seen[0], seen[2]) and not np.array_equal(seen[1], seen[3])      # the same windows, other shifts
    w = eng.P.get_weights()
    for k in p:
        d = np.abs(w[k] - p[k])
        assert float((d > 1e-4 * np.abs(p[k]) + 2e-5).mean()) <= 1e-2 and d.max() <= 2e-3 * steps, (k, d.max())


def test_cl_vae_trainstep_with_a_plan_follows_the_oracle(dev):
    from clvae_amd.augment import TransposePlan
    from clvae_amd.engine import VaeEngine
    from clvae_amd.trainer import TrainStep
    B, L, Cn, steps, period, seed = 100, 4, 2, 3, 2, 31
    cfg = O.vae_config(latent_dim=L, n_classes=Cn, use_x_prev=True)
    rng = np.random.default_rng(11)
    p = {k: f32(v) for k, v in O.vae_init_params(cfg, seed=1).items()}
    win = _windows_in_range(rng, period * B, 1)
    lab = rng.integers(0, Cn, period * B)
    keys = np.eye(Cn)[lab]
    cur, hist = win[:, 1], win[:, 0]
    plan = TransposePlan.build([cur, hist], lab, {'C': 0, 'G': 1}, semitones=6)
    eng = VaeEngine(cfg, B, dev)
    eng.P.set_weights(p)
    ts = TrainStep(eng, seed=seed)
    ts.bind_batches(U8(cur, dev), U8(hist, dev), F(keys, dev), idx=None, period=period, stride=B, augment=plan.to(dev))
    st = O.adam_wn_init(p)
    for it in range(steps):
        ts.step()
        torch.cuda.synchronize()
        got = eng.losses()
        wt, w_t, sh = _reference_batch(plan, win, keys, it, period, B, seed)
        assert np.array_equal(ts.shifts.cpu().numpy(), sh) and (sh != 0).any() and set(sh.tolist()) <= {-5, 0, 5}
        eW = f32(OP.normal(B * (Cn - 1), seed, step=it, stream_id=0).reshape(B, Cn - 1))
        eZ = f32(OP.normal(B * L, seed, step=it, stream_id=1).reshape(B, L))
        ref = O.vae_loss_and_grads(p, cfg, wt[:, 1].astype(np.float64), wt[:, 0].astype(np.float64), w_t.astype(np.float64), eW, eZ)
        O.adam_wn_step(p, ref['grads'], st)
        for k in ('vae', 'kl_z', 'kl_w', 'w_rec', 'total'):
            assert abs(got[k] - ref[k]) <= 1e-3, (it, k, got[k], ref[k])
    w = eng.P.get_weights()
    for k in p:
        np.testing.assert_allclose(w[k], p[k], rtol=2e-3, atol=2e-5, err_msg=k)


def test_large_batch_stays_bytes_under_a_plan(dev):
    from clvae_amd.augment import TransposePlan
    from clvae_amd.engine import VrnnEngine
    from clvae_amd.trainer import TrainStep
    B, Tn, L, Cn, period, seed = 768, 3, 12, 10, 2, 5
    cfg = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=True)
    rng = np.random.default_rng(B)
    win = _windows_in_range(rng, period * B, Tn)
    lab = rng.integers(0, Cn, period * B)
    keys = np.eye(Cn)[lab]
    cur, hist = win[:, 1:].reshape(period * B, -1), win[:, :-1].reshape(period * B, -1)
    plan = TransposePlan.build([win[:, 1:], win[:, :-1]], lab, JSB_KEYS, semitones=6)
    eng = VrnnEngine(cfg, B, dev)
    assert eng.frames_u8_route() == 'gather'
    eng.P.set_weights({k: np.asarray(v, np.float32) for k, v in O.vrnn_init_params(cfg, seed=3).items()})
    ts = TrainStep(eng, seed=seed)
    ts.bind_batches(U8(cur, dev), U8(hist, dev), F(keys, dev), idx=None, period=period, stride=B, augment=plan.to(dev))
    for it in range(3):                                         # eager, the capture, a replay
        ts.step()
        torch.cuda.synchronize()
        assert ts._f8 is not None and ts._f8[0] is ts.X8
        wt, w_t, sh = _reference_batch(plan, win, keys, it, period, B, seed)
        assert np.array_equal(ts.shifts.cpu().numpy(), sh)
        assert np.array_equal(ts.X8.cpu().numpy().reshape(B, Tn, D), wt[:, 1:])
        assert np.array_equal(ts.Xp8.cpu().numpy().reshape(B, Tn, D), wt[:, :-1])
        assert np.array_equal(ts.w_true.cpu().numpy(), w_t)
        assert all(np.isfinite(v) for v in eng.losses().values())


def test_bind_refuses_frames_that_are_not_bytes(dev):
    from clvae_amd.augment import TransposePlan
    from clvae_amd.engine import VrnnEngine
    from clvae_amd.trainer import TrainStep
    B, Tn, Cn = 4, 3, 10
    cfg = O.vrnn_config(latent_dim=2, seq_length=Tn, n_classes=Cn, use_x_prev=True)
    rng = np.random.default_rng(0)
    win = _windows_in_range(rng, B, Tn)
    lab = rng.integers(0, Cn, B)
    cur, hist = win[:, 1:].reshape(B, -1), win[:, :-1].reshape(B, -1)
    plan = TransposePlan.build([win[:, 1:], win[:, :-1]], lab, JSB_KEYS, semitones=6).to(dev)
    ts = TrainStep(VrnnEngine(cfg, B, dev), seed=1)
    with pytest.raises(ValueError, match='uint8'):
        ts.bind_batches(F(cur, dev), U8(hist, dev), F(np.eye(Cn)[lab], dev), augment=plan)
    with pytest.raises(ValueError, match='uint8'):
        ts.bind_batches(U8(cur, dev), F(hist, dev), F(np.eye(Cn)[lab], dev), augment=plan)
    assert ts._bound is None


# ---------------------------------------------------------------- Model.fit --
def test_fit_with_a_plan_trains_on_shifted_rows_and_validates_on_plain_ones(dev):
    from clvae_amd.augment import TransposePlan
    from clvae_amd.cl_vrnn.model import get_model
    from clvae_amd.keras_like import OptimizerSpec
    from clvae_amd.utils.pianoroll import Windows
    B, T, L, Cn = 8, 10, 2, 10
    rng = np.random.default_rng(6)
    n = 4 * B
    store = np.zeros((n + T + 1, D), np.uint8)
    store[:, 20:60] = rng.random((n + T + 1, 40)) < 0.08
    starts = rng.permutation(n).astype(np.int64)
    y, x = Windows(store, starts, 1, T), Windows(store, starts, 0, T)
    vy, vx = y[:2 * B], x[:2 * B]
    lab = rng.integers(0, Cn, n)
    w = np.eye(Cn)[lab]
    plan = TransposePlan.build([y, x], lab, JSB_KEYS, semitones=6)
    model, _ = get_model(B, 88, 88, L, T, Cn, True, 'adam-wn', seed=3)
    np.random.seed(1)
    hist = model.fit([y, x], [y, w, w, y], shuffle=True, epochs=2, batch_size=B, verbose=0, augment=plan,
                     validation_data=([vy, vx], [vy, w[:2 * B], w[:2 * B], vy]))
    assert len(hist.history['loss']) == 2 and all(np.isfinite(v).all() for v in hist.history.values())
    sh = model._step.shifts.cpu().numpy()
    assert sh.shape == (B,) and (sh != 0).any() and np.abs(sh).max() <= 6
    assert model._step._bound is None
    # validation is never augmented: with lr = 0 the weights stay, and val_* of a fit with and without the plan agree exactly
    vals = []
    for aug in (plan, None):
        m, _ = get_model(B, 88, 88, L, T, Cn, True, OptimizerSpec('adam-wn', lr=0.0), seed=3)      # the same initial weights
        np.random.seed(2)
        h = m.fit([y, x], [y, w, w, y], shuffle=True, epochs=1, batch_size=B, verbose=0, augment=aug,
                  validation_data=([vy, vx], [vy, w[:2 * B], w[:2 * B], vy]))
        vals.append({k: v for k, v in h.history.items() if k.startswith('val_')})
        train = {k: v for k, v in h.history.items() if not k.startswith('val_')}
        vals[-1]['_train_loss'] = train['loss']
    assert len(vals[0]) > 3
    for k in vals[0]:
        if k != '_train_loss':
            assert vals[0][k] == vals[1][k], (k, vals[0][k], vals[1][k])
    assert vals[0]['_train_loss'] != vals[1]['_train_loss']     # ... while the training rows did differ


# ------------------------------------------------------------------ train.py --
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_train_tool_with_transpose(dev, tmp_path, which):
    import importlib
    from clvae_amd.cli import AUGMENT_FLAGS, OPTIMIZER_FLAGS, parser_for
    TRN = importlib.import_module('clvae_amd.%s.train' % which)
    data = make_synthetic_pickle(str(tmp_path / "syn.pickle"), n_songs=(10, 4, 4), seed=2)
    mdir = str(tmp_path / "models")
    os.makedirs(mdir)
    extra = ['--seq_length', '8'] if which == 'cl_vrnn' else []
    args = parser_for(which + '.train', OPTIMIZER_FLAGS + AUGMENT_FLAGS).parse_args(
        ['tr', '--use_x_prev', '--batch_size', '20', '--num_epochs', '2', '--train_file', data, '--model_dir', mdir, '--patience', '0',
         '--transpose', '6'] + extra)
    np.random.seed(1)
    model, best = TRN.train(args)
    h = model.history.history
    assert len(h['loss']) == 2 and all(np.isfinite(v).all() for v in h.values())
    assert json.load(open(os.path.join(mdir, 'tr.json')))['transpose'] == 6
    sh = model._step.shifts.cpu().numpy()
    assert (sh != 0).any() and set(sh.tolist()) <= {-5, -2, 0, 2, 5}   # the synthetic keys are C, F and G
