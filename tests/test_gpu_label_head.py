"""-m gpu: the label head kernels (csrc/label_head.hip, label_bwd_row.h) called directly, every output against the fp64
reference of tests/label_reference.py: per element within the element's own rounding bound, hit exactly outside near-tie
rows, and per slice (batch row, column).  Every output buffer is NaN-filled with a canary tail (uint8 ones: 0xA5 inside),
strided ones with canary padding columns, and the canaries are checked after the launches.

Entry points and shapes (within each one's support):
  a  clv_vrnn_label_fwd            hW given (exact zeros in it): B 1 / 7 / 300, D 1 / 2 / 3 / 88 / 128, C 2 .. 32, G4 8 / 352 / 400
  b  clv_vrnn_label_fwd_x          float X, ldx > nx with NaN padding, an empty row, a dense row, values other than 0 / 1,
                                   nx = T D for T 1 / 3 / 16 / 128 (ragged last 64-input chunks)
  c  ... with a clv_label_stage    widened X / Xh (hist_ld > hist_chunk) or bytes X8 / Xh8; bytes 2 and 255; idx or row0;
                                   tables; a cursor with step < step0; labels from w_src copied to w_out
  d  clv_vrnn_label_fwd_parts      after clv_dense_window_fwd_bf16, splits 1 .. 176 (> 48: a wave's chunk loop runs twice)
  e  the front kernel (proj=)      B 1 / 63 / 64 / 65 / 130 around the 64-row projection workgroup, T = 1
  f  in-kernel noise               odd C - 1, first > 2^32, a device step
  g  label edge rows               exact ties (W = 1/C), an all-zero onehot row, w_rec clipped at both ends, prior != 0
  h  clv_vrnn_label_bwd            G4 = 400 > LH_T, C up to 32 (NA = 62: two 32-wide dhW passes); layer_grad none /
                                   immediate / deferred to a ReduceQueue (bit for bit the immediate one)
The worst error / bound ratio of every output and the number of near-tie rows and relu-edge elements are printed at the end
of the module (run with -s)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import philox as OP
import label_reference as LR
from helpers import Bufs, FILL_U8

pytestmark = pytest.mark.gpu

SLICE_RTOL = 1e-4
_REPORT = dict(ratios={}, tie_rows=0, relu_edge=0, rows=0)


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    yield torch.device("cuda:0")
    r = _REPORT
    print("\nlabel head: worst error / bound per output: %s" % ", ".join("%s %.3g" % kv for kv in sorted(r['ratios'].items())))
    print("label head: %d rows, %d near-tie rows and %d relu-edge hW elements flagged" % (r['rows'], r['tie_rows'], r['relu_edge']))


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def T(a, dev, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def N(t):
    return t.detach().cpu().numpy().astype(np.float64)


def params(rng, B, D, C, G4, prior=0.2):
    """the label head's weights and noise (fp32 values): wargs ~ N(0, 0.5^2) for unit-sized hW"""
    NA = 2 * (C - 1)
    return dict(Ka=f32(rng.standard_normal((D, NA)) * 0.6 / np.sqrt(D)), ba=f32(rng.standard_normal(NA) * 0.2),
                eps=f32(rng.standard_normal((B, C - 1))), onehot=np.eye(C)[rng.integers(0, C, B)], prior=prior,
                Kenc_w=f32(rng.standard_normal((C, G4)) * 0.3), benc=f32(rng.standard_normal(G4) * 0.1),
                Kdec_w=f32(rng.standard_normal((C, G4)) * 0.3), bdec=f32(rng.standard_normal(G4) * 0.1))


def outputs(bufs, B, D, C, G4):
    o = dict(wargs=bufs.out(B, 2 * (C - 1)), W=bufs.out(B, C), rowloss=bufs.out(B, 3), rb_enc=bufs.out(B, G4),
             rb_dec=bufs.out(B, G4))
    o['hW'] = bufs.out(B, D)
    return o


def label_args(p, o, dev, onehot=True):
    """the trailing arguments shared by the forward entry points (eps .. rb_dec)"""
    return dict(eps=o.get('eps', T(p['eps'], dev)), onehot=T(p['onehot'], dev) if onehot else None, prior=p['prior'],
                Kenc_w=T(p['Kenc_w'], dev), benc=T(p['benc'], dev), Kdec_w=T(p['Kdec_w'], dev), bdec=T(p['bdec'], dev))


def x_call(B, D, C, G4, X, ldx, nx, Kh, bh, p, o, dev, **kw):
    from clvae_amd import ops
    a = label_args(p, o, dev)
    ops.vrnn_label_fwd_x(B, D, C, G4, X, ldx, nx, Kh, bh, o['hW'], T(p['Ka'], dev), T(p['ba'], dev), a['eps'], a['onehot'],
                         a['prior'], a['Kenc_w'], a['benc'], a['Kdec_w'], a['bdec'], o['wargs'], o['W'], o['rowloss'],
                         o['rb_enc'], o['rb_dec'], **kw)


def check(o, ref, name):
    got = {k: N(o[k]) for k in LR.OUTPUTS + ('rowloss',)}
    r = LR.check_forward(got, ref, name + ': ', SLICE_RTOL)
    for k, v in r.items():
        _REPORT['ratios'][k] = max(_REPORT['ratios'].get(k, 0.0), v)
    _REPORT['tie_rows'] += int(ref['tie'].sum())
    _REPORT['relu_edge'] += int(ref['relu_edge'].sum())
    _REPORT['rows'] += ref['W'].shape[0]
    return got


def window(rng, B, nx, density=0.1):
    """float rows: row 0 has no notes, row 1 is dense, row 2 has values other than 0 / 1"""
    X = (rng.random((B, nx)) < density).astype(np.float64)
    X[0] = 0.0
    if B > 1:
        X[1] = 1.0
    if B > 2:
        X[2] = f32(rng.standard_normal(nx) * (rng.random(nx) < 0.3))
    return X


def kh(rng, nx, D, density=0.1):
    return f32(rng.standard_normal((nx, D)) / np.sqrt(max(density * nx, 1.0))), f32(rng.standard_normal(D) * 0.3)


# ---- a: clv_vrnn_label_fwd ----
@pytest.mark.parametrize("B,D,C,G4", [(1, 1, 2, 8), (7, 3, 17, 400), (300, 88, 10, 352), (7, 128, 32, 400), (7, 2, 3, 8),
                                      (1, 4, 32, 352)])
@pytest.mark.parametrize("with_onehot", [True, False])
def test_label_fwd_from_hW(dev, B, D, C, G4, with_onehot):
    from clvae_amd import ops
    rng = np.random.default_rng(B * 7 + D * 3 + C)
    p = params(rng, B, D, C, G4)
    hW = f32(np.maximum(rng.standard_normal((B, D)), 0))          # about half exact zeros
    bufs = Bufs(dev)
    o = outputs(bufs, B, D, C, G4)
    a = label_args(p, o, dev, with_onehot)
    ops.vrnn_label_fwd(B, D, C, G4, T(hW, dev), T(p['Ka'], dev), T(p['ba'], dev), a['eps'], a['onehot'], a['prior'],
                       a['Kenc_w'], a['benc'], a['Kdec_w'], a['bdec'], o['wargs'], o['W'], o['rowloss'], o['rb_enc'],
                       o['rb_dec'])
    torch.cuda.synchronize()
    q = dict(p, onehot=p['onehot'] if with_onehot else None)
    ref = LR.forward(q['Ka'], q['ba'], q['eps'], q['onehot'], q['prior'], q['Kenc_w'], q['benc'], q['Kdec_w'], q['bdec'],
                     hW=hW)
    o['hW'] = T(hW, dev)
    check(o, ref, 'fwd')
    if not with_onehot:
        assert (N(o['rowloss'])[:, 1:] == 0).all()
    bufs.check_canaries()


# ---- b: clv_vrnn_label_fwd_x from float X ----
@pytest.mark.parametrize("B,D,C,G4,Tn", [(7, 88, 10, 352, 3), (1, 2, 2, 8, 1), (300, 88, 3, 352, 16), (7, 128, 32, 400, 128),
                                         (7, 4, 17, 8, 3)])
def test_label_fwd_x_from_float_rows(dev, B, D, C, G4, Tn):
    rng = np.random.default_rng(B + D + C + Tn)
    nx = Tn * D
    ldx = nx + 6
    p = params(rng, B, D, C, G4)
    X = window(rng, B, nx)
    Kh, bh = kh(rng, nx, D)
    Xp = np.full((B, ldx), np.nan)          # the padding columns must not be read
    Xp[:, :nx] = X
    bufs = Bufs(dev)
    o = outputs(bufs, B, D, C, G4)
    x_call(B, D, C, G4, T(Xp, dev), ldx, nx, T(Kh, dev), T(bh, dev), p, o, dev)
    torch.cuda.synchronize()
    ref = LR.forward(p['Ka'], p['ba'], p['eps'], p['onehot'], p['prior'], p['Kenc_w'], p['benc'], p['Kdec_w'], p['bdec'],
                     X=X, Kh=Kh, bh=bh)
    got = check(o, ref, 'fwd_x')
    assert (got['hW'][0] == np.maximum(f32(bh), 0)).all()        # no notes: relu(bh) exactly
    bufs.check_canaries()


# ---- c: with a clv_label_stage ----
def _stores(rng, nrows, nx, C):
    """current / history byte stores (stride and offset multiples of 4, rows through a table), labels w_src"""
    stride, offset = nx + 8, 4
    cur = (rng.random(nrows * stride + 16) < 0.1).astype(np.uint8)
    cur[rng.random(cur.size) < 0.01] = 2
    cur[offset + stride * np.arange(1, nrows, 5)] = 2
    hist = (rng.random(nrows * nx + 8) < 0.1).astype(np.uint8)
    hist[rng.random(hist.size) < 0.02] = 255
    cur[offset + stride * 3 + 1] = 255              # one 255 in the current frames of stored row 3
    table = rng.permutation(nrows).astype(np.int64)
    w_src = np.eye(C)[rng.integers(0, C, nrows)]
    return (cur, stride, offset, table), (hist, nx, 0, None), w_src


@pytest.mark.parametrize("B,D,C,G4,Tn,as_bytes,use_idx", [(7, 88, 10, 352, 3, False, True), (7, 88, 10, 352, 3, True, False),
                                                          (65, 4, 2, 8, 16, False, False), (1, 128, 32, 400, 1, True, True)])
def test_label_fwd_x_with_stage(dev, B, D, C, G4, Tn, as_bytes, use_idx):
    from clvae_amd import ops
    rng = np.random.default_rng(B * 3 + Tn + as_bytes)
    nx, period, stride, off = Tn * D, 3, B + 2, 1
    nrows = period * stride + off + 4
    curs, hists, w_src = _stores(rng, nrows, nx, C)
    idx = rng.permutation(nrows).astype(np.int64) if use_idx else None
    row0 = 0 if use_idx else 2
    step, step0 = 4, 9                       # (4 - 9) mod 3 = 1
    if not use_idx:
        nrows_needed = row0 + ((step - step0) % period) * stride + off + B
        assert nrows_needed <= nrows
    sr = LR.stage_rows(B, idx, row0, (step, step0, period, stride, off))
    hist_chunk, hist_ld = D, D + 4
    want = LR.assemble(sr, nx, curs, hists, hist_chunk, hist_ld, w_src)
    p = params(rng, B, D, C, G4)
    Kh, bh = kh(rng, nx, D)
    Kh[1] = f32(Kh[1] / 64)                  # input 1 holds the 255 of stored row 3: keep its hW (and W) finite
    bufs = Bufs(dev)
    o = outputs(bufs, B, D, C, G4)
    dv = lambda a: None if a is None else torch.as_tensor(a, device=dev)
    sdev = torch.tensor([step], dtype=torch.int32, device=dev)
    w_out = bufs.out(B, C)
    if as_bytes:
        X8, Xh8 = bufs.out(B, nx, dtype=torch.uint8), bufs.out(B, nx, dtype=torch.uint8)
        Xo = Xh = None
    else:
        Xo, Xh = bufs.out(B, nx + 4, pad_cols=4), bufs.out(B * (nx // hist_chunk), hist_ld, pad_cols=hist_ld - hist_chunk)
    keep = [dv(curs[0]), dv(curs[3]), dv(hists[0]), dv(idx), T(w_src, dev)]     # alive until the launch: the stage holds pointers
    g = ops.label_stage((keep[0], curs[1], curs[2], keep[1]), (keep[2], hists[1], hists[2], None), keep[3], row0,
                        (sdev, step0, period, stride, off), Xo, Xh, hist_chunk, hist_ld, keep[4], w_out,
                        bytes_out=(X8, Xh8) if as_bytes else None)
    x_call(B, D, C, G4, None, nx + 4, nx, T(Kh, dev), T(bh, dev), p, o, dev, stage=g)
    torch.cuda.synchronize()
    if as_bytes:
        assert np.array_equal(X8.cpu().numpy(), want['X8']) and np.array_equal(Xh8.cpu().numpy(), want['Xh8'])
        assert FILL_U8 not in want['X8'] and FILL_U8 not in want['Xh8']
    else:
        assert np.array_equal(N(Xo)[:, :nx], want['X'])
        assert np.array_equal(N(Xh)[:, :hist_chunk], want['Xh'][:, :hist_chunk])
    assert np.array_equal(N(w_out), want['w_out'])
    assert (want['X'] == 2).any() and (want['Xh8'] == 255).any()
    p['onehot'] = want['w_out']
    ref = LR.forward(p['Ka'], p['ba'], p['eps'], p['onehot'], p['prior'], p['Kenc_w'], p['benc'], p['Kdec_w'], p['bdec'],
                     X=want['X'], Kh=Kh, bh=bh)
    check(o, ref, 'stage')
    bufs.check_canaries()


# ---- d: clv_vrnn_label_fwd_parts after clv_dense_window_fwd_bf16 ----
@pytest.mark.parametrize("B,D,C,G4,Tn,u8", [(1, 88, 10, 352, 128, True), (300, 4, 17, 400, 16, False), (7, 88, 32, 8, 3, True),
                                            (130, 96, 3, 352, 16, True)])
def test_label_fwd_parts(dev, B, D, C, G4, Tn, u8):
    from clvae_amd import ops
    rng = np.random.default_rng(B + Tn + D)
    nx = Tn * D
    assert ops.dense_window_fwd_bf16_supported(B, nx, D, nx, D)
    X = (rng.random((B, nx)) < 0.1).astype(np.float64)
    X[0] = 0.0
    if u8:
        X[-1, ::7] = 2.0
    Kh, bh = kh(rng, nx, D)
    p = params(rng, B, D, C, G4)
    ws = ops.Workspace(dev)
    Xd = T(X, dev, np.uint8) if u8 else T(X, dev)
    part, splits = ops.dense_window_fwd_bf16(B, nx, D, Xd, nx, T(Kh, dev), D, ws)
    assert splits == ops._lib.lib().clv_dense_window_fwd_bf16_splits(B, nx)
    if (B, Tn) == (1, 128):
        assert splits > 48, splits          # 8 loads x 6 waves: every wave's chunk loop runs twice or more
    bufs = Bufs(dev)
    o = outputs(bufs, B, D, C, G4)
    x_call(B, D, C, G4, None, 0, 0, None, T(bh, dev), p, o, dev, parts=(part, splits))
    torch.cuda.synchronize()
    ref = LR.forward(p['Ka'], p['ba'], p['eps'], p['onehot'], p['prior'], p['Kenc_w'], p['benc'], p['Kdec_w'], p['bdec'],
                     X=X, Kh=Kh, bh=bh)
    check(o, ref, 'parts')
    bufs.check_canaries()


# ---- e: the front kernel ----
@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_front_kernel(dev, B):
    from clvae_amd import ops
    D, C, G4, Tn, Np = 88, 10, 352, 1, 352
    rng = np.random.default_rng(500 + B)
    nx = Tn * D
    nrows = B + 5
    cur = (rng.random(nrows * nx) < 0.15).astype(np.uint8)
    hist = (rng.random(nrows * nx) < 0.15).astype(np.uint8)
    cur[:nx] = 1                          # a dense frame (source row 0)
    hist[nx:2 * nx] = 0
    w_src = np.eye(C)[rng.integers(0, C, nrows)]
    idx = rng.permutation(nrows).astype(np.int64)
    sr = LR.stage_rows(B, idx)
    want = LR.assemble(sr, nx, (cur, nx, 0, None), (hist, nx, 0, None), None, None, w_src)
    Kc, Kh_ = f32(rng.standard_normal((D, Np)) * 0.3), f32(rng.standard_normal((D, Np)) * 0.3)
    assert ops.vrnn_label_fwd_x_proj_supported(B, D, nx, Tn, Np)
    Kh, bh = kh(rng, nx, D, 0.15)
    p = params(rng, B, D, C, G4)
    bufs = Bufs(dev)
    o = outputs(bufs, B, D, C, G4)
    X8, Xh8 = bufs.out(B, nx, dtype=torch.uint8), bufs.out(B, nx, dtype=torch.uint8)
    oc, oh = bufs.out(B * Tn, Np), bufs.out(B * Tn, Np)
    dv = lambda a: torch.as_tensor(a, device=dev)
    w_out = bufs.out(B, C)
    keep = [dv(cur), dv(hist), dv(idx), T(w_src, dev)]          # alive until the launch: the stage holds pointers
    g = ops.label_stage((keep[0], nx, 0, None), (keep[1], nx, 0, None), keep[2], 0, None, None, None, D, D, keep[3], w_out,
                        bytes_out=(X8, Xh8))
    x_call(B, D, C, G4, None, nx, nx, T(Kh, dev), T(bh, dev), p, o, dev, stage=g,
           proj=(Tn, Np, T(Kc, dev), oc, T(Kh_, dev), oh))
    torch.cuda.synchronize()
    assert np.array_equal(X8.cpu().numpy(), want['X8']) and np.array_equal(Xh8.cpu().numpy(), want['Xh8'])
    assert np.array_equal(N(w_out), want['w_out'])
    for got, fr, K, name in ((oc, want['X'], Kc, 'out_cur'), (oh, want['Xh8'].astype(np.float64), Kh_, 'out_hist')):
        fr = fr.reshape(B * Tn, D)
        err = np.abs(N(got) - fr @ K)
        bound = LR.BOUND_K * LR.U * (np.abs(fr) @ np.abs(K))
        assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
        _REPORT['ratios'][name] = max(_REPORT['ratios'].get(name, 0.0), float((err / np.maximum(bound, 1e-300)).max()))
    p['onehot'] = want['w_out']
    ref = LR.forward(p['Ka'], p['ba'], p['eps'], p['onehot'], p['prior'], p['Kenc_w'], p['benc'], p['Kdec_w'], p['bdec'],
                     X=want['X'], Kh=Kh, bh=bh)
    check(o, ref, 'front')
    bufs.check_canaries()


# ---- f: in-kernel noise ----
@pytest.mark.parametrize("C", [4, 10])
def test_label_draws_its_own_noise(dev, C):
    """eps drawn in the kernel is the Philox normal at (seed, step + *step_dev, stream, first + b (C-1) + j): ops.philox_normal
    bit for bit, oracle/philox.py to libm precision; the outputs match the reference fed that eps"""
    from clvae_amd import ops
    B, D, G4, Tn = 7, 88, 352, 3
    C1 = C - 1
    seed, stream, step, first = 0x9876543210AB, 5, 3, (1 << 32) + 12345
    rng = np.random.default_rng(C)
    nx = Tn * D
    p = params(rng, B, D, C, G4)
    X = window(rng, B, nx)
    Kh, bh = kh(rng, nx, D)
    bufs = Bufs(dev)
    o = outputs(bufs, B, D, C, G4)
    o['eps'] = bufs.out(B, C1)
    it = torch.tensor([2], dtype=torch.int32, device=dev)
    nz = ops.noise_draw(seed, stream, first, step - 2, it)
    x_call(B, D, C, G4, T(X, dev), nx, nx, T(Kh, dev), T(bh, dev), p, o, dev, noise=nz)
    dref = torch.empty(B * C1, dtype=torch.float32, device=dev)
    ops.philox_normal(dref, B * C1, seed, step, stream, first)
    torch.cuda.synchronize()
    assert torch.equal(o['eps'].reshape(-1), dref)
    want = OP.normal(B * C1, seed, step=step, stream_id=stream, first_index=first).reshape(B, C1)
    np.testing.assert_allclose(N(o['eps']), want, atol=2e-5)
    p['eps'] = N(o['eps'])
    ref = LR.forward(p['Ka'], p['ba'], p['eps'], p['onehot'], p['prior'], p['Kenc_w'], p['benc'], p['Kdec_w'], p['bdec'],
                     X=X, Kh=Kh, bh=bh)
    check(o, ref, 'noise')
    bufs.check_canaries()


# ---- g: label edge rows ----
@pytest.mark.parametrize("C", [3, 32])
def test_label_edge_rows(dev, C):
    """Ka = ba = 0, so W = softmax([eps, 0]): rows with eps = 0 tie exactly (W = 1/C; hit by the first index), an all-zero
    onehot row, eps = +-40 saturating W so that w_rec clips at both ends; prior = 0.7"""
    from clvae_amd import ops
    B, D, G4 = 8, 6, 352
    rng = np.random.default_rng(C + 100)
    p = params(rng, B, D, C, G4, prior=0.7)
    p['Ka'], p['ba'] = np.zeros_like(p['Ka']), np.zeros_like(p['ba'])
    p['eps'][0] = 0.0
    p['onehot'][0] = np.eye(C)[0]              # tie, hit 1
    p['eps'][1] = 0.0
    p['onehot'][1] = np.eye(C)[C - 1]          # tie, hit 0 (the last index would say 1)
    p['onehot'][2] = 0.0                       # no label: w_rec 0, hit = (argmax W == 0)
    p['eps'][3] = -40.0
    p['onehot'][3] = np.eye(C)[C - 1]          # n[C-1] ~ 1: clipped at 1 - 1e-7
    p['eps'][4] = 0.0
    p['eps'][4, 0] = -40.0
    p['onehot'][4] = np.eye(C)[0]              # n[0] ~ e^-40: clipped at 1e-7
    hW = f32(np.maximum(rng.standard_normal((B, D)), 0))
    bufs = Bufs(dev)
    o = outputs(bufs, B, D, C, G4)
    a = label_args(p, o, dev)
    ops.vrnn_label_fwd(B, D, C, G4, T(hW, dev), T(p['Ka'], dev), T(p['ba'], dev), a['eps'], a['onehot'], a['prior'],
                       a['Kenc_w'], a['benc'], a['Kdec_w'], a['bdec'], o['wargs'], o['W'], o['rowloss'], o['rb_enc'],
                       o['rb_dec'])
    torch.cuda.synchronize()
    ref = LR.forward(p['Ka'], p['ba'], p['eps'], p['onehot'], p['prior'], p['Kenc_w'], p['benc'], p['Kdec_w'], p['bdec'],
                     hW=hW)
    o['hW'] = T(hW, dev)
    check(o, ref, 'edges')
    rl = N(o['rowloss'])
    assert (N(o['W'])[:2] == N(o['W'])[0, 0]).all()          # exact ties
    assert rl[0, 2] == 1.0 and rl[1, 2] == 0.0 and rl[2, 1] == 0.0
    n = (ref['W'] + 1e-10) / (ref['W'] + 1e-10).sum(1, keepdims=True)
    assert n[3, C - 1] > 1 - 1e-7 and n[4, 0] < 1e-7
    np.testing.assert_allclose(rl[4, 1], -(C - 1) * np.log(np.float32(1e-7)), rtol=1e-6)
    bufs.check_canaries()


# ---- h: clv_vrnn_label_bwd ----
@pytest.mark.parametrize("B,D,C", [(1, 1, 2), (7, 3, 17), (300, 88, 10), (7, 128, 32), (7, 2, 3)])
def test_label_bwd(dev, B, D, C):
    """G4 = 400 > LH_T: the dW loop strides twice; without the layer gradient, with it at once, and deferred (bit for bit);
    dhW masked by the same hW on both sides (exact zeros in it)"""
    from clvae_amd import ops
    G4, C1 = 400, C - 1
    rng = np.random.default_rng(B * 5 + D + C)
    wargs = f32(rng.standard_normal((B, 2 * C1)) * 0.5)
    eps = f32(rng.standard_normal((B, C1)))
    W = f32(LR.O.logistic_normal(wargs[:, :C1], wargs[:, C1:], eps))
    hW = f32(np.maximum(rng.standard_normal((B, D)), 0))
    lab = dict(Kenc_w=f32(rng.standard_normal((C, G4)) * 0.1), Kdec_w=f32(rng.standard_normal((C, G4)) * 0.1), wargs=wargs,
               eps=eps, onehot=np.eye(C)[rng.integers(0, C, B)], W=W, hW=hW, Ka=f32(rng.standard_normal((D, 2 * C1)) * 0.2),
               prior=0.2, class_weight=0.8, w_kl_weight=0.9, inv_b=1.0 / B)
    dze, dzd = f32(rng.standard_normal((B, G4))), f32(rng.standard_normal((B, G4)))
    d = {k: T(v, dev) if isinstance(v, np.ndarray) else v for k, v in lab.items()}
    bufs = Bufs(dev)

    def run(layer_grad, defer):
        o = dict(dwargs=bufs.out(B, 2 * C1), dhW=bufs.out(B, D))
        o['lg'] = (bufs.out(D, 2 * C1), bufs.out(2 * C1)) if layer_grad else None
        rq = ops.ReduceQueue(dev) if defer else None
        ops.vrnn_label_bwd(B, D, C, G4, T(dze, dev), T(dzd, dev), d['Kenc_w'], d['Kdec_w'], d['wargs'], d['eps'], d['onehot'],
                           d['W'], d['hW'], d['Ka'], lab['prior'], lab['class_weight'], lab['w_kl_weight'], lab['inv_b'],
                           o['dwargs'], o['dhW'], layer_grad=o['lg'], ws=ops.Workspace(dev), defer=rq)
        if rq is not None:
            rq.flush()
        return o

    o0, o1, o2 = run(False, False), run(True, False), run(True, True)
    torch.cuda.synchronize()
    want = LR.label_backward(dze, dzd, *[lab[k] for k in ('Kenc_w', 'Kdec_w', 'wargs', 'eps', 'onehot', 'W', 'hW', 'Ka',
                                                         'prior', 'class_weight', 'w_kl_weight', 'inv_b')])
    for k in ('dwargs', 'dhW'):
        for o in (o0, o1, o2):
            g = N(o[k])
            np.testing.assert_allclose(g, want[k], rtol=1e-4, atol=1e-5 * max(np.abs(want[k]).max(), 1e-30), err_msg=k)
            LR.assert_close_sliced(g, want[k], (0, 1), 1e-6 * max(np.abs(want[k]).max(), 1e-30), SLICE_RTOL, name=k)
        assert torch.equal(o0[k], o1[k]) and torch.equal(o1[k], o2[k]), k
    assert (N(o0['dhW'])[hW == 0] == 0).all()
    for a, b2, k in zip(o1['lg'], o2['lg'], ('dKa', 'dba')):
        assert torch.equal(a, b2), k
        g = N(a)
        np.testing.assert_allclose(g, want[k], rtol=1e-4, atol=1e-5 * max(np.abs(want[k]).max(), 1e-30), err_msg=k)
        LR.assert_close_sliced(g.reshape(len(g), -1), want[k].reshape(len(g), -1), (0, 1) if g.ndim == 2 else (0,),
                               1e-6 * max(np.abs(want[k]).max(), 1e-30), SLICE_RTOL, name=k)
    bufs.check_canaries()
