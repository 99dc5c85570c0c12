"""GPU tests of key tracking against tests/keytrack_reference.py: clv_key_track_windows element by element
within label_reference's BOUND_K budget (K = 0 and K = 3), its bitwise independence of batch, hop and piece order,
clv_key_track_smooth against the log-space reference HMM, and keytrack.track / keys.py end to end for both families."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import keytrack_reference as KR
from helpers import ROOT, Bufs, write_jsb_pickle
from oracle import philox as OP

pytestmark = pytest.mark.gpu

D = 88
SHAPES = [(1, 12, 5), (4, 88, 2), (32, 88, 18), (32, 88, 32)]          # (T, Hd, C): cl_vae's head, then cl_vrnn's
EPS_TOL = 2e-5          # tests/test_gpu_ops.py's tolerance on clv_philox_normal
_REPORT = {}


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    yield torch.device("cuda:0")
    print("\nkey tracking: worst error / bound: %s" % ", ".join("%s %.3g" % kv for kv in sorted(_REPORT.items())))


_CASES = {}


def case(T, Hd, C):
    """seeded weights at Glorot scale and the seven pieces of a shape; built once, never changed"""
    key = (T, Hd, C)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * T + 10 * Hd + C)
        f32 = lambda a: np.ascontiguousarray(a, np.float32)
        glorot = lambda m, n: f32(rng.uniform(-1, 1, (m, n)) * np.sqrt(6.0 / (m + n)))
        NA = 2 * (C - 1)
        w = dict(Kh=glorot(T * D, Hd), bh=f32(rng.uniform(-0.1, 0.1, Hd)), Ka=glorot(Hd, NA), ba=f32(rng.uniform(-0.1, 0.1, NA)))
        lengths = [T - 1, T, T + 1, 63, 64, 65, 200]
        pieces = [(rng.random((P, D)) < 0.05).astype(np.uint8) for P in lengths]
        pieces[3][:] = 1                     # every note on in every frame: the densest window, the longest sum
        pieces[4][:] = 0                     # all rests: hW = relu(bh)
        _CASES[key] = (w, pieces)
    return _CASES[key]


_REFS = {}


def reference(T, Hd, C, hop):
    """per piece (wargs, b_wargs, logp, b_logp) of the fp64 reference; computed once per (shape, hop)"""
    key = (T, Hd, C, hop)
    if key not in _REFS:
        w, pieces = case(T, Hd, C)
        w64 = {k: v.astype(np.float64) for k, v in w.items()}
        out = []
        for p in pieces:
            X, _ = KR.windows(p, T, hop)
            if X.shape[0] == 0:
                out.append((np.zeros((0, 2 * (C - 1))),) * 2 + (np.zeros((0, C)),) * 2)
                continue
            wa, bwa = KR.head(X, w64['Kh'], w64['bh'], w64['Ka'], w64['ba'])
            lp, blp = KR.logp0(wa, bwa)
            out.append((wa, bwa, lp, blp))
        _REFS[key] = out
    return _REFS[key]


def run_windows(dev, w, pieces, T, Hd, C, hop, K=0, seed=0, piece0=0, win_off=None):
    """-> (wargs [Wtot, NA], logp [Wtot, C], win_off); NaN-filled outputs with canaries behind them"""
    from clvae_amd import ops
    lengths = [p.shape[0] for p in pieces]
    counts = [KR.n_windows(P, T, hop) for P in lengths]
    po = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    wo = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64) if win_off is None else np.asarray(win_off, np.int64)
    Wtot = int(sum(counts))
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    roll = np.concatenate(pieces, 0) if sum(lengths) else np.zeros((1, D), np.uint8)
    B = Bufs(dev)
    wargs, logp = B.out(max(Wtot, 1), 2 * (C - 1)), B.out(max(Wtot, 1), C)
    ops.key_track_windows(len(pieces), T, D, Hd, C, hop, K, t(roll), t(po), t(wo), t(w['Kh']), t(w['bh']), t(w['Ka']), t(w['ba']),
                          seed, piece0, wargs, logp)
    torch.cuda.synchronize()
    B.check_canaries()
    return wargs.cpu().numpy()[:Wtot], logp.cpu().numpy()[:Wtot], wo


def _ratio(got, ref, bound):
    e = np.abs(np.asarray(got, np.float64) - ref)
    return float(np.nan_to_num(e / np.maximum(bound, 1e-300), nan=np.inf).max()) if e.size else 0.0


def _note(name, v):
    _REPORT[name] = max(_REPORT.get(name, 0.0), v)


@pytest.mark.parametrize("T,Hd,C", SHAPES)
def test_windows_kernel_within_its_bounds(dev, T, Hd, C):
    """every element of wargs and logp (K = 0) within its own bound, for hop in 1, 2, 3, T"""
    w, pieces = case(T, Hd, C)
    for hop in sorted({1, 2, 3, T}):
        wargs, logp, wo = run_windows(dev, w, pieces, T, Hd, C, hop)
        ref = reference(T, Hd, C, hop)
        assert wo[-1] == sum(r[0].shape[0] for r in ref) and ref[0][0].shape[0] == 0 and ref[1][0].shape[0] == 1
        for n, (wa, bwa, lp, blp) in enumerate(ref):
            rows = slice(wo[n], wo[n + 1])
            ra, rl = _ratio(wargs[rows], wa, bwa), _ratio(logp[rows], lp, blp)
            print("T %d Hd %d C %d hop %d piece %d (%d rows): wargs %.3g, logp %.3g of the bound" % (T, Hd, C, hop, n, wa.shape[0], ra, rl))
            _note('wargs', ra)
            _note('logp', rl)
            assert ra <= 1.0 and rl <= 1.0, (T, Hd, C, hop, n, ra, rl)
        np.testing.assert_allclose(np.exp(logp.astype(np.float64)).sum(1), 1.0, atol=1e-5)


def device_eps(dev, pieces, T, hop, C, K, seed, piece0=0):
    """eps [K, Wtot, C-1] from clv_philox_normal at the documented stream, step and index: one draw per (piece, k) over the
    piece's index range, sliced at its windows"""
    from clvae_amd import ops
    out = []
    for k in range(K):
        rows = []
        for n, p in enumerate(pieces):
            J = KR.n_windows(p.shape[0], T, hop)
            if J == 0:
                continue
            first, cnt = KR.eps_index(piece0 + n, 0, 0), ((J - 1) * hop + 1) * 32
            buf = torch.empty(cnt, dtype=torch.float32, device=dev)
            ops.philox_normal(buf, cnt, seed, step=k, stream_id=KR.KEY_STREAM, first_index=first)
            got = buf.cpu().numpy()
            np.testing.assert_allclose(got, OP.normal(cnt, seed, k, KR.KEY_STREAM, first), atol=EPS_TOL)
            rows.append(got.reshape(-1, 32)[::hop][:J, :C - 1])
        out.append(np.concatenate(rows, 0))
    return np.stack(out)


@pytest.mark.parametrize("T,Hd,C", SHAPES)
def test_windows_kernel_with_label_samples(dev, T, Hd, C):
    """K = 3: the reference is fed the device's own wargs and the eps clv_philox_normal gives"""
    w, pieces = case(T, Hd, C)
    K, seed, hop = 3, 0x5EED0123456, 1
    wargs, logp, wo = run_windows(dev, w, pieces, T, Hd, C, hop, K=K, seed=seed, piece0=5)
    wargs0, _, _ = run_windows(dev, w, pieces, T, Hd, C, hop)
    assert np.array_equal(wargs, wargs0)                    # the samples do not touch wargs
    eps = device_eps(dev, pieces, T, hop, C, K, seed, piece0=5)
    lp, b = KR.logpK(wargs, eps, eps_tol=EPS_TOL)
    r = _ratio(logp, lp, b)
    print("T %d Hd %d C %d K %d: logp %.3g of the bound" % (T, Hd, C, K, r))
    _note('logp_K3', r)
    assert r <= 1.0
    # another seed, another piece number: other noise
    _, other, _ = run_windows(dev, w, pieces, T, Hd, C, hop, K=K, seed=seed, piece0=6)
    assert not np.array_equal(other, logp)


@pytest.mark.parametrize("T,Hd,C", SHAPES)
@pytest.mark.parametrize("K", [0, 3])
def test_windows_are_bitwise_independent_of_the_launch(dev, T, Hd, C, K):
    w, pieces = case(T, Hd, C)
    seed = 77
    wargs, logp, wo = run_windows(dev, w, pieces, T, Hd, C, 1, K=K, seed=seed)
    # every piece alone, under its global number
    for n, p in enumerate(pieces):
        wa1, lp1, _ = run_windows(dev, w, [p], T, Hd, C, 1, K=K, seed=seed, piece0=n)
        assert np.array_equal(wa1, wargs[wo[n]:wo[n + 1]]) and np.array_equal(lp1, logp[wo[n]:wo[n + 1]]), n
    # hop 2 = every second row of hop 1 (also through another tile position)
    wargs2, logp2, wo2 = run_windows(dev, w, pieces, T, Hd, C, 2, K=K, seed=seed)
    for n in range(len(pieces)):
        assert np.array_equal(wargs2[wo2[n]:wo2[n + 1]], wargs[wo[n]:wo[n + 1]][::2]), n
        assert np.array_equal(logp2[wo2[n]:wo2[n + 1]], logp[wo[n]:wo[n + 1]][::2]), n
    # the pieces in another order, their rows where they were (K = 0: the noise follows the piece's number)
    if K == 0:
        perm = [6, 2, 4, 0, 5, 1, 3]
        wo_perm = np.concatenate([wo[perm], [wo[-1]]])
        wa3, lp3, _ = run_windows(dev, w, [pieces[i] for i in perm], T, Hd, C, 1, win_off=wo_perm)
        assert np.array_equal(wa3, wargs) and np.array_equal(lp3, logp)


# --------------------------------------------------------------------------------------------------------- smoothing
def smooth_case(C):
    rng = np.random.default_rng(50 + C)
    Js = [1, 2, 65, 1000, 0]
    rows = []
    for J in Js:
        lp = np.log(rng.dirichlet(np.ones(C), J)).astype(np.float32).reshape(J, C)
        sharp = rng.random(J) < 0.3
        win = rng.integers(0, C, J)
        for j in np.flatnonzero(sharp):
            lp[j] = -80.0
            lp[j, win[j]] = 0.0
        rows.append(lp)
    prior = rng.dirichlet(np.ones(C) * 3)
    trans = 0.9 * KR.sticky(C, 1, 16) + 0.1 * rng.dirichlet(np.ones(C), C)
    return Js, rows, prior, trans


def run_smooth(dev, C, rows, log_prior, log_trans, kappa):
    from clvae_amd import ops
    Js = [r.shape[0] for r in rows]
    wo = np.concatenate([[0], np.cumsum(Js)]).astype(np.int64)
    Wtot, N = int(wo[-1]), len(rows)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
    B = Bufs(dev)
    post, ev, pp = B.out(Wtot, C, dtype=torch.float64), B.out(N, dtype=torch.float64), B.out(N, C, dtype=torch.float64)
    path = torch.full((Wtot + 64,), -7, dtype=torch.int32, device=dev)
    ops.key_track_smooth(N, C, t(wo), t(np.concatenate(rows, 0)), None if log_prior is None else t(log_prior), t(log_trans), kappa,
                         post, path, ev, pp)
    torch.cuda.synchronize()
    B.check_canaries()
    assert (path[Wtot:] == -7).all()
    return post.cpu().numpy(), path[:Wtot].cpu().numpy(), ev.cpu().numpy(), pp.cpu().numpy(), wo


@pytest.mark.parametrize("C", [2, 5, 32])
@pytest.mark.parametrize("kappa", [1.0, 0.25])
def test_smoothing_kernel_against_the_reference(dev, C, kappa):
    """one launch of N = 5 pieces with J = 1, 2, 65, 1000 and 0 rows, 30 % of the rows one-hot-sharp"""
    Js, rows, prior, trans = smooth_case(C)
    for log_prior in (np.log(prior), None):
        post, path, ev, pp, wo = run_smooth(dev, C, rows, log_prior, np.log(trans), kappa)
        for n, lp in enumerate(rows):
            ref = KR.smooth(lp, log_prior, np.log(trans), kappa)
            np.testing.assert_allclose(pp[n], ref['piece_post'], rtol=0, atol=1e-8)
            if lp.shape[0] == 0:
                assert ev[n] == 0.0
                continue
            sl = slice(wo[n], wo[n + 1])
            np.testing.assert_allclose(post[sl], ref['post'], rtol=0, atol=1e-8)
            assert abs(ev[n] - ref['log_evidence']) <= 1e-10 * abs(ref['log_evidence']), (n, ev[n], ref['log_evidence'])
            score = KR.path_score(path[sl], lp, log_prior, np.log(trans), kappa)
            assert abs(score - ref['best']) <= 1e-9, (n, score, ref['best'])
            _note('post_abs_err', float(np.abs(post[sl] - ref['post']).max()))
        again = run_smooth(dev, C, rows, log_prior, np.log(trans), kappa)
        for a, b in zip((post, path, ev, pp), again[:4]):
            assert np.array_equal(a, b)                       # bitwise reproducible


# -------------------------------------------------------------------------------------------------------- end to end
def _model(dev, family):
    if family == 'cl_vae':
        from clvae_amd.cl_vae.model import get_model
        model, _ = get_model(4, D, (88, 2), (12, 5), 'adam-wn', seed=3, device=dev)
        g = lambda n: [a.astype(np.float64) for a in model.get_layer(n).get_weights()]
        (Kh, bh), (Km, bm), (Kv, bv) = g('h_w'), g('w_mean'), g('w_log_var')
        return model, 1, dict(Kh=Kh, bh=bh, Ka=np.concatenate([Km, Kv], 1), ba=np.concatenate([bm, bv]))
    from clvae_amd.cl_vrnn.model import get_model
    model, _ = get_model(4, D, 88, 2, 4, 5, True, 'adam-wn', seed=3, device=dev)
    g = lambda n: [a.astype(np.float64) for a in model.get_layer(n).get_weights()]
    (Kh, bh), (Ka, ba) = g('hW'), g('Wargs')
    return model, 4, dict(Kh=Kh, bh=bh, Ka=Ka, ba=ba)


@pytest.mark.parametrize("family", ['cl_vae', 'cl_vrnn'])
def test_track_end_to_end(dev, family):
    from clvae_amd import keytrack, vary
    model, T, w = _model(dev, family)
    C = 5
    rng = np.random.default_rng(8)
    pieces = [(rng.random((P, D)) < 0.06).astype(np.float64) for P in (40, T, 57, max(T - 1, 1), 88)]
    for hop in (1, T, 3):
        kt = keytrack.track(model, pieces, hop=hop, expected_segment=24)
        A, kappa = KR.sticky(C, hop, 24), min(1.0, hop / T)
        mean_p, b_mean = [], []
        for n, p in enumerate(pieces):
            X, starts = KR.windows(p, T, hop)
            assert np.array_equal(kt.starts[n], starts) and kt.lengths[n] == p.shape[0]
            if X.shape[0] == 0:
                assert kt.wargs[n].shape == (0, 2 * (C - 1)) and kt.segments(n) == [(kt.key(n), 0, p.shape[0])]
                np.testing.assert_allclose(kt.piece_post[n], 1.0 / C, atol=1e-12)
                continue
            wa, bwa = KR.head(X, w['Kh'], w['bh'], w['Ka'], w['ba'])
            lp, blp = KR.logp0(wa, bwa)
            assert _ratio(kt.wargs[n], wa, bwa) <= 1.0 and _ratio(kt.logp[n], lp, blp) <= 1.0
            ref = KR.smooth(kt.logp[n], None, np.log(A), kappa)        # the HMM on the rows the device produced
            np.testing.assert_allclose(kt.post[n], ref['post'], rtol=0, atol=1e-8)
            np.testing.assert_allclose(kt.piece_post[n], ref['piece_post'], rtol=0, atol=1e-8)
            assert abs(kt.log_evidence[n] - ref['log_evidence']) <= 1e-10 * abs(ref['log_evidence'])
            assert abs(KR.path_score(kt.path[n], kt.logp[n], None, np.log(A), kappa) - ref['best']) <= 1e-9
            assert KR.segments_cover(kt.segments(n), p.shape[0])
            assert kt.key(n) == int(np.argmax(kt.piece_post[n]))
            mean_p.append(np.exp(lp).mean(0))
            b_mean.append((np.exp(lp) * np.expm1(blp)).mean(0))      # |e^(lp + d) - e^lp| <= e^lp (e^|d| - 1)
        if hop == T:
            # the label head's own average by two routes: this launch, and vary.infer_labels' batch-1 host loop
            full = [n for n, p in enumerate(pieces) if p.shape[0] >= T]
            got = kt.labels(soft=True)[full]
            old = vary.infer_labels(model, [pieces[n] for n in full])
            bound = 2 * np.asarray(b_mean)                   # each route within the budget of the same fp32 contract
            assert (np.abs(got - np.asarray(mean_p)) <= np.asarray(b_mean)).all()
            assert (np.abs(got - old) <= bound).all(), float((np.abs(got - old) / bound).max())
            hard = kt.labels()
            assert hard.shape == (len(pieces), C) and (hard.sum(1) == 1).all()
    # samples > 0 runs, and the noise is the seed's
    a = keytrack.track(model, pieces, samples=2, seed=4)
    b = keytrack.track(model, pieces, samples=2, seed=4)
    c = keytrack.track(model, pieces, samples=2, seed=5)
    assert np.array_equal(a.logp[0], b.logp[0]) and not np.array_equal(a.logp[0], c.logp[0])
    assert np.array_equal(a.wargs[0], c.wargs[0])


@pytest.mark.parametrize("family", ['cl_vae', 'cl_vrnn'])
def test_keys_tool_on_the_jsb_fixture(dev, tmp_path, family):
    from clvae_amd.keytrack import split_songs
    data = write_jsb_pickle('all', str(tmp_path / "jsb.pickle"))
    rolls, keys, key_map = split_songs(data, 'test')
    C = len(key_map)
    assert 2 <= C <= 32 and len(rolls) == len(keys) > 0
    if family == 'cl_vae':
        from clvae_amd.cl_vae.model import get_model
        model, _ = get_model(4, D, (88, 2), (24, C), 'adam-wn', seed=1, device=dev)
        margs = dict(batch_size=4, original_dim=D, intermediate_dim=88, latent_dim=2, intermediate_class_dim=24, n_classes=C,
                     class_weight=1.0, use_x_prev=False, optimizer='adam-wn')
    else:
        from clvae_amd.cl_vrnn.model import get_model
        model, _ = get_model(4, D, 88, 2, 8, C, True, 'adam-wn', seed=1, device=dev)
        margs = dict(batch_size=4, original_dim=D, intermediate_dim=88, latent_dim=2, seq_length=8, n_classes=C, class_weight=1.0,
                     use_x_prev=True, optimizer='adam-wn')
    model.save_weights(str(tmp_path / "m.h5"))
    json.dump(margs, open(str(tmp_path / "m.json"), 'w'))
    out = str(tmp_path / "keys.json")
    script = os.path.join(ROOT, 'classifying-vae-lstm_amd', family, 'keys.py')
    r = subprocess.run([sys.executable, script, 'k', '-i', str(tmp_path / "m.h5"), '--train_file', data, '--hop', '2', '--out', out],
                       capture_output=True, text=True, timeout=240, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.load(open(out))
    assert res['n_songs'] == len(rolls) and res['split'] == 'test' and res['hop'] == 2
    assert 0.0 <= res['accuracy'] <= 1.0 and 0.0 <= res['modulating'] <= 1.0
    conf = np.asarray(res['confusion'])
    assert conf.shape == (C, C) and conf.sum() == len(rolls)
    assert abs(res['accuracy'] - np.trace(conf) / conf.sum()) < 1e-12
    assert [res['key_names'].index(s['key']) for s in res['songs']] == keys
    for s, roll in zip(res['songs'], rolls):
        assert KR.segments_cover([(k, f, n) for k, f, n in s['segments']], roll.shape[0])
    assert "key accuracy" in r.stdout and "confusion" in r.stdout
