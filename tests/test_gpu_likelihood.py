"""-m gpu: the importance-weighted log-likelihood: csrc/iw_eval.hip against numpy fp64, the whole estimate
against an fp64 oracle loop with the documented noise keying, its invariants, two ranks, Model.evaluate and the two
evaluate CLIs."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import make_synthetic_pickle
from likelihood_case import vrnn_case
from oracle import clvae_oracle as O
from oracle import philox as OP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELBO_TOL = 1e-3          # nats per frame


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _lse(a, axis=0):
    m = a.max(axis=axis)
    return m + np.log(np.exp(a - m).sum(axis=axis))


def _figures(lw):
    """lw [K, n] -> (log_p, elbo, ess) per window, fp64"""
    K = lw.shape[0]
    m = lw.max(axis=0)
    e = np.exp(lw - m)
    return _lse(lw) - math.log(K), lw.mean(axis=0), e.sum(0) ** 2 / (e ** 2).sum(0)


# ------------------------------------------------------------------ 1. the kernel against numpy fp64
@pytest.mark.parametrize("T", [1, 16, 128])
@pytest.mark.parametrize("L", [2, 32])
@pytest.mark.parametrize("C1", [0, 9])
def test_accumulate_and_finish_match_numpy_fp64(dev, T, L, C1):
    from clvae_amd import ops
    R, nvalid, K, prior = 37, 29, 7, -0.75
    rng = np.random.default_rng(T * 1000 + L * 10 + C1)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    state0 = np.empty((R, 4))
    state0[:, 0], state0[:, 1:] = -np.inf, 0.0
    state0[nvalid:] = rng.standard_normal((R - nvalid, 4))          # padding rows: anything, and they must stay so
    state = torch.as_tensor(state0, device=dev)
    counter = torch.tensor([5], dtype=torch.int32, device=dev)
    lws = []
    for k in range(K):
        # log weights near -1e4, hundreds of nats apart between the samples of a window
        nll = (1e4 / T + rng.uniform(-300, 300, (R, 1)) / T + rng.uniform(0, 1, (R, T))).astype(np.float32)
        za = np.concatenate([f(R * T, L), 0.5 * f(R * T, L)], axis=1)
        ez = f(R * T, L)
        wa = np.concatenate([f(R, C1), 0.5 * f(R, C1)], axis=1)
        ew = f(R, C1)
        t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)
        ops.iw_accumulate(R, T, L, C1, t(nll.ravel()), t(za), t(ez), t(wa), t(ew), prior, nvalid, state, counter)
        # numpy fp64
        d = lambda a: a.astype(np.float64)
        mz, lvz, e = d(za[:, :L]), d(za[:, L:]), d(ez)
        z = mz + np.exp(0.5 * lvz) * e
        lz = (0.5 * (lvz + e * e - z * z)).reshape(R, T * L).sum(1)
        mw, lvw, ewd = d(wa[:, :C1]), d(wa[:, C1:]), d(ew)
        s = mw + np.exp(0.5 * lvw) * ewd
        pr = float(np.float32(prior))
        lwt = (0.5 * (lvw + ewd * ewd - pr - s * s / math.exp(pr))).sum(1)
        lws.append(-d(nll).sum(1) + lz + lwt)
    out = torch.full((3, R), float('nan'), dtype=torch.float64, device=dev)
    ops.iw_finish(R, nvalid, K, state, out[0], out[1], out[2])
    torch.cuda.synchronize()
    lw = np.stack(lws)[:, :nvalid]
    assert lw.min() < -9e3 and (lw.max(0) - lw.min(0)).min() > 50
    want = _figures(lw)
    got = out.cpu().numpy()
    for g, w, name in zip(got, want, ('log_p', 'elbo', 'ess')):
        assert np.isfinite(g[:nvalid]).all(), name
        np.testing.assert_allclose(g[:nvalid], w, rtol=1e-9, atol=0, err_msg=name)
        assert np.isnan(g[nvalid:]).all(), name          # rows >= nvalid are not written
    st = state.cpu().numpy()
    assert np.array_equal(st[nvalid:].view(np.uint64), state0[nvalid:].view(np.uint64))
    assert int(counter.item()) == 5 + K


def test_a_nan_weight_makes_its_window_nan(dev):
    from clvae_amd import ops
    R, T, L = 3, 4, 2
    nll = torch.ones(R * T, device=dev)
    za, ez = torch.zeros(R * T, 2 * L, device=dev), torch.zeros(R * T, L, device=dev)
    state = torch.zeros(R, 4, dtype=torch.float64, device=dev)
    state[:, 0] = -math.inf
    for k in range(3):
        nll[T + 1] = float('nan') if k == 1 else 1.0          # window 1, sample 1
        ops.iw_accumulate(R, T, L, 0, nll, za, ez, None, None, 0.0, R, state)
    out = torch.empty(3, R, dtype=torch.float64, device=dev)
    ops.iw_finish(R, R, 3, state, out[0], out[1], out[2])
    o = out.cpu().numpy()
    assert np.isnan(o[:, 1]).all() and np.isfinite(o[:, [0, 2]]).all()
    np.testing.assert_allclose(o[0, [0, 2]], -T, rtol=1e-12)


# ------------------------------------------------------------------ 2. the whole estimate against an fp64 oracle
def _iw_streams():
    from clvae_amd.trainer import IW_STREAM_W, IW_STREAM_Z
    return IW_STREAM_W, IW_STREAM_Z


def _oracle_vrnn(p, cfg, X, Xp, K, seed, prior=0.0):
    n, T, _ = X.shape
    C1, L = cfg['C'] - 1, cfg['L']
    sw, sz = _iw_streams()
    lw = np.empty((K, n))
    for k in range(K):
        eW = OP.normal(n * C1, seed, step=k, stream_id=sw).reshape(n, C1).astype(np.float64)
        eZ = OP.normal(n * T * L, seed, step=k, stream_id=sz).reshape(n, T, L).astype(np.float64)
        c = O.vrnn_forward(p, cfg, X, Xp, eW, eZ)
        nll, _ = O.bce_from_logits_keras(c['logits'], X)
        lz = 0.5 * (c['Z_log_var'] + eZ ** 2 - c['Z'] ** 2)
        s = c['W_mean'] + np.exp(c['W_log_var'] / 2) * eW
        lwt = 0.5 * (c['W_log_var'] + eW ** 2 - prior - s ** 2 / math.exp(prior))
        lw[k] = -nll.sum(1) + lz.sum((1, 2)) + lwt.sum(1)
    return _figures(lw)


def _oracle_vae(p, cfg, x, K, seed, prior=0.0):
    n = x.shape[0]
    C1, L = cfg['C'] - 1, cfg['L']
    sw, sz = _iw_streams()
    lw = np.empty((K, n))
    for k in range(K):
        ew = OP.normal(n * C1, seed, step=k, stream_id=sw).reshape(n, C1).astype(np.float64)
        ez = OP.normal(n * L, seed, step=k, stream_id=sz).reshape(n, L).astype(np.float64)
        c = O.vae_forward(p, cfg, x, None, ew, ez)
        nll, _ = O.bce_from_logits_keras(c['logits'], x)
        lz = 0.5 * (c['z_log_var'] + ez ** 2 - c['z'] ** 2)
        s = c['w_mean'] + np.exp(c['w_log_var'] / 2) * ew
        lwt = 0.5 * (c['w_log_var'] + ew ** 2 - prior - s ** 2 / math.exp(prior))
        lw[k] = -nll + lz.sum(1) + lwt.sum(1)
    return _figures(lw)


def _check_against(r, want, T):
    got = r['windows']
    for name, w in zip(('log_p', 'elbo'), want[:2]):
        d = np.abs(got[name] - w)
        assert d.max() <= ELBO_TOL * T, (name, d.max())
    np.testing.assert_allclose(got['ess'], want[2], rtol=0.05, atol=0.05)
    assert r['n_windows'] == len(want[0]) and r['k'] == 5
    assert r['log_likelihood'] == pytest.approx(got['log_p'].mean(), rel=1e-12)
    assert r['log_likelihood_per_frame'] == pytest.approx(got['log_p'].mean() / T, rel=1e-12)


@pytest.mark.parametrize("path,B,T,L,H", [('pair', 32, 16, 2, 88), ('generic', 32, 16, 2, 64), ('mx', 768, 3, 12, 88)])
def test_cl_vrnn_estimate_matches_the_oracle_loop(dev, path, B, T, L, H):
    model, x, y, (p, cfg, X, Xp, _) = vrnn_case(dev, B=B, T=T, L=L, H=H)
    eng = model.engine
    assert {'pair': eng.fuse_pair, 'generic': not (eng.fuse_pair or eng.use_mx), 'mx': eng.use_mx}[path]
    r = model.log_likelihood(x, y, k=5, seed=3, per_window=True)
    _check_against(r, _oracle_vrnn(p, cfg, X, Xp, 5, 3), T)


@pytest.mark.parametrize("fused", [True, False])
def test_cl_vae_estimate_matches_the_oracle_loop(dev, fused):
    from clvae_amd.cl_vae.model import get_model
    B, L, C, n = 32, 4, 3, 45
    model, _ = get_model(B, 88, (88, L), (88, C), 'adam', seed=4, device=dev)
    model.engine.fused = fused and model.engine.fused
    assert model.engine.fused == fused
    cfg = O.vae_config(latent_dim=L, n_classes=C)
    p = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in O.vae_init_params(cfg, seed=4).items()}
    model.engine.P.set_weights(p)
    rng = np.random.default_rng(1)
    x = (rng.random((n, 88)) < 0.08).astype(np.float64)
    wt = np.eye(C)[rng.integers(0, C, n)]
    r = model.log_likelihood(x, [x, wt, wt, x], k=5, seed=3, per_window=True)
    _check_against(r, _oracle_vae(p, cfg, x, 5, 3), 1)


# ------------------------------------------------------------------ 3. invariants
def test_bounds_graph_equals_eager_and_batch_size_does_not_matter(dev):
    model, x, y, _ = vrnn_case(dev, B=32)
    g = model.log_likelihood(x, y, k=6, seed=9, per_window=True)['windows']
    e = model.log_likelihood(x, y, k=6, seed=9, per_window=True, use_graph=False)['windows']
    for name in g:
        assert np.array_equal(g[name], e[name]), name
    assert (g['log_p'] >= g['elbo'] - 1e-9 * np.abs(g['elbo'])).all()
    assert (g['ess'] >= 1 - 1e-9).all() and (g['ess'] <= 6 + 1e-9).all()
    m64, x64, y64, _ = vrnn_case(dev, B=64)
    w64 = m64.log_likelihood(x64, y64, k=6, seed=9, per_window=True)['windows']
    np.testing.assert_allclose(w64['log_p'], g['log_p'], rtol=1e-5, atol=0)


def test_training_state_is_left_alone(dev):
    """Parameters, `iterations`, the step's graphs and bound batches, the last loss means: unchanged; and the next fit epoch
    is bit for bit the epoch it would have been without the estimate in between."""
    runs = []
    for with_estimate in (False, True):
        model, x, y, _ = vrnn_case(dev, B=16, n=48)
        model.fit(x, y, shuffle=False, epochs=1, batch_size=16, verbose=0)
        ts = model._step
        before = (model.engine.P.get_weights(), int(model.engine.P.iterations.item()), ts._graphs, ts._bound,
                  model.engine.scal.clone())
        if with_estimate:
            model.log_likelihood(x, y, k=3, seed=1)
            after = model.engine.P.get_weights()
            for k in before[0]:
                assert np.array_equal(before[0][k], after[k]), k
            assert int(model.engine.P.iterations.item()) == before[1]
            assert model._step is ts and ts._graphs is before[2] and ts._bound is before[3]
            assert torch.equal(model.engine.scal, before[4])
        h = model.fit(x, y, shuffle=False, epochs=1, batch_size=16, verbose=0)
        runs.append((h.history, model.engine.P.get_weights()))
    assert runs[0][0] == runs[1][0]
    for k in runs[0][1]:
        assert np.array_equal(runs[0][1][k], runs[1][1][k]), k


# ------------------------------------------------------------------ 4. two ranks
def test_two_ranks_return_the_one_rank_estimate(dev, tmp_path):
    here = os.path.dirname(os.path.abspath(__file__))
    out = str(tmp_path / "ll%d.npz")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.join(here, "dp_worker_likelihood.py"), out], env=env))
    for pr in procs:
        assert pr.wait(timeout=300) == 0
    r0, r1 = np.load(out % 0), np.load(out % 1)
    model, x, y, _ = vrnn_case(dev, B=8)
    ref = model.log_likelihood(x, y, k=5, seed=3, per_window=True)['windows']
    for name in ref:
        assert np.array_equal(r0[name], r1[name]), name
    np.testing.assert_allclose(r0['log_p'], ref['log_p'], rtol=1e-5, atol=0)
    np.testing.assert_allclose(r0['elbo'], ref['elbo'], rtol=1e-5, atol=0)


# ------------------------------------------------------------------ 5. evaluate()
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_evaluate_equals_the_last_validation_entries(dev, which):
    rng = np.random.default_rng(2)
    if which == 'cl_vrnn':
        model, x, y, _ = vrnn_case(dev, B=16, n=48)
        xv, yv = [a[:32] for a in x], [a[:32] for a in y]
    else:
        from clvae_amd.cl_vae.model import get_model
        model, _ = get_model(16, 88, (88, 2), (88, 3), 'adam-wn', seed=5, device=dev)
        xa = (rng.random((48, 88)) < 0.08).astype(np.float64)
        wt = np.eye(3)[rng.integers(0, 3, 48)]
        x, y = xa, [xa, wt, wt, xa]
        xv, yv = xa[:32], [xa[:32], wt[:32], wt[:32], xa[:32]]
    h = model.fit(x, y, shuffle=False, epochs=2, batch_size=16, verbose=0, validation_data=(xv, yv))
    got = model.evaluate(xv, yv)
    want = [h.history['val_' + m][-1] for m in model.metrics_names]
    assert len(model.metrics_names) == 6 and model.metrics_names[0] == 'loss'
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7)
    with pytest.raises(ValueError):
        model.evaluate(xv[:20] if which == 'cl_vae' else [a[:20] for a in xv], [a[:20] for a in yv])


# ------------------------------------------------------------------ 6. the CLIs end to end
@pytest.mark.parametrize("which,extra", [('cl_vae', ['--latent_dim', '2', '--batch_size', '50']),
                                         ('cl_vrnn', ['--use_x_prev', '--seq_length', '8', '--batch_size', '20'])])
def test_evaluate_cli_end_to_end(dev, tmp_path, which, extra):
    import importlib
    TR = importlib.import_module('clvae_amd.%s.train' % which)
    data = make_synthetic_pickle(str(tmp_path / "syn.pickle"), n_songs=(10, 4, 4), seed=3)
    mdir = str(tmp_path / "models")
    os.makedirs(mdir)
    args = TR.build_parser().parse_args(['r', '--num_epochs', '2', '--train_file', data, '--model_dir', mdir] + extra)
    np.random.seed(0)
    TR.train(args)
    model_file = os.path.join(mdir, 'r.h5')
    assert os.path.exists(model_file)
    script = os.path.join(ROOT, 'classifying-vae-lstm_amd', which, 'evaluate.py')
    outs = []
    for i in range(2):
        out = str(tmp_path / ("ll%d.json" % i))
        r = subprocess.run([sys.executable, script, 'e', '-i', model_file, '--train_file', data, '-k', '4', '--seed', '11',
                            '--out', out], capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs.append(open(out).read())
    assert outs[0] == outs[1]
    res = json.loads(outs[0])
    assert res['split'] == 'test' and res['k'] == 4 and res['n_windows'] > 0
    for key in ('log_likelihood', 'log_likelihood_per_frame', 'elbo', 'ess'):
        assert math.isfinite(res[key]), key
    assert res['log_likelihood'] >= res['elbo']
    assert len(res['evaluate']) == 6 and all(math.isfinite(v) for v in res['evaluate'].values())
