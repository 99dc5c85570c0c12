"""-m gpu: a training pass keeps its state in its own record (engine._Pass), not on the engine -- a finished pass leaves
nothing behind that the next one could read, no attribute appears on an engine while it runs, and grads_tail() without a
pass to finish says so."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import clvae_oracle as O

pytestmark = pytest.mark.gpu

B, T, L, CN, SEED = 16, 10, 2, 10, 808


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


@pytest.fixture(scope="module")
def case(dev):
    """cl_vrnn at B=16, T=10, L=2, C=10: weights, two mini-batches of byte frames, the first one as float arguments"""
    cfg = O.vrnn_config(latent_dim=L, seq_length=T, n_classes=CN, use_x_prev=True)
    rng = np.random.default_rng(5)
    p = {k: f32(v) for k, v in O.vrnn_init_params(cfg, seed=9).items()}
    win = rng.random((2 * B, T + 1, 88)) < 0.05
    keys = np.eye(CN)[rng.integers(0, CN, 2 * B)].astype(np.float32)
    u8 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint8), device=dev)
    ft = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)
    bound = (u8(win[:, 1:].reshape(2 * B, -1)), u8(win[:, :-1].reshape(2 * B, -1)), ft(keys))
    direct = (ft(win[:B, 1:]), ft(win[:B, :-1]), ft(keys[:B]), ft(rng.standard_normal((B, CN - 1))),
              ft(rng.standard_normal((B * T, L))))
    return cfg, p, bound, direct


def _bound_steps(eng, bound):
    """two steps of a TrainStep over the bound byte batches: byte frames, in-kernel noise, the label launch stages the batch"""
    from clvae_amd.trainer import TrainStep
    ts = TrainStep(eng, seed=SEED)
    ts.bind_batches(*bound, idx=None, period=2, stride=eng.B)
    assert ts._label_stage() is not None and eng.folds_noise()
    for _ in range(2):
        ts.step()
    torch.cuda.synchronize()
    assert ts._f8 is not None
    return ts


def _direct(eng, p, direct):
    eng.P.set_weights(p)
    eng.loss_and_grads(*direct)
    torch.cuda.synchronize()
    return eng.scal.clone(), eng.P.grads.clone()


def test_a_pass_leaves_nothing_behind(dev, case):
    """Behind two bound TrainStep steps, a direct loss_and_grads() on float frames with explicit eps gives what it gives on
    a fresh engine.  Exact: every launch of this route sums in a fixed order (no float atomics), and the parent commit
    reproduces P.params, P.grads and the loss means bit for bit from run to run on it."""
    from clvae_amd.engine import VrnnEngine
    cfg, p, bound, direct = case
    used = VrnnEngine(cfg, B, dev)
    used.P.set_weights(p)
    _bound_steps(used, bound)
    fresh = VrnnEngine(cfg, B, dev)
    fresh.frames_exact_bf16 = True          # (what the bound byte batches have told the used engine)
    assert used.frames_exact_bf16
    (s_used, g_used), (s_fresh, g_fresh) = _direct(used, p, direct), _direct(fresh, p, direct)
    assert torch.isfinite(g_fresh).all() and float(g_fresh.abs().max()) > 0
    assert torch.equal(s_used, s_fresh), (s_used, s_fresh)
    assert torch.equal(g_used, g_fresh), float((g_used - g_fresh).abs().max())


def test_no_attribute_appears_during_a_pass(dev, case):
    from clvae_amd.engine import VaeEngine, VrnnEngine
    from clvae_amd.trainer import TrainStep
    cfg, p, bound, direct = case
    eng = VrnnEngine(cfg, B, dev)
    declared = set(vars(eng))
    eng.P.set_weights(p)
    _bound_steps(eng, bound)
    _direct(eng, p, direct)
    assert set(vars(eng)) == declared
    eng.loss_and_grads(*direct, do_tail=False)
    eng.grads_tail(direct[0])
    torch.cuda.synchronize()
    assert set(vars(eng)) == declared
    # cl_vae: a fused step (bound byte batches through TrainStep) and a step of the layer chain
    vcfg = O.vae_config(latent_dim=L, n_classes=CN, use_x_prev=True)
    for fused in (True, False):
        vae = VaeEngine(dict(vcfg, fused_step=fused), B, dev)
        assert bool(vae.fused) == fused
        declared = set(vars(vae))
        vae.P.set_weights({k: f32(v) for k, v in O.vae_init_params(vcfg, seed=3).items()})
        ts = TrainStep(vae, seed=SEED)
        ts.bind_batches(bound[0][:, -88:].contiguous(), bound[1][:, -88:].contiguous(), bound[2], idx=None, period=2, stride=B)
        assert (ts._label_stage() is not None) == fused
        for _ in range(2):
            ts.step()
        torch.cuda.synchronize()
        assert set(vars(vae)) == declared, (fused, set(vars(vae)) ^ declared)


def test_grads_tail_without_a_pending_pass_raises(dev, case):
    from clvae_amd.engine import VrnnEngine
    cfg, p, _, direct = case
    eng = VrnnEngine(cfg, B, dev)
    with pytest.raises(RuntimeError, match="pending pass"):
        eng.grads_tail(direct[0])
    eng.P.set_weights(p)
    eng.loss_and_grads(*direct, do_tail=False)
    eng.grads_tail(direct[0])
    with pytest.raises(RuntimeError, match="pending pass"):
        eng.grads_tail(direct[0])
    eng.loss_and_grads(*direct)             # a whole pass ends itself
    with pytest.raises(RuntimeError, match="pending pass"):
        eng.grads_tail(direct[0])
    torch.cuda.synchronize()
