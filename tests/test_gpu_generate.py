"""-m gpu: the two persistent sampling kernels (csrc/generate.hip: vrnn_generate_kernel, csrc/vae_generate.hip:
vae_generate_kernel) launched directly through ops.vrnn_* / ops.vae_* with weight tensors, every output against the fp64
reference of tests/generate_reference.py, per element and per frame.

The reference runs ALONG THE LAUNCH'S OWN PATH: after the launch the input of every frame is known exactly (a seed or
source frame, the bridge sample [u <= x_hat], Xs[:, t-1] after its roll, a state's row), the noise is what
clv_philox_normal / clv_philox_uniform write for the kernels' (seed, step, stream, index), and then
  * z_mean, z_log_var, z (vary_latents), the x_hat of every frame and the returned state (resume) lie within
    bound_t = 4 x max |ref32_t - ref64_t| of the float64 reference, per output and per frame (generate_reference.check);
  * Xs is exact: [u <= x_hat_device] on free notes, the roll on clamped ones;
  * z equals fma(exp(lv / 2), fl(Tz eps), mean) of the launch's own mean and log-variance within z's bound.
Every output (Xs, x_hat, zout, the states) is NaN before the launch and followed by canaries (helpers.Bufs).

Template instances and the case that launches each (generate_reference.make_case(family, mode, k); hs = hard sigmoid,
s = sigmoid; narrow: L <= 16, wide: L > 16; the tail names the flags CL, TP, VR, ZO, ZG, ST that are set).  All 40 ran in one
kernel-trace pass over this file:
  vrnn<hs,narrow,TAIL>   test_launch_against_fp64[cl_vrnn-MODE-0] (L = 1), [cl_vrnn-MODE-4] (L = 16)
  vrnn<hs,wide,TAIL>     ... [cl_vrnn-MODE-1] (L = 17)
  vrnn<s,narrow,TAIL>    ... [cl_vrnn-MODE-2] (L = 2)
  vrnn<s,wide,TAIL>      ... [cl_vrnn-MODE-3] (L = 32), [cl_vrnn-MODE-5] (L = 17)
      MODE -> TAIL:  plain -> none (clv_vrnn_generate), CL -> CL (a roll), TP -> TP (tempered, no roll), CL+TP -> CL,TP
      (tempered with a roll), vary -> CL,TP,VR (clv_vrnn_vary), vary_latents -> CL,TP,VR,ZO (with a zout), decode -> CL,TP,VR,ZG
      (clv_vrnn_decode), resume -> CL,TP,ST (clv_vrnn_generate from / to a state; the wide ones are the RBL variant)
  vae<TAIL>              ... [cl_vae-MODE-0 .. 5], the same eight modes through the clv_vae_* entry points
  N = 260 (more workgroups than CUs)  ... [cl_vrnn-vary_latents-1-big], [cl_vrnn-resume-3-big], [cl_vae-...-big]
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import generate_reference as GR
import temper_reference as TR
from helpers import Bufs

pytestmark = pytest.mark.gpu

D, H = GR.D, GR.H
CASES = GR.all_cases()


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    return torch.device("cuda:0")


def T(a, dev, dtype=np.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def device_noise(c, dev):
    """the case's eps and u as the device's own generators write them"""
    from clvae_amd import ops

    def draw(fn):
        def f(n, seed, step, stream_id):
            out = torch.empty(n, dtype=torch.float32, device=dev)
            fn(out, n, seed, step=step, stream_id=stream_id)
            return out.cpu().numpy()
        return f
    return GR.noise(c, draw(ops.philox_normal), draw(ops.philox_uniform))


def weights(c, p, dev):
    """(encoder half, decoder half) in the order ops.vrnn_* / ops.vae_* take them"""
    L = c['L']
    if c['which'] == 'cl_vrnn':
        Ke, Kd = T(p['encoder_h/kernel'], dev), T(p['decoder_h/kernel'], dev)
        off = D if c['use_x_prev'] else 0
        enc = (Ke, Ke[D:], T(p['encoder_h/bias'], dev), T(p['encoder_h/recurrent_kernel'], dev),
               T(np.concatenate([p['Z_mean/kernel'], p['Z_log_var/kernel']], 1), dev),
               T(np.concatenate([p['Z_mean/bias'], p['Z_log_var/bias']]), dev))
        dec = (Kd if c['use_x_prev'] else None, Kd[off:off + L], Kd[off + L:], T(p['decoder_h/bias'], dev),
               T(p['decoder_h/recurrent_kernel'], dev), T(p['X_decoded_mean/kernel'], dev), T(p['X_decoded_mean/bias'], dev))
        return enc, dec
    enc = (T(p['h/kernel'], dev), T(p['h/bias'], dev), T(np.concatenate([p['z_mean/kernel'], p['z_log_var/kernel']], 1), dev),
           T(np.concatenate([p['z_mean/bias'], p['z_log_var/bias']]), dev))
    dec = (T(p['decoder_h/kernel'], dev), T(p['decoder_h/bias'], dev), T(p['x_decoded_mean/kernel'], dev),
           T(p['x_decoded_mean/bias'], dev))
    return enc, dec


def launch(c, p, dev, xhat=True, state_out='second'):
    """one launch of the case's entry point on NaN-filled outputs with canaries behind them -> the outputs as float32 arrays.
    state_out: None, 'second' (a buffer of its own) or 'alias' (state_in itself).  (A resume case with t0 = 0 and no state
    either way is a call without a state: state_out=None then launches the case's CL / TP instance.)"""
    from clvae_amd import ops
    vrnn, mode = c['which'] == 'cl_vrnn', c['mode']
    N, S, ns, L, C = c['N'], c['S'], c['nsteps'], c['L'], c['C']
    Tn = S + ns
    bufs = Bufs(dev)
    enc, dec = weights(c, p, dev)
    Xs = bufs.out(N, ns, D) if ns > 0 else None
    xh = bufs.out(N, Tn, D) if xhat else None
    temper = None if c['temper'] is None else tuple(float(v) for v in TR.factors(*c['temper']))
    clamp = T(c.get('clamp'), dev, np.uint8)
    w = T(c['w'], dev)
    gate = (0 if c['gate'] == 'hard_sigmoid' else 1,) if vrnn else (c['use_x_prev'],)
    got, zout, st_out = {}, None, None
    if mode in GR.GENERATE_MODES or mode == 'resume':
        state = {}
        if mode == 'resume':
            st_in = bufs.inp(c['state_in']) if c.get('state_in') is not None else None
            assert state_out != 'alias' or st_in is not None
            st_out = None if state_out is None else st_in if state_out == 'alias' else bufs.out(N, 5 if vrnn else 2, D)
            state = dict(t0=c['t0'], state_in=st_in, state_out=st_out)
        if vrnn:
            ops.vrnn_generate(N, S, ns, D, H, L, C, gate[0], c['z_prior'], c['seed'], T(c.get('seeds'), dev), w, *enc, *dec, Xs, xh,
                              clamp=clamp, temper=temper, **state)
        else:
            ops.vae_generate(N, ns, D, H, L, C, c['use_x_prev'], c['z_prior'], c['seed'], T(c.get('seeds'), dev), w, *enc, *dec, Xs,
                             xh, clamp=clamp, temper=temper, **state)
    elif mode in ('vary', 'vary_latents'):
        zout = bufs.out(3, N, Tn, L) if mode == 'vary_latents' else None
        head = (N, Tn, D, H, L, C, gate[0], c['hist_source'], c['seed'], T(c['sources'], dev), T(c.get('x0'), dev), w,
                T(c['w_dec'], dev), *enc, *dec, Xs)
        (ops.vrnn_vary if vrnn else ops.vae_vary)(*head, xhat=xh, clamp=clamp, temper=temper, zout=zout)
    else:
        f = ops.vrnn_decode if vrnn else ops.vae_decode
        f(N, Tn, D, H, L, C, gate[0], c['seed'], T(c['z_in'], dev), T(c.get('x0'), dev), T(c.get('history'), dev), T(c['w_dec'], dev),
          T(c.get('noise_rows'), dev, np.int32), *dec, Xs, xhat=xh, clamp=clamp, inv_T=1.0 if temper is None else temper[0])
    torch.cuda.synchronize()
    bufs.check_canaries()
    n = lambda t: None if t is None else t.cpu().numpy()
    got = dict(Xs=n(Xs), xhat=n(xh), zout=n(zout), state=n(st_out))
    for k, v in got.items():
        assert v is None or np.isfinite(v).all(), (k, "an element was not written")
    return got


@pytest.mark.parametrize("c", CASES, ids=lambda c: c['id'])
def test_launch_against_fp64(dev, c):
    p = GR.params_of(c)
    eps, u = device_noise(c, dev)
    got = launch(c, p, dev)
    ratio, ref_dev, wrong = GR.check(c, p, eps, u, got)
    print("%s %s: device / bound %s; smallest reference deviation %s; inexact %s"
          % (c['id'], GR.instance_of(c), {k: float('%.3g' % v) for k, v in ratio.items()},
             {k: float('%.2g' % v) for k, v in ref_dev.items()}, wrong))
    assert all(v > 0 for v in ref_dev.values()), ref_dev
    assert not any(wrong.values()), wrong
    assert all(v <= 1 for v in ratio.values()), ratio
    if c['mode'] == 'resume':
        # state_out absent, a second buffer, state_in itself: the same frames bit for bit, the latter two the same state
        for how in (None, 'alias') if c.get('state_in') is not None else (None,):      # nothing to alias on a zero start
            again = launch(c, p, dev, state_out=how)
            assert np.array_equal(again['xhat'], got['xhat'])
            assert (again['Xs'] is None and got['Xs'] is None) or np.array_equal(again['Xs'], got['Xs'])
            if how == 'alias':
                assert np.array_equal(again['state'], got['state'])
    if c['xhat_none']:
        assert np.array_equal(launch(c, p, dev, xhat=False)['Xs'], got['Xs'])         # xhat=None: the same frames


# ------------------------------------------------------------------------------- cl_vae: frames are read as on / off
def _vae_engine(dev):
    from clvae_amd.engine import VaeEngine
    from oracle import clvae_oracle as O
    cfg = O.vae_config(latent_dim=3, n_classes=4, use_x_prev=True)
    eng = VaeEngine(cfg, 8, dev)
    eng.P.set_weights({k: np.asarray(v, np.float32) for k, v in O.vae_init_params(cfg, seed=6).items()})
    return eng


@pytest.mark.parametrize("persistent", [True, False])
def test_cl_vae_refuses_frames_that_are_not_binary(dev, persistent):
    """a frame entry other than 0 or 1 in any frame array the caller supplies: ValueError on both routes, nothing launched
    (x_hat keeps its NaN fill); a state that a sampler returned is taken as it is"""
    from clvae_amd.engine_generate import GenState
    eng = _vae_engine(dev)
    N, Tn, bufs = 2, 3, Bufs(dev)
    rng = np.random.default_rng(0)
    good = lambda *s: (rng.random(s + (D,)) < 0.06).astype(np.float32)
    bad = lambda *s: np.where(good(*s) > 0, np.float32(0.5), np.float32(0)) + (np.arange(D) == 3) * np.float32(2.0)
    w, z = T(np.eye(4)[[0, 1]], dev), T(rng.standard_normal((N, Tn, 3)), dev)
    xh = bufs.out(N, Tn, D)
    kw = dict(persistent=persistent, xhat_out=xh)
    calls = [lambda: eng.generate(T(bad(N), dev), w, Tn, **kw),
             lambda: eng.generate(T(bad(N), dev), w, Tn, return_state=True, **kw),
             lambda: eng.generate(None, w, Tn, state=GenState.fresh('cl_vae', eng.cfg, dev, seed_frame=T(bad(N), dev)), **kw),
             lambda: eng.generate(None, w, Tn, state=GenState('cl_vae', dict(x_in=T(good(N), dev), hist=T(bad(N), dev)), 0), **kw),
             lambda: eng.vary(T(bad(N, Tn), dev), w, **kw),
             lambda: eng.vary(T(good(N, Tn), dev), w, x0=T(bad(N), dev), **kw),
             lambda: eng.decode_latents(z, w, x0=T(bad(N), dev), **kw),
             lambda: eng.decode_latents(z, w, history=T(bad(N, Tn), dev), **kw),
             lambda: eng.vary(T(np.full((N, Tn, D), np.nan), dev), w, **kw)]
    for call in calls:
        with pytest.raises(ValueError, match="on/off"):
            call()
        torch.cuda.synchronize()
        assert torch.isnan(xh).all()
    bufs.check_canaries()
    # binary frames pass, and the returned state continues without another check
    Xs, st = eng.generate(T(good(N), dev), w, Tn, return_state=True, **kw)
    assert st.binary and (not persistent or not torch.isnan(xh).any())          # the frame chain returns no x_hat here
    eng.generate(None, w, Tn, state=st.clone(), **kw)
