"""-m gpu: re-decoding a piece on both routes: the VR instances of the persistent kernels (csrc/generate.hip,
csrc/vae_generate.hip) and the frame chains with clv_take_frame, the public calls and the sample tools' --vary.  The
reference is tests/vary_reference.py; the conditions on this file's inputs that need no device (flip cap, logit range, power
and seeds of the keyed enumeration) are asserted in tests/test_vary_reference.py."""
import importlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import test_gpu_clamped_generation as TC
import vary_reference as VR
from helpers import write_jsb_pickle

pytestmark = pytest.mark.gpu

FREE, D = 255, 88
ROUTES = ['persistent', 'chain']


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


_ENGINES = {}


def _engine(dev, which, L, use_x_prev=True, gate='hard_sigmoid', B=8):
    """the engine of VR.case_params (cached per module: building one uploads and packs the weights)"""
    key = (which, L, use_x_prev, gate, B)
    if key not in _ENGINES:
        from clvae_amd.engine import VaeEngine, VrnnEngine
        cfg, p = VR.case_params(which, L, VR.classes_of(which), use_x_prev, gate or 'hard_sigmoid')
        eng = (VrnnEngine if which == 'cl_vrnn' else VaeEngine)(cfg, B, dev)
        eng.P.set_weights(p)
        _ENGINES[key] = (eng, p)
    return _ENGINES[key]


def _t(dev, a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _vary(eng, dev, route, src, w_enc, w_dec=None, x0=None, xhat=True, **kw):
    """engine.vary on numpy inputs by `route`: (Xs, x_hat) as device tensors"""
    src = _t(dev, src)
    xh = torch.full_like(src, float('nan')) if xhat else None
    use_graph = kw.pop('use_graph', True)
    Xs = eng.vary(src, _t(dev, w_enc), _t(dev, w_dec), x0=_t(dev, x0), persistent=route == 'persistent', use_graph=use_graph,
                  xhat_out=xh, **kw)
    torch.cuda.synchronize()
    assert set(torch.unique(Xs).tolist()) <= {0.0, 1.0} and (xh is None or not torch.isnan(xh).any())
    return Xs, xh


def _near_flip(dev, Xa, Xb, xhat, seed, clamp, win):
    """the rule of test_gpu_temperature._agree_until_a_near_flip: both routes satisfy the roll, give the same frames and may
    part only where a free draw lies within `win` of its probability (the frames after that are each route's own)"""
    if clamp is not None:
        TC._check_clamped(Xa, clamp)
        TC._check_clamped(Xb, clamp)
    N = Xa.shape[0]
    for j in range(Xa.shape[1]):
        diff = Xa[:, j] != Xb[:, j]
        if diff.any():
            u = TC._uniform(dev, N, seed, j)
            assert float((u - xhat[:, j]).abs()[diff].max()) < win
            return j
    return None


# ------------------------------------------------------------------ 1. the training identity
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which,L,gate,use_x_prev", VR.IDENTITY_CASES)
def test_source_history_is_the_training_forward_pass(dev, which, L, gate, use_x_prev, route):
    """history='source', w_dec = w_enc, neutral temperatures: x_hat is the training forward pass (the fp64 reference, which
    tests/test_vary_reference.py holds to oracle.vrnn_forward / vae_forward at 1e-12), within the per-note logit tolerance
    of DESIGN.md 2, compared on the logit side"""
    eng, p = _engine(dev, which, L, use_x_prev, gate)
    C = VR.classes_of(which)
    src, x0, w_enc, _ = VR.case_inputs(VR.IDENTITY_N, VR.IDENTITY_T, C)
    _, _, want = VR.vary(which, p, src, w_enc, None, x0=x0, history='source', seed=VR.IDENTITY_SEED, L=L, gate=gate)
    _, xh = _vary(eng, dev, route, src, w_enc, None, x0, history='source', seed=VR.IDENTITY_SEED)
    err = np.abs(VR.logit_of(xh.cpu().numpy()) - want).max()
    print("%s L=%d %s x_prev=%s %s: max |logit - fp64| = %.3e (bound %.0e)" % (which, L, gate, use_x_prev, route, err, VR.LOGIT_TOL))
    assert err < VR.LOGIT_TOL


# ------------------------------------------------------------------ 2. the free-running loop against the reference
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("T,Tz", VR.FREE_RUN_TEMPS)
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_free_running_loop_matches_reference(dev, which, T, Tz, route):
    """history='own' under a roll with about 30 % of the notes clamped and another decoder label: clamped notes exact; a
    free note differs from the fp64 reference only within window(T) of its probability; at most FLIP_CAP such flips (a
    condition on the inputs: tests/test_vary_reference.py)"""
    _, p, src, x0, w_enc, w_dec, clamp, L, seed = VR.free_run_case(which)
    eng, p2 = _engine(dev, which, L)
    assert all(np.array_equal(p[k], p2[k]) for k in p)
    Xs, _ = _vary(eng, dev, route, src, w_enc, w_dec, x0, history='own', seed=seed, clamp=clamp, temperature=T, z_temperature=Tz)
    fol = VR.Follow(Xs.cpu().numpy(), VR.window(T))
    VR.vary(which, p, src, w_enc, w_dec, x0=x0, history='own', seed=seed, L=L, clamp=clamp, T=T, Tz=Tz, follow=fol)
    print("%s %s T=%g Tz=%g: %d flips, %d outside the window of %.1e, %d clamped notes wrong"
          % (which, route, T, Tz, fol.flips, fol.far, fol.win, fol.clamp_wrong))
    assert fol.clamp_wrong == 0
    assert fol.far == 0
    assert fol.flips <= VR.FLIP_CAP
    ref1, _, _ = VR.vary(which, p, src, w_enc, w_enc, x0=x0, history='own', seed=seed, L=L, clamp=clamp, T=T, Tz=Tz)
    assert not np.array_equal(ref1, Xs.cpu().numpy())                    # and it is not the run under the source's key


# ------------------------------------------------------------------ 3. the routes
@pytest.mark.parametrize("with_x0", [True, False])
@pytest.mark.parametrize("Tn", [1, 2, 9])
@pytest.mark.parametrize("N", [1, 4, 300])
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_routes_agree(dev, which, N, Tn, with_x0):
    """the chain captured as a graph equals the chain run eagerly, bit for bit; the persistent kernel and the chain agree
    until a near flip.  N = 300 on the NaN-poisoned memory of the suite: more workgroups than one wave of launches"""
    L, C, seed = (2 if which == 'cl_vrnn' else 3), VR.classes_of(which), 7 + N + Tn
    eng, _ = _engine(dev, which, L, B=304)
    src, x0, w_enc, w_dec = VR.case_inputs(N, Tn, C, data_seed=N + Tn)
    clamp = VR.roll(N, Tn, seed=Tn)
    kw = dict(history='own', seed=seed, clamp=clamp, temperature=0.8, z_temperature=1.25)
    x0[:, 40] = 1.0                         # a sounding note in every row
    x0 = x0 if with_x0 else None
    Xp, xhp = _vary(eng, dev, 'persistent', src, w_enc, w_dec, x0, **kw)
    Xg, xhg = _vary(eng, dev, 'chain', src, w_enc, w_dec, x0, **kw)
    Xe, xhe = _vary(eng, dev, 'chain', src, w_enc, w_dec, x0, use_graph=False, **kw)
    assert torch.equal(Xg, Xe) and torch.equal(xhg, xhe)
    _near_flip(dev, Xp, Xg, xhp, seed, clamp, VR.window(0.8))
    assert float((xhp[:, 0] - xhg[:, 0]).abs().max()) < 2e-5 * 1.25       # frame 0 has no history of samples: the same x_hat
    if with_x0:                             # x0 is read: the decoder's first history
        X0, xh0 = _vary(eng, dev, 'persistent', src, w_enc, w_dec, None, **kw)
        assert not torch.equal(xh0[:, 0], xhp[:, 0])


# ------------------------------------------------------------------ 4. the identities of the definition
def _same_or_near_flip(dev, route, a, b, seed, clamp, win):
    """bit for bit on the chain; on the persistent route the near-flip rule (both runs are the same instance on the same
    inputs there too, so they are in fact equal: the rule is the bound, equality the observation printed)"""
    (Xa, xa), (Xb, xb) = a, b
    if route == 'chain':
        assert torch.equal(Xa, Xb) and torch.equal(xa, xb)
    else:
        _near_flip(dev, Xa, Xb, xa, seed, clamp, win)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_identities(dev, which, route):
    L, C, N, Tn, seed = (2 if which == 'cl_vrnn' else 3), VR.classes_of(which), 5, 7, 19
    eng, _ = _engine(dev, which, L)
    src, x0, w_enc, w_dec = VR.case_inputs(N, Tn, C, data_seed=2)
    win = VR.window(1.0)
    run = lambda **kw: _vary(eng, dev, route, src, kw.pop('w_enc', w_enc), kw.pop('w_dec', w_dec), x0, seed=seed, **kw)
    # a NULL roll is an all-FREE roll
    base = run()
    _same_or_near_flip(dev, route, base, run(clamp=np.full((N, Tn, D), FREE, np.uint8)), seed, None, win)
    if route == 'persistent':               # the same instance on the same inputs: equal outright
        assert torch.equal(base[0], run(clamp=np.full((N, Tn, D), FREE, np.uint8))[0])
    # w_dec=None is w_dec=w_enc; neutral temperatures are the call without them
    _same_or_near_flip(dev, route, run(w_dec=None), run(w_dec=w_enc), seed, None, win)
    _same_or_near_flip(dev, route, base, run(temperature=1.0, z_temperature=1.0), seed, None, win)
    # an all-clamped roll equal to the sources under 'own' gives 'source''s x_hat
    own = run(history='own', clamp=src.astype(np.uint8))
    source = run(history='source')
    assert torch.equal(own[0], _t(dev, src))
    if route == 'chain':
        assert torch.equal(own[1], source[1])
    else:
        assert float((own[1] - source[1]).abs().max()) < 2e-5
    # without use_x_prev, 'own' equals 'source'
    eng2, _ = _engine(dev, which, L, use_x_prev=False)
    a = _vary(eng2, dev, route, src, w_enc, w_dec, x0, history='own', seed=seed)
    b = _vary(eng2, dev, route, src, w_enc, w_dec, x0, history='source', seed=seed)
    _same_or_near_flip(dev, route, a, b, seed, None, win)
    c = _vary(eng2, dev, route, src, w_enc, w_dec, None, history='own', seed=seed)           # and x0 is not read
    _same_or_near_flip(dev, route, a, c, seed, None, win)
    assert not torch.equal(a[1], base[1])


# ------------------------------------------------------------------ 5. labels do what they say
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_each_label_reaches_its_side(dev, which, route):
    L, C, N, Tn, seed = (2 if which == 'cl_vrnn' else 3), VR.classes_of(which), 4, 5, 3
    eng, _ = _engine(dev, which, L)
    src, x0, w_enc, w_dec = VR.case_inputs(N, Tn, C, data_seed=6)
    other = np.roll(w_enc, 2, axis=1)
    run = lambda we, wd: _vary(eng, dev, route, src, we, wd, x0, history='source', seed=seed)[1]
    base = run(w_enc, w_dec)
    assert not torch.equal(run(other, w_dec), base)           # only w_enc changed: z_mean / z_log_var, hence x_hat
    assert not torch.equal(run(w_enc, other), base)           # only w_dec changed
    if route == 'chain' and which == 'cl_vae':                # the chain leaves the last frame's head outputs in eng.zargs
        run(w_enc, w_dec)
        za = eng.zargs[:N].clone()
        run(w_enc, other)
        assert torch.equal(eng.zargs[:N], za)                 # the decoder's label does not reach the encoder
        run(other, w_dec)
        assert not torch.equal(eng.zargs[:N], za)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_keyed_models_follow_w_dec_and_not_w_enc(dev, which, route):
    """the keyed enumerable models (z rows zero: only w_dec reaches the output), 4096 rows of one source per class: the
    frequencies of the 4^4 histories under w_dec = c are within 4 binomial standard errors of the enumeration for that
    class, and identically distributed under a different w_enc"""
    from clvae_amd.engine import VaeEngine, VrnnEngine
    L, C = (2, 10) if which == 'cl_vrnn' else (3, 4)
    cfg, p, keys = VR.keyed_params(which)
    n = VR.KEYED_ROWS
    eng = VrnnEngine(cfg, 4, dev) if which == 'cl_vrnn' else VaeEngine(cfg, n, dev)
    eng.P.set_weights(p)
    src = np.repeat(VR.keyed_source()[None], n, 0)
    label = lambda c: np.eye(C)[np.full(n, c)]
    for c in keys:
        want, _, _ = VR.enumerate_redecoding(which, p, L, C, keys[0], c)
        counts = []
        for c_enc in (keys[0], keys[-1]):
            Xs, _ = _vary(eng, dev, route, src, label(c_enc), label(c), None, xhat=False, seed=VR.KEYED_SEED[which],
                          temperature=VR.KEYED_T)
            Xs = Xs.cpu().numpy()
            assert np.all(Xs[:, :, 2:] == 0)
            got = VR.history_counts(Xs)
            worst = VR.worst_cell(got, want, n)
            print("%s %s w_dec=%d w_enc=%d: worst history %.2f SE" % (which, route, c, c_enc, worst))
            assert worst < 4
            counts.append(got)
        assert np.array_equal(counts[0], counts[1])
        for c2 in keys:                     # and the frequencies tell this key from the others
            if c2 != c:
                assert VR.worst_cell(counts[0], VR.enumerate_redecoding(which, p, L, C, keys[0], c2)[0], n) > 4


# ------------------------------------------------------------------ 6. Tz = 0, T = 1e-3, 'source'
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_cold_sampling_is_the_greedy_reconstruction(dev, which, route):
    """z_temperature = 0 puts z at its mean, temperature = 1e-3 makes every draw the rounding of x_hat(z = mean): the output
    is [x_hat > 0.5] except where the neutral-temperature probability is within window(1e-3) = 0.01 of 0.5 (outside it the
    tempered logit is beyond +-40: probabilities below 1e-17 or their complements)"""
    L, C, N, Tn = (2 if which == 'cl_vrnn' else 3), VR.classes_of(which), 6, 8
    eng, p = _engine(dev, which, L)
    src, x0, w_enc, w_dec = VR.case_inputs(N, Tn, C, data_seed=11)
    Xa, _ = _vary(eng, dev, route, src, w_enc, w_dec, x0, history='source', seed=1, temperature=1e-3, z_temperature=0.0)
    Xb, _ = _vary(eng, dev, route, src, w_enc, w_dec, x0, history='source', seed=2, temperature=1e-3, z_temperature=0.0)
    _, mean_xhat = _vary(eng, dev, route, src, w_enc, w_dec, x0, history='source', seed=1, z_temperature=0.0)
    decided = (mean_xhat - 0.5).abs() >= VR.window(1e-3)
    want = (mean_xhat > 0.5).float()
    assert torch.equal(Xa[decided], want[decided]) and torch.equal(Xb[decided], want[decided])
    _, ref_xhat, _ = VR.vary(which, p, src, w_enc, w_dec, x0=x0, history='source', seed=1, L=L, Tz=0.0)
    assert np.abs(ref_xhat - mean_xhat.cpu().numpy()).max() < 2e-5
    print("%s %s: %.1f %% of the notes decided, %.1f %% of those on" % (which, route, 100 * float(decided.float().mean()),
                                                                       100 * float(want[decided].mean())))
    assert bool(decided.any())


# ------------------------------------------------------------------ 7. refusals through the C ABI
def test_c_abi_refusals(dev):
    from clvae_amd import _lib, ops
    N, Tn = 2, 4
    nan, inf = float('nan'), float('inf')
    src, x0, w_enc, w_dec = (_t(dev, a) for a in VR.case_inputs(N, Tn, 10))
    Xs = torch.zeros(N, Tn, D, device=dev)
    eng, _ = _engine(dev, 'cl_vrnn', 2)
    P, off = eng.P, eng.off
    rows = lambda name, r: P.rows(P.params, name, r)

    def vrnn_call(inv_T=1.0, Tz=1.0, N=N, Tn=Tn, src=src):
        try:
            ops.vrnn_vary(N, Tn, D, 88, 2, 10, eng.gate_act, False, 1, src, x0, w_enc, w_dec, P.p('encoder_h/kernel'),
                          rows('encoder_h/kernel', D), P.p('encoder_h/bias'), P.p('encoder_h/recurrent_kernel'),
                          P.p('Zargs/kernel'), P.p('Zargs/bias'), P.p('decoder_h/kernel'), rows('decoder_h/kernel', off),
                          rows('decoder_h/kernel', off + 2), P.p('decoder_h/bias'), P.p('decoder_h/recurrent_kernel'),
                          P.p('X_decoded_mean/kernel'), P.p('X_decoded_mean/bias'), Xs, None, temper=(inv_T, Tz))
        except _lib.ClvError as e:
            return str(e)
        return None
    ev, _ = _engine(dev, 'cl_vae', 3)
    Pv = ev.P
    w4 = _t(dev, np.eye(4)[[0, 1]])

    def vae_call(inv_T=1.0, Tz=1.0, N=N, Tn=Tn, src=src):
        try:
            ops.vae_vary(N, Tn, D, 88, 3, 4, True, False, 1, src, x0, w4, w4, Pv.p('h/kernel'), Pv.p('h/bias'),
                         Pv.p('zargs/kernel'), Pv.p('zargs/bias'), Pv.p('decoder_h/kernel'), Pv.p('decoder_h/bias'),
                         Pv.p('x_decoded_mean/kernel'), Pv.p('x_decoded_mean/bias'), Xs, None, temper=(inv_T, Tz))
        except _lib.ClvError as e:
            return str(e)
        return None
    for call in (vrnn_call, vae_call):
        assert call(1.25, 0.5) is None and call(1.0, 0.0) is None
        for kw in (dict(inv_T=0.0), dict(inv_T=-1.0), dict(inv_T=nan), dict(inv_T=inf), dict(Tz=-1.0), dict(Tz=nan),
                   dict(Tz=inf), dict(N=0), dict(Tn=0), dict(N=-3), dict(src=None)):
            msg = call(**kw)
            assert msg is not None and '(-1)' in msg, (kw, msg)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    out = torch.full((N, D), -7.0, device=dev)
    lib = _lib.lib()
    for n, T_, D_ in ((0, Tn, D), (N * D, 0, D), (N * D, Tn, 0), (N * D + 1, Tn, D)):
        assert lib.clv_take_frame(n, T_, D_, ops._ptr(src), ops._ptr(counter), ops._ptr(out), ops._stream()) == -1
    # a step outside [0, T) leaves the output as it is; a step inside reads that frame
    for c, want in ((-1, None), (Tn, None), (2, src[:, 2]), (Tn - 1, src[:, Tn - 1])):
        counter.fill_(c)
        out.fill_(-7.0)
        ops.take_frame(N, Tn, D, src, counter, out)
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(out, -7.0) if want is None else want)


# ------------------------------------------------------------------ 8. the public calls and both sample tools
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_public_call_returns_float64_numpy(dev, which):
    M = importlib.import_module('clvae_amd.%s.model' % which)
    from clvae_amd.vary import transfer_key, vary
    C = 4
    if which == 'cl_vrnn':
        model, _ = M.get_model(4, D, 88, 2, 8, C, True, 'adam', seed=1)
    else:
        model, _ = M.get_model(4, D, (88, 2), (88, C), 'adam', use_x_prev=True, seed=1)
    src, x0, w_enc, w_dec = VR.case_inputs(3, 8, C, data_seed=5)
    Xs, xh = M.vary_samples_device(model, src, w_enc, w_dec, x0=x0, seed=3, return_xhat=True)
    assert Xs.dtype == np.float64 and xh.dtype == np.float64 and Xs.shape == xh.shape == (3, 8, D)
    assert set(np.unique(Xs)) <= {0.0, 1.0} and np.all((xh > 0) & (xh < 1))
    again = M.vary_samples_device(model, src, w_enc, w_dec, x0=x0, seed=3)
    assert np.array_equal(again, Xs)
    k = int(np.argmax(w_dec[0]))
    same_key = np.array_equal(w_dec, np.eye(C)[np.full(3, k)])
    out = transfer_key(model, src, k, w=w_enc, x0=x0, seed=3)
    assert out.shape == Xs.shape and (not same_key or np.array_equal(out, Xs))
    np.random.seed(0)
    inferred = vary(model, src, seed=3)                                  # w inferred by the model's own w-encoder
    assert inferred.shape == Xs.shape and set(np.unique(inferred)) <= {0.0, 1.0}


@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_sample_tools_vary_end_to_end(dev, tmp_path, which):
    from clvae_amd.cli import DEVICE_LOOP_FLAGS, HARMONIZE_FLAGS, TEMPERATURE_FLAGS, VARY_FLAGS, parser_for
    from clvae_amd.utils.midi_utils import write_sample
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    TRN = importlib.import_module('clvae_amd.%s.train' % which)
    data = write_jsb_pickle('all', str(tmp_path / "JSB Chorales_all.pickle"))
    mdir = str(tmp_path / "models")
    os.makedirs(mdir)
    extra = ['--latent_dim', '4'] if which == 'cl_vae' else ['--seq_length', '8']
    np.random.seed(0)
    TRN.train(TRN.build_parser().parse_args(['m', '--use_x_prev', '--num_epochs', '2', '--patience', '0', '--train_file', data,
                                             '--model_dir', mdir] + extra))
    parser = parser_for('%s.sample' % which, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS + TEMPERATURE_FLAGS + VARY_FLAGS)
    from clvae_amd.utils.pianoroll import PianoData
    P = PianoData(data, batch_size=1, seq_length=8, squeeze_x=which == 'cl_vae')
    windows = {np.asarray(x, np.float64).reshape(8, -1).tobytes() for x in P.x_test}
    key = sorted(P.key_map)[0]
    assert len(P.key_map) > 1
    outs = []
    for run in ('a', 'b'):
        sdir = str(tmp_path / run)
        os.makedirs(sdir)
        args = parser.parse_args(['v', '-n', '3', '-t', '8', '--seed', '4', '-i', os.path.join(mdir, 'm.h5'), '--train_file',
                                  data, '--sample_dir', sdir, '--vary', '--to_key', key, '--temperature', '0.9'])
        seen = []
        real = S.vary

        def spy(model, sources, w, **kw):
            seen.append((np.asarray(sources), kw))
            return real(model, sources, w, **kw)
        S.vary = spy
        try:
            np.random.seed(3)
            rolls = S.sample(args)
        finally:
            S.vary = real
        assert len(rolls) == 3 and all(r.shape == (8, D) and set(np.unique(r)) <= {0.0, 1.0} for r in rolls)
        assert len(seen) == 1 and seen[0][1]['to_key'] == key and seen[0][1]['temperature'] == 0.9
        files = sorted(os.listdir(sdir))
        assert files == sorted(['v_%d.mid' % j for j in range(3)] + ['v_%d_source.mid' % j for j in range(3)])
        blobs = {f: open(os.path.join(sdir, f), 'rb').read() for f in files}
        assert all(b[:4] == b'MThd' for b in blobs.values())
        # the source file is the test frames that were re-decoded
        half_speed = True
        for j in range(3):
            assert np.asarray(seen[0][0][j], np.float64).tobytes() in windows
            write_sample(seen[0][0][j], sdir, 'check', half_speed)
            assert open(os.path.join(sdir, 'check.mid'), 'rb').read() == blobs['v_%d_source.mid' % j]
        os.remove(os.path.join(sdir, 'check.mid'))
        outs.append(blobs)
    assert outs[0] == outs[1]                                           # the same --seed: identical bytes
