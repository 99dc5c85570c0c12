"""-m gpu: resumable device generation: the ST instances of the persistent kernels (csrc/generate.hip,
csrc/vae_generate.hip), the frame chains started from a state, GenState between the two routes, the public calls, Stream /
modulate and the sample tools' --chunk / --modulate.  A piece cut into chunks must be the piece of one call, bit for bit.
The references are tests/temper_reference.py and tests/resume_reference.py; the condition on the modulation inputs that
needs no device (the flip cap) is asserted in tests/test_resume_reference.py."""
import importlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import resume_reference as RR
import temper_reference as TR
import test_gpu_clamped_generation as TC
from helpers import make_synthetic_pickle

pytestmark = pytest.mark.gpu

D, C, N, NSTEPS, SEED = 88, 10, 3, 9, 4242
SPLITS = [(4, 5), (1, 8)]
TEMPS = [(1.0, 1.0), (0.5, 1.5)]
U32 = 2 ** 32 - 1


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def _same_state(a, b):
    assert a.kind == b.kind and a.t == b.t and a.N == b.N
    for k, v in a.tensors().items():
        assert torch.equal(v, b[k]), k


def _kw(T, Tz, **more):
    return dict(seed=SEED, temperature=T, z_temperature=Tz, **more)


# ------------------------------------------------------------------------------------------------ cl_vrnn, persistent
def _vrnn_call(eng, x_seed, w, nsteps, roll, state=None, return_state=True, **kw):
    """one persistent call -> (Xs, xhat, state); roll: numpy rows for this call's frames, or None"""
    S = 0 if x_seed is None else int(x_seed.shape[1])
    xh = torch.zeros(w.shape[0], S + nsteps, D, device=w.device)
    extra = dict(state=state, return_state=True) if return_state else {}
    out = eng.generate(x_seed, w, nsteps, xhat_out=xh, clamp=roll if nsteps else None, **extra, **kw)
    torch.cuda.synchronize()
    return (out[0], xh, out[1]) if return_state else (out, xh, None)


@pytest.mark.parametrize("T,Tz", TEMPS)
@pytest.mark.parametrize("with_roll", [False, True])
@pytest.mark.parametrize("S", [0, 5])
@pytest.mark.parametrize("use_x_prev", [True, False])
@pytest.mark.parametrize("gate", ['hard_sigmoid', 'sigmoid'])
@pytest.mark.parametrize("L", [2, 19])
def test_split_invariance_and_the_st_instances_vrnn(dev, L, gate, use_x_prev, S, with_roll, T, Tz):
    """1. one call of 9 frames against 4+5, 1+8 and priming + 9: frames, x_hat and every tensor of the final state are
    bit-equal, t is equal.  2. the same call without state / return_state (today's instances) gives the same Xs and x_hat."""
    eng = TC._vrnn(dev, L, use_x_prev, gate, C)
    x_seed, w = TC._inputs(dev, N, S, C, L + S)
    roll = TC._roll(N, NSTEPS, seed=L) if with_roll else None
    cut = lambda a, b: None if roll is None else np.ascontiguousarray(roll[:, a:b])
    kw = _kw(T, Tz)
    Xs, xhat, st = _vrnn_call(eng, x_seed, w, NSTEPS, roll, **kw)
    assert st.t == S + NSTEPS and st.kind == 'cl_vrnn' and st.N == N
    assert set(torch.unique(Xs).tolist()) <= {0.0, 1.0} and 0 < float(Xs.mean()) < 1 and not torch.isnan(xhat).any()
    assert torch.equal(st.x, Xs[:, -1])                     # the next input is the last (clamped) sample
    if with_roll:
        TC._check_clamped(Xs, roll)
    # 2. today's instances (untempered: the plain / CL instance; tempered: the TP one)
    X0, xh0, _ = _vrnn_call(eng, x_seed, w, NSTEPS, roll, return_state=False, **kw)
    assert torch.equal(X0, Xs) and torch.equal(xh0, xhat)
    # 1. the splits
    for a, b in SPLITS:
        Xa, xha, sa = _vrnn_call(eng, x_seed, w, a, cut(0, a), **kw)
        assert sa.t == S + a
        Xb, xhb, sb = _vrnn_call(eng, None, w, b, cut(a, a + b), state=sa, **kw)
        assert torch.equal(torch.cat([Xa, Xb], 1), Xs) and torch.equal(torch.cat([xha, xhb], 1), xhat)
        _same_state(sb, st)
    if S > 0:               # priming: the seed alone, then the 9 frames from the bridge sample
        Xp, xhp, sp = _vrnn_call(eng, x_seed, w, 0, None, **kw)
        assert Xp.shape == (N, 0, D) and sp.t == S
        bridge = (TC._uniform(dev, N, SEED, S - 1) <= xhp[:, S - 1]).float()
        assert torch.equal(sp.x, bridge)                    # the unreturned sample of step S-1
    else:                   # nothing to prime on: the explicit fresh state
        from clvae_amd.engine_generate import GenState
        sp, xhp = GenState.fresh('cl_vrnn', eng.cfg, dev, N=N), xhat[:, :0]
    keep = sp.rows.clone()
    Xb, xhb, sb = _vrnn_call(eng, None, w, NSTEPS, roll, state=sp, **kw)
    assert torch.equal(Xb, Xs) and torch.equal(torch.cat([xhp, xhb], 1), xhat)
    _same_state(sb, st)
    assert torch.equal(sp.rows, keep)                       # a call does not write the state it takes
    # more teacher-forced frames on top of a state: the seed fed in two parts
    if S > 0:
        _, xh1, s1 = _vrnn_call(eng, x_seed[:, :2].contiguous(), w, 0, None, **kw)
        Xc, xh2, s2 = _vrnn_call(eng, x_seed[:, 2:].contiguous(), w, NSTEPS, roll, state=s1, **kw)
        assert torch.equal(Xc, Xs) and torch.equal(torch.cat([xh1, xh2], 1), xhat)
        _same_state(s2, st)


# ------------------------------------------------------------------------------------------------ cl_vrnn, frame chain
@pytest.mark.parametrize("T,Tz", TEMPS)
@pytest.mark.parametrize("with_roll", [False, True])
@pytest.mark.parametrize("S", [0, 5])
@pytest.mark.parametrize("L,gate,use_x_prev", [(2, 'hard_sigmoid', True), (19, 'sigmoid', False)])
def test_split_invariance_on_the_frame_chain_vrnn(dev, L, gate, use_x_prev, S, with_roll, T, Tz):
    """3. persistent=False, graph and eager: outputs and states are bit-equal between the two and across the splits"""
    eng = TC._vrnn(dev, L, use_x_prev, gate, C)
    x_seed, w = TC._inputs(dev, N, S, C, L + S)
    roll = TC._roll(N, NSTEPS, seed=L) if with_roll else None
    cut = lambda a, b: None if roll is None else np.ascontiguousarray(roll[:, a:b])
    runs = []
    for use_graph in (True, False):
        kw = _kw(T, Tz, persistent=False, use_graph=use_graph, return_state=True)
        Xs, st = eng.generate(x_seed, w, NSTEPS, clamp=roll, **kw)
        assert st.t == S + NSTEPS and torch.equal(st.x, Xs[:, -1])
        for a, b in SPLITS:
            Xa, sa = eng.generate(x_seed, w, a, clamp=cut(0, a), **kw)
            Xb, sb = eng.generate(None, w, b, clamp=cut(a, a + b), state=sa, **kw)
            assert torch.equal(torch.cat([Xa, Xb], 1), Xs)
            _same_state(sb, st)
        if S > 0:
            Xp, sp = eng.generate(x_seed, w, 0, **kw)
            Xb, sb = eng.generate(None, w, NSTEPS, clamp=roll, state=sp, **kw)
            assert torch.equal(Xb, Xs)
            _same_state(sb, st)
        runs.append((Xs, st))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0])
    _same_state(runs[0][1], runs[1][1])
    # and without state / return_state the chain is today's
    X0 = eng.generate(x_seed, w, NSTEPS, clamp=roll, **_kw(T, Tz, persistent=False))
    assert torch.equal(X0, runs[0][0])


def _agree_until_a_near_flip(dev, Xp, Xf, xhat, t0, roll, win):
    """the existing rule between two routes: the same frames; they may part only where a free draw lies within `win` of its
    probability (xhat: the first route's, local frames; the uniforms are those of step t0 + j); clamped notes are exact"""
    if roll is not None:
        TC._check_clamped(Xp, roll)
        TC._check_clamped(Xf, roll)
    for j in range(Xp.shape[1]):
        diff = Xp[:, j] != Xf[:, j]
        if diff.any():
            u = TC._uniform(dev, Xp.shape[0], SEED, t0 + j)
            assert float((u - xhat[:, j]).abs()[diff].max()) < win
            return j
    return None


@pytest.mark.parametrize("T,Tz", TEMPS)
@pytest.mark.parametrize("L", [2, 19])
def test_routes_are_interchangeable(dev, L, T, Tz):
    """4. the persistent state after 4 frames continued 5 frames on both routes, and the chain's state likewise"""
    S, a, b = 5, 4, 5
    eng = TC._vrnn(dev, L)
    x_seed, w = TC._inputs(dev, N, S, C, 3)
    roll = TC._roll(N, NSTEPS, seed=9)
    kw = _kw(T, Tz)
    _, _, sp = _vrnn_call(eng, x_seed, w, a, roll[:, :a].copy(), **kw)
    _, sf = eng.generate(x_seed, w, a, clamp=roll[:, :a].copy(), persistent=False, return_state=True, **kw)
    assert sp.t == sf.t == S + a
    for st in (sp, sf):
        Xp, xhat, _ = _vrnn_call(eng, None, w, b, roll[:, a:].copy(), state=st, **kw)
        Xf, _ = eng.generate(None, w, b, clamp=roll[:, a:].copy(), persistent=False, state=st, return_state=True, **kw)
        torch.cuda.synchronize()
        _agree_until_a_near_flip(dev, Xp, Xf, xhat, S + a, roll[:, a:], TR.window(T))


# ------------------------------------------------------------------------------------------------ against fp64
def _case_model(dev, which):
    p = TR.case_params(which)
    if which == 'cl_vrnn':
        from clvae_amd.cl_vrnn import model as M
        c = TR.VRNN_CASE
        model, _ = M.get_model(8, D, 88, c['L'], c['T_len'], c['C'], True, 'adam', seed=c['model_seed'])
    else:
        from clvae_amd.cl_vae import model as M
        c = TR.VAE_CASE
        model, _ = M.get_model(8, D, (88, c['L']), (88, c['C']), 'adam', use_x_prev=True, seed=c['model_seed'])
    model.engine.P.set_weights(p)
    return model, M, p


def test_state_against_fp64(dev):
    """5. a TR.VrnnStepper fed the device's own inputs; its he, ce, hd, cd against the returned state.  The bound is 4 x the
    largest deviation of the float32 stepper from the float64 one on the same inputs (the kernel sums in 4 k-slices and a
    lane tree, not in numpy's order)."""
    model, M, p = _case_model(dev, 'cl_vrnn')
    c = TR.VRNN_CASE
    seeds, w, _ = TR.vrnn_case_inputs()
    S, seed = c['S'], 31
    _, s0 = M.generate_samples_device(model, seeds, 0, w, seed=seed, return_state=True)          # primed: x is the bridge
    Xs, s1 = M.generate_samples_device(model, None, NSTEPS, w, seed=seed, state=s0, return_state=True)
    inputs = np.concatenate([seeds, s0.x.cpu().numpy()[:, None].astype(np.float64), Xs[:, :-1]], 1)
    assert inputs.shape[1] == S + NSTEPS and np.array_equal(s1.x.cpu().numpy(), Xs[:, -1])
    st64 = TR.VrnnStepper(p, w, seed, c['L'])
    st32 = TR.VrnnStepper(p, w, seed, c['L'], dtype=np.float32)
    names = (('he', 'h_enc'), ('ce', 'c_enc'), ('hd', 'h_dec'), ('cd', 'c_dec'))
    ref_dev = got_dev = 0.0
    for t in range(S + NSTEPS):
        st64.step(t, inputs[:, t])
        st32.step(t, inputs[:, t])
        ref_dev = max([ref_dev] + [float(np.abs(getattr(st32, a).astype(np.float64) - getattr(st64, a)).max()) for a, _ in names])
        if t + 1 in (S, S + NSTEPS):
            dev_state = s0 if t + 1 == S else s1
            assert dev_state.t == t + 1
            got_dev = max([got_dev] + [float(np.abs(dev_state[k].cpu().numpy().astype(np.float64) - getattr(st64, a)).max())
                                       for a, k in names])
    print("state against fp64: device %.3e, float32 reference %.3e (bound 4 x = %.3e)" % (got_dev, ref_dev, 4 * ref_dev))
    assert ref_dev > 0
    assert got_dev <= 4 * ref_dev


@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_modulation_against_fp64(dev, which):
    """6. modulate() with two labels, 5 + 6 frames, against the stepper whose .w is replaced at the boundary"""
    from clvae_amd.stream import modulate
    model, M, p = _case_model(dev, which)
    _, seeds, w, L, gen = RR.case(which)
    plan, seed = RR.plan_of(w), RR.MOD_SEED[which]
    n0, n1 = RR.PLAN_FRAMES
    out = modulate(model, seeds, plan, seed=seed)
    assert out.shape == (seeds.shape[0], n0 + n1, D) and out.dtype == np.float64
    fol = TR.Follow(out, TR.window(1.0))
    gen(p, seeds, plan, seed, L, follow=fol)
    print("%s: %d flips, %d outside the window of %.1e, %d clamped notes wrong" % (which, fol.flips, fol.far, fol.win,
                                                                                  fol.clamp_wrong))
    assert fol.far == 0
    assert fol.clamp_wrong == 0
    assert fol.flips <= TR.FLIP_CAP
    plain = M.generate_samples_device(model, seeds, n0 + n1, w, seed=seed)
    assert np.array_equal(out[:, :n0], plain[:, :n0])
    assert not np.array_equal(out[:, n0:], plain[:, n0:])


# ------------------------------------------------------------------------------------------------ fork
@pytest.mark.parametrize("persistent", [True, False])
def test_fork(dev, persistent):
    """7. state.select([0, 0, 1]): row 0 continues like sequence 0; row 1 shares its prefix state and differs from it"""
    S, a, b = 5, 4, 5
    eng = TC._vrnn(dev, 2)
    x_seed, w = TC._inputs(dev, N, S, C, 7)
    kw = dict(seed=SEED, persistent=persistent, return_state=True)
    _, st = eng.generate(x_seed, w, a, **kw)
    Xu, su = eng.generate(None, w, b, state=st, **kw)
    sel = st.select([0, 0, 1])
    assert sel.t == st.t and torch.equal(sel.rows[1], st.rows[0]) and torch.equal(sel.rows[2], st.rows[1])
    Xf, sf = eng.generate(None, w[[0, 0, 1]].contiguous(), b, state=sel, **kw)
    torch.cuda.synchronize()
    assert torch.equal(Xf[0], Xu[0])
    for k, v in sf.tensors().items():
        assert torch.equal(v[0], su[k][0]), k
    assert not torch.equal(Xf[1], Xf[0])                    # the same prefix under the noise of index 1
    _, su2 = eng.generate(None, w, b, state=st, **kw)       # and the unforked state is still good for the same continuation
    _same_state(su2, su)


# ------------------------------------------------------------------------------------------------ cl_vae
@pytest.mark.parametrize("T,Tz", TEMPS)
@pytest.mark.parametrize("with_roll", [False, True])
@pytest.mark.parametrize("persistent", [True, False])
@pytest.mark.parametrize("use_x_prev", [True, False])
@pytest.mark.parametrize("L", [3, 32])
def test_split_invariance_and_the_st_instance_vae(dev, L, use_x_prev, persistent, with_roll, T, Tz):
    """8. items 1 - 3 for cl_vae: splits against one call on the persistent kernel and on the chain (graph and eager),
    today's instances against the ST one, and the state after a chunk is (Xs[:, -1], Xs[:, -2])"""
    from clvae_amd.engine_generate import GenState
    Cv = 4
    eng = TC._vae(dev, L=L, C=Cv, use_x_prev=use_x_prev)
    x_seed, w = TC._inputs(dev, N, None, Cv, L)
    roll = TC._roll(N, NSTEPS, seed=L) if with_roll else None
    cut = lambda a, b: None if roll is None else np.ascontiguousarray(roll[:, a:b])
    runs = []
    for use_graph in ((True,) if persistent else (True, False)):
        kw = _kw(T, Tz, persistent=persistent, use_graph=use_graph)

        def call(seed_frame, nsteps, clamp, state=None, return_state=True):
            xh = torch.zeros(N, nsteps, D, device=dev) if persistent else None
            extra = dict(state=state, return_state=True) if return_state else {}
            out = eng.generate(seed_frame, w, nsteps, xhat_out=xh, clamp=clamp, **extra, **kw)
            torch.cuda.synchronize()
            xh = xh if persistent else torch.zeros(N, nsteps, 0, device=dev)
            return (out[0], xh, out[1]) if return_state else (out, xh, None)

        Xs, xhat, st = call(x_seed, NSTEPS, roll)
        assert st.kind == 'cl_vae' and st.t == NSTEPS and 0 < float(Xs.mean()) < 1
        assert torch.equal(st.x_in, Xs[:, -1]) and torch.equal(st.hist, Xs[:, -2])
        if with_roll:
            TC._check_clamped(Xs, roll)
        X0, xh0, _ = call(x_seed, NSTEPS, roll, return_state=False)           # today's launches
        assert torch.equal(X0, Xs) and torch.equal(xh0, xhat)
        for a, b in SPLITS:
            Xa, xha, sa = call(x_seed, a, cut(0, a))
            assert sa.t == a and torch.equal(sa.x_in, Xa[:, -1]) and torch.equal(sa.hist, Xa[:, -2] if a > 1 else x_seed)
            Xb, xhb, sb = call(None, b, cut(a, a + b), state=sa)
            assert torch.equal(torch.cat([Xa, Xb], 1), Xs) and torch.equal(torch.cat([xha, xhb], 1), xhat)
            _same_state(sb, st)
        fresh = GenState.fresh('cl_vae', eng.cfg, dev, seed_frame=x_seed)   # a fresh start: x_in = hist = seed, t = 0
        keep = fresh.rows.clone()
        Xb, xhb, sb = call(None, NSTEPS, roll, state=fresh)
        assert torch.equal(Xb, Xs) and torch.equal(xhb, xhat) and torch.equal(fresh.rows, keep)
        _same_state(sb, st)
        runs.append((Xs, st))
    if len(runs) == 2:
        assert torch.equal(runs[0][0], runs[1][0])
        _same_state(runs[0][1], runs[1][1])


def test_routes_are_interchangeable_vae(dev):
    a, b, T = 4, 5, 0.5
    eng = TC._vae(dev)
    x_seed, w = TC._inputs(dev, N, None, 4, 4)
    roll = TC._roll(N, NSTEPS, seed=11)
    kw = _kw(T, 1.5)
    _, sp = eng.generate(x_seed, w, a, clamp=roll[:, :a].copy(), return_state=True, **kw)
    _, sf = eng.generate(x_seed, w, a, clamp=roll[:, :a].copy(), persistent=False, return_state=True, **kw)
    for st in (sp, sf):
        xhat = torch.zeros(N, b, D, device=dev)
        Xp, _ = eng.generate(None, w, b, clamp=roll[:, a:].copy(), xhat_out=xhat, state=st, return_state=True, **kw)
        Xf, _ = eng.generate(None, w, b, clamp=roll[:, a:].copy(), persistent=False, state=st, return_state=True, **kw)
        torch.cuda.synchronize()
        _agree_until_a_near_flip(dev, Xp, Xf, xhat, a, roll[:, a:], TR.window(T))


# ------------------------------------------------------------------------------------------------ Stream
@pytest.mark.parametrize("which", ['cl_vrnn', 'cl_vae'])
def test_stream(dev, which):
    """9. three advance calls with changing temperature and a roll equal the generate_samples_device calls chained by hand;
    a state saved with to_numpy and restored continues like the state itself; fork"""
    from clvae_amd.engine_generate import GenState
    from clvae_amd.stream import Stream
    model, M, _ = _case_model(dev, which)
    _, seeds, w, L, _ = RR.case(which)
    n = seeds.shape[0]
    w2 = RR.second_label(w)
    steps = [(4, None, dict()), (3, TC._roll(n, 3, seed=1), dict(temperature=0.7, z_temperature=0.5)),
             (5, TC._roll(n, 5, seed=2), dict(temperature=1.3))]
    s = Stream(model, seeds, w, seed=23)
    assert s.N == n and s.t == (seeds.shape[1] if which == 'cl_vrnn' else 0)
    got = [s.advance(4), s.advance(3, clamp=steps[1][1], **steps[1][2]), s.advance(5, w=w2, clamp=steps[2][1], **steps[2][2])]
    assert s.t == (seeds.shape[1] if which == 'cl_vrnn' else 0) + 12
    # by hand
    if which == 'cl_vrnn':
        _, st = M.generate_samples_device(model, seeds, 0, w, seed=23, return_state=True)
    else:
        st = GenState.fresh('cl_vae', model.engine.cfg, dev, seed_frame=seeds)
    saved = None
    for j, ((k, roll, temper), lab) in enumerate(zip(steps, (w, w, w2))):
        if j == 2:
            saved = st.to_numpy()
        Xs, st = M.generate_samples_device(model, None, k, lab, seed=23, clamp=roll, state=st, return_state=True, **temper)
        assert Xs.shape == (n, k, D) and np.array_equal(Xs, got[j])
        if roll is not None:
            fixed = roll <= 1
            assert np.array_equal(Xs[fixed], roll[fixed].astype(np.float64))
    _same_state(st, s.state)
    # to_numpy -> from_numpy -> continue equals continuing directly
    back = GenState.from_numpy(saved, dev)
    Xs = M.generate_samples_device(model, None, 5, w2, seed=23, clamp=steps[2][1], state=back, **steps[2][2])
    assert np.array_equal(Xs, got[2])
    # fork: the same rows go on alike, and the fork does not disturb the stream
    f = s.fork()
    g = s.fork([1, 1, 0])
    a, b, c = s.advance(3), f.advance(3), g.advance(3)
    assert np.array_equal(a, b) and g.N == 3 and not np.array_equal(c[0], c[1])
    assert np.array_equal(c[2][:0], a[0][:0]) and s.t == f.t == g.t
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            s.advance(bad)
    with pytest.raises(ValueError):
        s.advance(2, w=w[:1])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev):
    """10. every ValueError of the public calls on real models, and CLV_EINVAL for the step overflow"""
    from clvae_amd import _lib, ops
    from clvae_amd.engine_generate import GenState, STATE_FIELDS
    vr, MR, _ = _case_model(dev, 'cl_vrnn')
    va, MV, _ = _case_model(dev, 'cl_vae')
    seeds_r, w_r, _ = TR.vrnn_case_inputs()
    seeds_a, w_a, _ = TR.vae_case_inputs()
    _, st_r = MR.generate_samples_device(vr, seeds_r, 2, w_r, return_state=True)
    _, st_a = MV.generate_samples_device(va, seeds_a, 2, w_a, return_state=True)
    roll_r = np.full((seeds_r.shape[0], 4, D), 255, np.uint8)
    roll_a = np.full((seeds_a.shape[0], 4, D), 255, np.uint8)
    late = lambda s, t: GenState(s.kind, None, t, rows=s.rows)
    narrow = lambda s: GenState(s.kind, {k: torch.zeros(s.N, 64, device=dev) for k in STATE_FIELDS[s.kind]}, 0)
    for gen, model, w, st, other, roll, seeds in ((MR.generate_samples_device, vr, w_r, st_r, st_a, roll_r, seeds_r),
                                                   (MV.generate_samples_device, va, w_a, st_a, st_r, roll_a, seeds_a)):
        for kw in (dict(state=st, particles=4, clamp=roll), dict(state=other), dict(state=st.select([0, 1])),
                   dict(state=narrow(st)), dict(state=late(st, U32 - 3)), dict(state=st.to_numpy())):
            with pytest.raises(ValueError):
                gen(model, None, 4, w, **kw)
        with pytest.raises(ValueError):
            gen(model, seeds, 4, w, return_state=True, particles=4, clamp=roll)
        assert gen(model, None, 4, w, state=late(st, U32 - 4)).shape[1] == 4           # the last step there is: 2^32 - 1
    with pytest.raises(ValueError):
        MV.generate_samples_device(va, seeds_a, 4, w_a, state=st_a)                     # cl_vae seeds together with a state
    with pytest.raises(ValueError):
        MR.generate_samples_device(vr, seeds_r, 4, w_r, state=late(st_r, U32 - 3 - seeds_r.shape[1] + 1))   # S counts too
    eng = vr.engine
    with pytest.raises(ValueError):
        eng.generate(None, torch.zeros(5, 10, device=dev), 4)
    with pytest.raises(ValueError):
        eng.generate(None, torch.zeros(5, 10, device=dev), 0, state=st_r)               # nothing to run
    # the C ABI: t0 + S + nsteps > UINT32_MAX is CLV_EINVAL (-1); one less runs
    eng = TC._vrnn(dev, 2)
    x_seed, wv = TC._inputs(dev, N, 2, C, 1)
    Xs, out = torch.zeros(N, 4, D, device=dev), torch.zeros(N, 5, D, device=dev)

    def vrnn_call(t0):
        try:
            ops.vrnn_generate(N, 2, 4, D, 88, 2, C, eng.gate_act, False, 1, x_seed, wv, *eng._weights(), Xs, t0=t0, state_out=out)
        except _lib.ClvError as e:
            return str(e)
        return None
    ev = TC._vae(dev)
    xs1, w1 = TC._inputs(dev, N, None, 4, 2)
    sin = torch.stack([xs1, xs1], 1).contiguous()
    out2 = torch.zeros(N, 2, D, device=dev)

    def vae_call(t0, state_in=sin):
        try:
            ops.vae_generate(N, 4, D, 88, 3, 4, True, False, 1, None, w1, *ev._weights(), Xs, t0=t0, state_in=state_in,
                             state_out=out2)
        except _lib.ClvError as e:
            return str(e)
        return None
    assert vrnn_call(0) is None and vrnn_call(U32 - 6) is None
    assert vae_call(0) is None and vae_call(U32 - 4) is None
    for msg in (vrnn_call(U32 - 5), vrnn_call(U32), vae_call(U32 - 3), vae_call(U32), vae_call(0, None)):
        assert msg is not None and '(-1)' in msg, msg
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the tools
def _make_the_label_matter(M, which, h5):
    """Two epochs on the synthetic songs leave the label rows of both first layers near their initial values: a change of
    key then moves a note's probability by about 1e-3, and of the 3 x 5 x 88 draws behind the switch one or none falls that
    close to it (measured: 1 and 0 of 1320 for cl_vrnn), so "the frames differ after the switch" would test nothing.  The
    saved model's label rows get a draw of unit scale on top, as the engine tests use livelier weights than the
    initialisers give: a key then shifts the gates / hidden units by O(1)."""
    model = M.load_model(h5, optimizer='adam')[0] if which == 'cl_vrnn' else M.load_model(h5)[0]
    Cn = model.engine.cfg['C']
    rng = np.random.default_rng(5)
    for name, first in (('encoder_h', False), ('decoder_h', False)) if which == 'cl_vrnn' else (('h', False), ('decoder_h', True)):
        lay = model.get_layer(name)
        ws = lay.get_weights()
        k = lay.weight_names.index('kernel')
        rows = slice(0, Cn) if first else slice(ws[k].shape[0] - Cn, ws[k].shape[0])       # where the label enters the layer
        ws[k][rows] += rng.standard_normal(ws[k][rows].shape).astype(np.float32)
        lay.set_weights(ws)
    model.save_weights(h5)


@pytest.mark.parametrize("which", ['cl_vae', 'cl_vrnn'])
def test_sample_tools_in_chunks_and_modulated(dev, tmp_path, which):
    """11. --chunk 4 -t 10 writes byte-identical files to the run without it, plain and with --harmonize top --temperature
    0.8; --modulate writes frames that equal the plain run's up to the frame and differ after it"""
    from clvae_amd.cli import (DEVICE_LOOP_FLAGS, HARMONIZE_FLAGS, MORPH_FLAGS, RESUME_FLAGS, TEMPERATURE_FLAGS, VARY_FLAGS,
                               parser_for)
    from clvae_amd.utils.pianoroll import PianoData
    S = importlib.import_module('clvae_amd.%s.sample' % which)
    TRN = importlib.import_module('clvae_amd.%s.train' % which)
    data = make_synthetic_pickle(str(tmp_path / "syn.pickle"), n_songs=(10, 4, 4), seed=1)
    mdir = str(tmp_path / "models")
    os.makedirs(mdir)
    extra = ['--latent_dim', '4', '--batch_size', '50'] if which == 'cl_vae' else ['--seq_length', '8', '--batch_size', '20']
    np.random.seed(0)
    TRN.train(TRN.build_parser().parse_args(['m', '--use_x_prev', '--num_epochs', '2', '--patience', '0', '--train_file', data,
                                             '--model_dir', mdir] + extra))
    _make_the_label_matter(S.M, which, os.path.join(mdir, 'm.h5'))
    parser = parser_for('%s.sample' % which, DEVICE_LOOP_FLAGS + HARMONIZE_FLAGS + TEMPERATURE_FLAGS + VARY_FLAGS + MORPH_FLAGS
                        + RESUME_FLAGS)
    common = ['h', '-n', '3', '-t', '10', '--seed', '4', '-i', os.path.join(mdir, 'm.h5'), '--train_file', data]

    def run(name, flags):
        sdir = str(tmp_path / name)
        os.makedirs(sdir)
        np.random.seed(3)
        rolls = S.sample(parser.parse_args(common + ['--sample_dir', sdir] + flags))
        files = {f: open(os.path.join(sdir, f), 'rb').read() for f in sorted(os.listdir(sdir))}
        assert len(rolls) == 3 and all(np.asarray(r).shape == (10, D) for r in rolls) and files
        assert all(v[:4] == b'MThd' for v in files.values())
        return [np.asarray(r) for r in rolls], files

    plain, plain_files = run('plain', ['--device_loop'])
    for name, flags in (('chunk', ['--chunk', '4']), ('chunk1', ['--chunk', '1', '--device_loop']), ('chunk32', ['--chunk', '32'])):
        rolls, files = run(name, flags)
        assert files == plain_files and all(np.array_equal(a, b) for a, b in zip(rolls, plain))
    harm = ['--harmonize', 'top', '--temperature', '0.8']
    hrolls, hfiles = run('harm', harm)
    rolls, files = run('harm_chunk', harm + ['--chunk', '4'])
    assert files == hfiles and all(np.array_equal(a, b) for a, b in zip(rolls, hrolls))
    assert any(k.endswith('_source.mid') for k in hfiles) and hfiles != plain_files
    # --modulate: two names of the key map (a piece can have only one of them as its own key)
    P = PianoData(data, batch_size=1, seq_length=10, squeeze_x=which == 'cl_vae')
    names = sorted(P.key_map)[:2]
    assert len(names) == 2
    changed = 0
    for k, name in enumerate(names):
        rolls, files = run('mod%d' % k, ['--modulate', '%s@5' % name, '--chunk', '3'])
        assert sorted(files) == sorted(plain_files)
        for a, b in zip(rolls, plain):
            assert np.array_equal(a[:5], b[:5])
            changed += int(not np.array_equal(a[5:], b[5:]))
        print("%s --modulate %s@5: %d of %d notes after the frame differ from the plain run's" % (
            which, name, sum(int((a[5:] != b[5:]).sum()) for a, b in zip(rolls, plain)), 3 * 5 * D))
    assert changed >= 3             # every pick changes under at least one of the two keys: one of them is not its own
    with pytest.raises(ValueError):
        run('mod_bad', ['--modulate', 'no such key@5'])


# --------------------------------------------------------------------------- chunks under a temperature, seed frames
@pytest.mark.parametrize("temper", [dict(temperature=0.5), dict(temperature=2.0, z_temperature=0.5)],
                         ids=lambda t: ','.join('%s=%s' % kv for kv in t.items()))
def test_chunks_and_modulation_prime_under_the_runs_temperatures(dev, temper):
    """12. cl_vrnn with seed frames: one call draws the latents of the seed steps and the bridge sample under its own
    temperatures, so a Stream has to prime under them too.  64 pieces: with the priming at temperature 1 some bridge draw of
    the 64 x 88 falls between the two probabilities (the reference: 100 or more of them differ), and the pieces part."""
    from clvae_amd.stream import Stream, generate_chunked, modulate
    model, M, p = _case_model(dev, 'cl_vrnn')
    c, N, nsteps, seed = TR.VRNN_CASE, 64, 7, 23
    rng = np.random.default_rng(12)
    seeds = (rng.random((N, c['S'], D)) < 0.06).astype(np.float64)
    w = np.eye(c['C'])[rng.integers(0, c['C'], N)]
    # the condition on the inputs: the bridge under the run's temperatures is not the bridge at temperature 1
    bridge = lambda **t: TR.vrnn_generate(p, seeds, w, 1, seed, c['L'], **t)[1][:, c['S'] - 1]
    u = TR._noise(N, c['L'], seed, c['S'] - 1, np.float64)[1]
    cold, warm = bridge(), bridge(T=temper['temperature'], Tz=temper.get('z_temperature', 1.0))
    assert ((u <= cold) != (u <= warm)).sum() >= 100
    whole = M.generate_samples_device(model, seeds, nsteps, w, seed=seed, **temper)
    assert np.array_equal(generate_chunked(model, seeds, nsteps, w, chunk=3, seed=seed, **temper), whole)
    assert np.array_equal(modulate(model, seeds, [(w, 4), (w, 3)], seed=seed, **temper), whole)
    # a Stream built without them primes again at its first advance; a fork taken before keeps the first priming
    s = Stream(model, seeds, w, seed=seed)
    f = s.fork()
    assert np.array_equal(np.concatenate([s.advance(4, **temper), s.advance(3, **temper)], 1), whole)
    assert not np.array_equal(f.advance(7, **temper), whole)
