"""CPU: tests/generate_reference.py, the reference of the persistent sampling kernels -- pinned to the three earlier
references (temper, vary, latent) with the oracle's Philox noise, the sensitivity of its comparison to planted faults on
the very cases tests/test_gpu_generate.py launches, and the conditions on those cases that need no device."""
import numpy as np
import pytest

import generate_reference as GR
import latent_reference as LR
import temper_reference as TR
import vary_reference as VR

D = GR.D
PIN = 1e-12
CASES = GR.all_cases()


def _case(which, mode, N, L, C, nsteps, S=0, **over):
    c = dict(which=which, mode=mode, N=N, L=L, C=C, S=S, nsteps=nsteps, gate='hard_sigmoid' if which == 'cl_vrnn' else None,
             use_x_prev=True, z_prior=False, seed=0, t0=0, temper=None, clamp=None, hist_source=False, valued=False)
    c.update(over)
    return c


def _close(a, b):
    np.testing.assert_allclose(a, b, rtol=0, atol=PIN)


@pytest.fixture(scope="module")
def runs():
    """every case's weights, oracle noise and float32 loop on its own path, made once"""
    out = {}
    for c in CASES:
        p = GR.params_of(c)
        eps, u = GR.noise(c)
        out[c['id']] = (p, eps, u, GR.run(c, p, eps, u, np.float32))
    return out


# ------------------------------------------------------------------------------------------ pins to the earlier references
@pytest.mark.parametrize("z_prior", [False, True])
@pytest.mark.parametrize("T,Tz,seed", TR.ORACLE_RUNS + [(1.0, 1.0, 5)])
def test_reproduces_the_tempered_vrnn_loop_and_its_state(T, Tz, seed, z_prior):
    tc, p = TR.VRNN_CASE, TR.case_params('cl_vrnn')
    seeds, w, clamp = TR.vrnn_case_inputs()
    Xs, xh = TR.vrnn_generate(p, seeds, w, tc['nsteps'], seed, tc['L'], clamp, T, Tz, z_prior=z_prior)
    c = _case('cl_vrnn', 'CL+TP', tc['N'], tc['L'], tc['C'], tc['nsteps'], tc['S'], seeds=seeds, w=w, clamp=clamp, temper=(T, Tz),
              seed=seed, z_prior=z_prior)
    r = GR.run(c, p, *GR.noise(c))
    assert np.array_equal(r.Xs, Xs)
    _close(r.xhat, xh)
    # the state of TR.VrnnStepper fed the same inputs
    st = TR.VrnnStepper(p, w, seed, tc['L'], T, Tz, z_prior=z_prior)
    inputs = np.concatenate([seeds, r.samples[:, tc['S'] - 1:-1]], 1)
    for t in range(inputs.shape[1]):
        st.step(t, inputs[:, t])
    _close(r.state[:, :4], np.stack([st.he, st.ce, st.hd, st.cd], 1))
    assert np.array_equal(r.state[:, 4], Xs[:, -1])


@pytest.mark.parametrize("z_prior", [False, True])
@pytest.mark.parametrize("T,Tz,seed", TR.ORACLE_RUNS_VAE + [(1.0, 1.0, 5)])
def test_reproduces_the_tempered_vae_loop(T, Tz, seed, z_prior):
    tc, p = TR.VAE_CASE, TR.case_params('cl_vae')
    seeds, w, clamp = TR.vae_case_inputs()
    Xs, xh = TR.vae_generate(p, seeds, w, tc['nsteps'], seed, tc['L'], clamp, T, Tz, z_prior=z_prior)
    c = _case('cl_vae', 'CL+TP', tc['N'], tc['L'], tc['C'], tc['nsteps'], seeds=seeds, w=w, clamp=clamp, temper=(T, Tz),
              seed=seed, z_prior=z_prior)
    r = GR.run(c, p, *GR.noise(c))
    assert np.array_equal(r.Xs, Xs)
    _close(r.xhat, xh)
    assert np.array_equal(r.state, np.stack([Xs[:, -1], Xs[:, -2]], 1))
    # a resume from the state after 3 frames is the same piece
    c3 = dict(c, nsteps=3, clamp=clamp[:, :3])
    r3 = GR.run(c3, p, *GR.noise(c3))
    c4 = dict(c, mode='resume', nsteps=tc['nsteps'] - 3, clamp=np.ascontiguousarray(clamp[:, 3:]), t0=3, state_in=r3.state,
              seeds=None)
    r4 = GR.run(c4, p, *GR.noise(c4))
    assert np.array_equal(np.concatenate([r3.Xs, r4.Xs], 1), Xs)
    _close(np.concatenate([r3.xhat, r4.xhat], 1), xh)


@pytest.mark.parametrize("which,L,gate,use_x_prev", VR.IDENTITY_CASES)
@pytest.mark.parametrize("history", ['own', 'source'])
def test_reproduces_vary_encode_and_decode(which, L, gate, use_x_prev, history):
    C, N, Tn, seed = VR.classes_of(which), VR.IDENTITY_N, VR.IDENTITY_T, VR.IDENTITY_SEED
    _, p = VR.case_params(which, L, C, use_x_prev, gate or 'hard_sigmoid')
    src, x0, w_enc, w_dec = VR.case_inputs(N, Tn, C)
    clamp = VR.roll(N, Tn, seed=3)
    T, Tz = 0.5, 1.5
    Xs, xh, lg = VR.vary(which, p, src, w_enc, w_dec, x0, history, seed, L, clamp, T, Tz, gate=gate or 'hard_sigmoid')
    c = _case(which, 'vary_latents', N, L, C, Tn, sources=src, x0=x0, w=w_enc, w_dec=w_dec, clamp=clamp, temper=(T, Tz),
              seed=seed, gate=gate, use_x_prev=use_x_prev, hist_source=history == 'source')
    r = GR.run(c, p, *GR.noise(c))
    assert np.array_equal(r.Xs, Xs)
    _close(r.xhat, xh)
    _close(r.logit, lg)
    z, zm, zlv = LR.encode(which, p, src, w_enc, seed, L, Tz, gate=gate or 'hard_sigmoid')
    _close(r.z, z)
    _close(r.zm, zm)
    _close(r.zlv, zlv)
    # the decode-only loop on that path, a given history, the uniforms of other rows
    rows = np.array([3, 0, 3, 7, 1])
    z = z.astype(np.float32).astype(np.float64)                 # the path as a launch holds it
    hist = 'own' if history == 'own' else src
    Xd, xd, ld = LR.decode(which, p, z, w_dec, x0, hist, seed, L, clamp, T, gate=gate or 'hard_sigmoid', noise_rows=rows)
    cd = _case(which, 'decode', N, L, C, Tn, z_in=z, x0=x0, w=w_dec, w_dec=w_dec, clamp=clamp, temper=(T, 1.0), seed=seed,
               gate=gate, use_x_prev=use_x_prev, history=None if history == 'own' else src, noise_rows=rows)
    rd = GR.run(cd, p, *GR.noise(cd))
    assert np.array_equal(rd.Xs, Xd)
    _close(rd.xhat, xd)
    _close(rd.logit, ld)


def test_vrnn_resume_is_the_same_piece():
    """two calls through a state, Philox steps counted on, against one call"""
    tc, p = TR.VRNN_CASE, TR.case_params('cl_vrnn')
    seeds, w, clamp = TR.vrnn_case_inputs()
    c = _case('cl_vrnn', 'resume', tc['N'], tc['L'], tc['C'], tc['nsteps'], tc['S'], seeds=seeds, w=w, clamp=clamp, seed=31)
    whole = GR.run(c, p, *GR.noise(c))
    c1 = dict(c, nsteps=0, clamp=None)                      # primed: x is the bridge sample
    r1 = GR.run(c1, p, *GR.noise(c1))
    c2 = dict(c, S=0, seeds=None, t0=tc['S'], state_in=r1.state)
    r2 = GR.run(c2, p, *GR.noise(c2))
    assert np.array_equal(r2.Xs, whole.Xs)
    _close(r2.xhat, whole.xhat[:, tc['S']:])
    _close(r2.state, whole.state)


def test_kernel_formulas_in_float32():
    x = np.linspace(-9, 9, 2001, dtype=np.float32)
    assert np.abs(GR._tanh_kernel(x).astype(np.float64) - np.tanh(x.astype(np.float64))).max() < 3e-7
    assert GR._tanh_kernel(x).dtype == np.float32


# ---------------------------------------------------------------------------------------------- the cases themselves
def test_every_instance_and_every_listed_value_is_launched():
    inst = {GR.instance_of(c) for c in CASES}
    assert len([i for i in inst if i.startswith('vrnn')]) == 32 and len([i for i in inst if i.startswith('vae')]) == 8
    for which in ('cl_vrnn', 'cl_vae'):
        for mode in GR.MODES:
            cs = [c for c in CASES if c['which'] == which and c['mode'] == mode]
            assert {c['L'] for c in cs} >= set(GR.LATENTS[which]) and {c['C'] for c in cs} >= set(GR.CLASSES[which])
            assert {c['N'] for c in cs} >= {1, 5} and {c['use_x_prev'] for c in cs} == {True, False}
            assert max(GR.frames_of(c) for c in cs) <= 12 or mode in ('vary_latents', 'resume')
            if which == 'cl_vrnn':
                assert {(c['gate'], c['L'] > 16) for c in cs} == {(g, wd) for g in ('hard_sigmoid', 'sigmoid')
                                                                  for wd in (False, True)}
            if mode in GR.GENERATE_MODES + ('resume',):
                assert {c['z_prior'] for c in cs} == {True, False}
            if mode in ('TP', 'CL+TP'):
                assert {c['temper'] for c in cs} == set(GR.TEMPERS)
            if mode in ('CL', 'CL+TP'):
                assert {c['roll'] for c in cs} == set(GR.ROLLS)
            if mode in ('vary', 'vary_latents'):
                assert {c['hist_source'] for c in cs} == {True, False} and {c.get('x0') is None for c in cs} == {True, False}
                assert {c['clamp'] is None for c in cs} == {True, False}
                assert all(not np.array_equal(c['w'], c['w_dec']) for c in cs)
            if mode == 'decode':
                assert {c.get('history') is None for c in cs} == {True, False}
                assert any(c.get('noise_rows') is not None and len(set(c['noise_rows'])) < c['N'] for c in cs)
            if mode == 'resume':
                assert {c['t0'] for c in cs} >= {0, 7} and any(c['t0'] + GR.frames_of(c) == 2 ** 32 - 1 for c in cs)
                if which == 'cl_vrnn':
                    assert {c.get('state_in') is None for c in cs} == {True, False}
                    assert any(c['S'] == 0 for c in cs) and any(c['nsteps'] == 0 for c in cs)
            if which == 'cl_vrnn' and mode in GR.GENERATE_MODES:
                assert {(c['S'], c['nsteps']) for c in cs} >= set(GR.SHAPES_CL if 'CL' in mode else GR.SHAPES)
    assert {c['N'] for c in CASES} == {1, 5, 260}
    # xhat = NULL is launched once per (family, mode), on a case that returns frames
    none = [c for c in CASES if c['xhat_none']]
    assert all(c['nsteps'] > 0 for c in none)
    assert sorted((c['which'], c['mode']) for c in none) == sorted((f, m) for f in ('cl_vrnn', 'cl_vae') for m in GR.MODES)
    # the probability side of the x_hat comparison is reached: logits beyond +-5.8 in the 'far' case of each family
    for c in (c for c in CASES if c['id'].endswith('-far')):
        assert not GR.teacher_forced(c)
        logit = GR.run(c, GR.params_of(c), *GR.noise(c)).logit
        assert (np.abs(logit) > GR.MAX_LOGIT).sum() >= 10 and (np.abs(logit) <= GR.MAX_LOGIT).sum() >= 10, c['id']
    assert len([c for c in CASES if c['id'].endswith('-far')]) == 2
    # an edge frame of every kind at every place
    for which, edges in (('cl_vrnn', GR.EDGE_FRAMES), ('cl_vae', GR.EDGE_FRAMES_VAE)):
        places = ('seeds', 'sources', 'x0', 'history', 'state_x', 'clamp')
        for place in places:
            seen = set()
            for c in (c for c in CASES if c['which'] == which):
                a = c.get('state_in') if place == 'state_x' else c.get(place)
                if a is None:
                    continue
                if place == 'state_x' and which == 'cl_vrnn':
                    a = a[:, 4]
                rows = np.asarray(a, np.float32).reshape(-1, D)
                seen |= {i for i, e in enumerate(edges) if (rows == e).all(1).any()}
            assert seen == set(range(len(edges))), (which, place, seen)
    valued = [c for c in CASES if c['valued']]
    assert {c['mode'] for c in valued} == {'plain', 'vary', 'resume'}
    for name in ('seeds', 'sources', 'x0'):
        assert any(c.get(name) is not None and {0.5, 2.0} <= set(np.unique(c[name])) for c in valued), name
    assert any(c.get('state_in') is not None and {0.5, 2.0} <= set(np.unique(c['state_in'][:, 4])) for c in valued)
    frames = ('seeds', 'sources', 'x0', 'history', 'state_in')
    assert all(set(np.unique(c[n])) <= {0.0, 1.0} for c in CASES if c['which'] == 'cl_vae' for n in frames if c.get(n) is not None)


@pytest.mark.parametrize("c", CASES, ids=lambda c: c['id'])
def test_conditions_on_the_inputs(c, runs):
    """what the GPU test would otherwise have to discover: the float32 reference deviates in every frame of every output
    (no bound is 0), the reference's own float32 run passes its own comparison, the fully teacher-forced and fully clamped
    cases keep |logit| <= 5.8, and on the free-running ones the float32 loop on its own path stays within the flip cap"""
    p, eps, u, r32 = runs[c['id']]
    ratio, ref_dev, wrong = GR.check(c, p, eps, u, GR.outputs_of(r32, c))
    assert all(v > 0 for v in ref_dev.values()), ref_dev
    # its own deviation is a quarter of each bound by construction; on the probability side (the 'far' cases) the float32
    # sigmoid's rounding of p comes on top of the logit's deviation carried through the slope: within half the bound
    own = {k: 0.5 if (k == 'xhat' and c['id'].endswith('-far')) else 1.0 if k == 'z_formula' else 1 / GR.FACTOR + 1e-12 for k in ratio}
    assert all(v <= own[k] for k, v in ratio.items()), ratio
    assert not any(wrong.values()), wrong
    r64 = GR.run(c, p, eps, u)
    if GR.teacher_forced(c):
        assert np.abs(r64.logit).max() <= GR.MAX_LOGIT, np.abs(r64.logit).max()
    else:
        T_ = c['temper'][0] if c['temper'] is not None else 1.0
        along = GR.run(c, p, eps, u, along=r32.samples)             # the float64 loop fed the float32 loop's samples
        diff = along.samples != r32.samples.astype(np.float64)
        far = diff & ~(np.abs(u.transpose(1, 0, 2).astype(np.float64) - along.xhat) < TR.window(T_))
        print(c['id'], "flips", int(diff.sum()), "outside the window", int(far.sum()))
        assert far.sum() == 0 and diff.sum() <= TR.FLIP_CAP


# ------------------------------------------------------------------------------------------------- the planted faults
@pytest.mark.parametrize("name", sorted(GR.FAULTS))
def test_planted_fault_exceeds_a_bound(name, runs):
    """each fault, planted in the float32 loop on the GPU test's own cases, exceeds the bound of some frame of some output
    at least 4 times over (or breaks an entry that must be exact) -- in at least one case, and in how many is printed"""
    applies = GR.FAULTS[name][0]
    cases = [c for c in CASES if applies(c) and c['N'] <= 5]
    assert cases, name
    caught, worst = [], 0.0
    for c in cases:
        p, eps, u, _ = runs[c['id']]
        ratio, _, wrong = GR.planted(c, p, eps, u, name)
        top = max(ratio.values())
        worst = max(worst, top)
        if top >= 4 or any(wrong.values()):
            caught.append(c['id'])
    print("%s: caught in %d of %d cases, largest ratio %.3g" % (name, len(caught), len(cases), worst))
    assert caught, (name, worst)
