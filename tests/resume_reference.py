"""numpy reference of a MODULATED piece (TEST ORACLE): the frame loops of tests/temper_reference.py with the
label replaced at a returned frame, which is what Stream.advance(w=...) / modulate() do on the device.  The steppers keep
their state in plain attributes, so a modulation is `stepper.w = ...` between two steps.  In float64 or, for the flip-cap
condition of the GPU tests (tests/test_resume_reference.py), in float32."""
import numpy as np

import temper_reference as TR

D = TR.D
PLAN_FRAMES = (5, 6)                    # two labels, 5 + 6 frames
# the Philox seed of each family's run: an INPUT chosen so that the float32 run of the loops below stays within the flip cap
# of its float64 run (tests/test_resume_reference.py asserts it); models, seed frames and first labels are the cases' own
MOD_SEED = {'cl_vrnn': 31, 'cl_vae': 17}


def second_label(w):
    """another key for every piece: the class three above its own"""
    w = np.asarray(w)
    return np.eye(w.shape[1])[(w.argmax(1) + 3) % w.shape[1]]


def plan_of(w):
    return [(np.asarray(w, np.float64), PLAN_FRAMES[0]), (second_label(w), PLAN_FRAMES[1])]


def _label_at(plan):
    """returned frame -> the label that takes over there"""
    at, j = {}, 0
    for w, n in plan:
        at[j] = w
        j += n
    return at, j


def vrnn_modulated(p, seeds, plan, seed, L, T=1.0, Tz=1.0, dtype=np.float64, follow=None):
    """TR.vrnn_generate without a roll, the label replaced at the first frame of every stage of plan (the seed steps and
    the bridge run under the first label) -> Xs [N, sum n, D]"""
    N, S = seeds.shape[:2]
    at, total = _label_at(plan)
    st = TR.VrnnStepper(p, plan[0][0], seed, L, T, Tz, dtype)
    free = np.full((N, D), TR.FREE)
    x_prev, Xs = np.zeros((N, D), dtype), []
    for t in range(S + total):
        if t < S:
            x_prev = seeds[:, t]
        elif t - S in at:
            st.w = np.asarray(at[t - S], dtype)
        xhat = st.step(t, x_prev)
        x_t = (st.u <= xhat).astype(dtype)
        if t >= S:
            if follow is not None:
                x_t = follow.frame(t - S, x_t, st.u, xhat, free).astype(dtype)
            Xs.append(x_t)
        x_prev = x_t
    return np.stack(Xs, 1)


def vae_modulated(p, seeds, plan, seed, L, T=1.0, Tz=1.0, dtype=np.float64, follow=None):
    """TR.vae_generate without a roll, the label replaced at the first frame of every stage of plan -> Xs [N, sum n, D]"""
    N = seeds.shape[0]
    at, total = _label_at(plan)
    st = TR.VaeStepper(p, plan[0][0], seed, L, T, Tz, dtype)
    free = np.full((N, D), TR.FREE)
    x_in, hist, Xs = seeds, seeds, []
    for t in range(total):
        if t in at:
            st.w = np.asarray(at[t], dtype)
        xhat = st.step(t, x_in, hist)
        x_t = (st.u <= xhat).astype(dtype)
        if follow is not None:
            x_t = follow.frame(t, x_t, st.u, xhat, free).astype(dtype)
        Xs.append(x_t)
        hist, x_in = x_in, x_t
    return np.stack(Xs, 1)


def case(which):
    """(weights, seed frames, first label, L, the modulated loop) of a family's run"""
    p = TR.case_params(which)
    if which == 'cl_vrnn':
        seeds, w, _ = TR.vrnn_case_inputs()
        return p, seeds, w, TR.VRNN_CASE['L'], vrnn_modulated
    seeds, w, _ = TR.vae_case_inputs()
    return p, seeds, w, TR.VAE_CASE['L'], vae_modulated


def flips_f32_against_f64(which, seed=None):
    """the Follow of the float64 modulated loop along the float32 loop's frames"""
    p, seeds, w, L, gen = case(which)
    seed = MOD_SEED[which] if seed is None else seed
    plan = plan_of(w)
    got = gen(p, seeds.astype(np.float32), plan, seed, L, dtype=np.float32)
    fol = TR.Follow(got, TR.window(1.0))
    gen(p, seeds, plan, seed, L, follow=fol)
    return fol, got
