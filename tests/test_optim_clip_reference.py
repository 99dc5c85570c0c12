"""CPU: tests/optim_clip_reference.py itself -- the norm's bound holds honest fp32 evaluations in several orders and is not
vacuous, g_eff / gdot_eff / the decayed rate are what the contract says, and every case of GPU_CASES is SENSITIVE to the
clip: the reference's clipped params' differ from the unclipped ones beyond their bounds in at least half of the elements not
flagged insensitive (two steps of history make them differ; a first Adam step alone is scale-invariant and would hide a
missing clip)."""
import numpy as np
import pytest

import optim_clip_reference as RC
import optim_reference as R
from vae_reference import U

F = np.float32


def _sum32(x, order):
    x = np.asarray(x, F)
    if order == 'seq':
        acc = F(0)
        for v in x:
            acc = F(acc + v)
        return acc
    if order == 'pair':
        k = 1
        while k < x.size:
            k *= 2
        y = np.zeros(k, F)
        y[:x.size] = x
        while k > 1:
            k //= 2
            y = y[:k] + y[k:]
        return y[0]
    if order == 'blocks':                 # fp32 partials of 1408 terms (pairwise), their sum in fp64
        parts = [np.float64(_sum32(x[i:i + 1408], 'pair')) for i in range(0, x.size, 1408)]
        return np.sum(parts)
    raise ValueError(order)


NORM_CASES = ['small', 'chain_tall_last', 'flat_193x100', 'mixed_plain']


@pytest.mark.parametrize("cname", NORM_CASES)
def test_honest_fp32_norms_lie_within_the_bound_and_wrong_ones_do_not(cname):
    case = RC.BY_NAME[cname]
    table, n, _ = R.layout(case['shapes'])
    g, _ = R.make_grads(table, n, 41)
    ref = RC.norm_ref(g, table, np.inf)
    assert ref['norm'] == RC.norm64(g, table) and ref['scale'] == 1.0 and ref['b_scale'] == 0.0
    own = RC.owned(table, n)
    sq = (g[own] * g[own]).astype(F)
    for order in ('seq', 'pair', 'blocks'):
        got = float(F(np.sqrt(_sum32(sq, order))))
        assert abs(got - ref['norm']) <= ref['b_norm'], (order, got, ref)
    assert 0 < ref['b_norm'] < 1e-4 * ref['norm']
    # not vacuous: one padding float read into the sum, the largest term left out, the terms not squared
    pad = np.flatnonzero(~own)
    wrong = [np.sqrt(np.square(g[own].astype(np.float64)).sum() - float(np.abs(g[own]).max()) ** 2), np.abs(g[own].astype(np.float64)).sum()]
    if pad.size:
        wrong.append(np.sqrt(ref['norm'] ** 2 + float(g[pad[0]]) ** 2))
    for w in wrong:
        assert abs(w - ref['norm']) > ref['b_norm'], w


def test_scale_and_its_bound():
    table, n, _ = R.layout(RC.BY_NAME['small']['shapes'])
    g, _ = R.make_grads(table, n, 42)
    nm = RC.norm64(g, table)
    clip = RC.norm_ref(g, table, 0.25 * nm)
    assert abs(clip['scale'] - 0.25) < 1e-7 and 0 < clip['b_scale'] < 1e-5
    # one more division: the scale's relative bound is the norm's and one rounding
    rel = np.hypot(clip['s_norm'] / clip['norm'], U)
    assert abs(clip['s_scale'] / clip['scale'] - rel) <= 1e-6 * rel
    loose = RC.norm_ref(g, table, 4 * nm)
    assert loose['scale'] == 1.0 and loose['b_scale'] == 0.0
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError):
            RC.norm_ref(g, table, bad)
    with pytest.raises(ValueError):
        RC.norm_ref(g, table, nm)               # the branch would be undetermined


def test_effective_gradient_is_the_contract_bit_for_bit():
    table, n, _ = R.layout(RC.BY_NAME['small']['shapes'])
    g, _ = R.make_grads(table, n, 43)
    own = RC.owned(table, n)
    same = RC.g_eff(g, table, 1.0)
    assert (same.view(np.uint32) == g.view(np.uint32)).all()
    s = F(0.3)
    e = RC.g_eff(g, table, s)
    assert e.dtype == F and (e[~own] == R.SENTINEL).all()
    exact = (g[own].astype(np.float64) * float(s))
    assert (e[own] == exact.astype(F)).all()                      # one exactly rounded product
    cv = RC.median_abs(g, table)
    c = RC.g_eff(g, table, s, cv)
    assert (np.abs(c[own]) <= F(cv)).all() and (c[~own] == R.SENTINEL).all()
    inside = np.abs(e[own]) <= F(cv)
    assert (c[own][inside] == e[own][inside]).all() and (c[own][~inside] == np.sign(e[own][~inside]) * F(cv)).all()
    assert 0.2 < (np.abs(g[own]) > cv).mean() < 0.6               # the median: about half are clamped without a scale
    # scale first, clamp second (Keras' order): the other order gives other numbers
    other = (np.clip(g[own], -F(cv), F(cv)) * s).astype(F)
    assert (other != c[own]).any()
    h = g.copy()
    h[own.nonzero()[0][0]] = np.nan
    assert np.isnan(RC.g_eff(h, table, s, cv)[own][0])
    gd = np.asarray([1.5, -2.25, 0.0], F)
    assert (RC.gdot_eff(gd, s) == (gd.astype(np.float64) * float(s)).astype(F)).all()


def test_decayed_rate():
    assert RC.decayed_lr(1e-3, 1e-4, 1) == float(F(1e-3))                  # it = 0 at the first step
    assert RC.decayed_lr(1e-3, 1.0, 2) == float(F(float(F(1e-3)) / 2.0))
    for t in (1, 2, 1000, 10 ** 6):
        for decay in (1e-4, 1.0):
            want = float(F(1e-3)) / (1.0 + float(F(decay)) * (t - 1))
            assert abs(RC.decayed_lr(1e-3, decay, t) - want) <= U * want            # one rounding to fp32
    h = R.hyper()
    assert RC.decayed_hyper(h, 0.0, 5) == h and RC.decayed_hyper(h, 1.0, 3)['lr'] == RC.decayed_lr(h['lr'], 1.0, 3)


@pytest.mark.parametrize("case,route", RC.CASE_ROUTES, ids=RC.IDS)
def test_every_case_is_sensitive_to_the_clip(case, route):
    """clipnorm = 0.25 norm64: at at least half of the elements of params' not flagged insensitive the unclipped reference lies
    beyond the clipped reference's bounds -- optim_reference.violations would report a device that left the clip out.  The
    tightest case is pair_first_145x2: 147 of its 293 elements (0.502); the other 145 are column 1 of its 145 x 2 matrix, whose
    gradient make_grads keeps at zero at every step, so that no gradient, clipped or not, ever moves them.  With
    clipvalue = the median |g| alone: at least half of the elements whose gradient the clamp changes (under plain Adam and
    RMSprop the clamp leaves the others exactly as they were, and they are the other half)."""
    table, n, n_cols, st, g = RC.prepared(case, route)
    hyp = R.hyper(opt=R.ROUTE_OPT[route])
    wn = hyp['opt'] == R.OPT_ADAM_WN
    known = RC.known_for(table, st, g, route == 'fast') if wn else None
    own = RC.owned(table, n)
    plain = R.ref_step(st, g, table, hyp, 'advance', known)
    assert R.insensitive_share(plain, table) <= 0.01
    nm = RC.norm_ref(g, table, RC.clip_args('clipnorm', g, table)[0])
    assert abs(nm['scale'] - RC.CLIP_FACTOR) < 1e-6
    clipped, ge = RC.clipped_ref(st, g, table, hyp, 'advance', known, F(nm['scale']))
    share = RC.differing_share(clipped, plain, own & ~plain['insens'] & ~clipped['insens'])
    assert share >= 0.5, share
    assert (ge[~own] == R.SENTINEL).all()
    cv = RC.clip_args('clipvalue', g, table)[1]
    assert cv > 0
    clamped, _ = RC.clipped_ref(st, g, table, hyp, 'advance', dict(known, use=False) if known else None, F(1), cv)
    hit = own & (np.abs(g) > F(cv)) & ~plain['insens'] & ~clamped['insens']
    unclamped = plain if route != 'fast' else R.ref_step(st, g, table, hyp, 'advance', dict(known, use=False))
    share_v = RC.differing_share(clamped, unclamped, hit)
    assert hit.sum() > 0 and share_v >= 0.5, share_v
