"""CPU: what tests/filter_reference.py promises about its own tables and judges, shown on the reference alone -- every counted
frame feasible, no draw within 1e-9 of its threshold, no ESS beside the resampling threshold, the bounds of logW / logZ / ess
neither loose nor tight by accident, the clamping references equal to the plain ones in range -- and a subtly wrong kernel
modelled three ways, each of which its judge catches."""
import numpy as np
import pytest

import filter_reference as F
import gibbs_reference as GR
import smc_reference as SR
import voices_reference as VR
from helpers import FILL_U8


# --------------------------------------------------------------------------------------------------------- the tables --
def test_tables_hold_the_shapes_they_name():
    assert {c['D'] for c in F.SAMPLE} == {1, 63, 64, 65, 88, 129, 200}
    assert {(c['R'], c['P']) for c in F.SAMPLE} == {(1, 1), (3, 1), (4, 4), (5, 5), (66, 11), (1028, 4)}
    for key in ('D', 'R'):                                # both S with every width and every row count
        for v in {c[key] for c in F.SAMPLE}:
            assert {c['S'] for c in F.SAMPLE if c[key] == v} == {0, 2}
    assert {c['D'] for c in F.VOICES} == {1, 15, 16, 17, 63, 64, 65, 88, 96, 97, 127, 128}
    for R in (15, 16, 17, 67):
        Ps = {c['P'] for c in F.VOICES if c['R'] == R}
        assert 1 in Ps and len(Ps) == 2 and all(R % P == 0 for P in Ps)
    assert {c['P'] for c in F.RESAMPLE} == {1, 2, 3, 5, 63, 64, 65, 100, 1023, 1024}
    assert {c['G'] for c in F.RESAMPLE} == {1, 2, 3, 4, 5, 300} and all(c['G'] == 2 for c in F.RESAMPLE if c['P'] >= 1023)
    for key, vals in (('tau', set(F.TAUS)), ('m0', set(F.M0S)), ('S', {0, 3}), ('script', set(F.SCRIPTS))):
        assert {c[key] for c in F.RESAMPLE} == vals
    assert any(c['script'] == 'uniform' and c['tau'] == 1.0 for c in F.RESAMPLE)
    assert {c['nbuf'] for c in F.GATHER} == {1, 3, 8} and {c['flags'] for c in F.GATHER} == {0, 1, 2}
    assert {w for c in F.GATHER if c['nbuf'] == 1 for w in c['widths']} == {1, 63, 64, 65}
    assert {w for c in F.GATHER for w in c['widths']} == set(F.WIDTHS)
    assert {(c['P'], c['n_out']) for c in F.BACKTRACK} == {(1, 1), (1, 5), (5, 64), (64, 64), (200, 9), (1024, 3), (70, 40)}
    assert {c['D'] for c in F.BACKTRACK} == {1, 65, 88, 200} and {c['picks'] for c in F.BACKTRACK} == {True, False}
    for t in (F.PATH, F.PIN):
        assert {1, 4, 5} <= {c['G'] for c in t} and {c['L'] for c in t} == {1, 3, 65} and {c['D'] for c in t} == {1, 65, 88}
    assert {2, 32} <= {c['C'] for c in F.INIT_W} and F.BIG_M0 in {c['m0'] for c in F.INIT_W if c['mode'] == 1}
    names = [c['name'] for t in (F.SAMPLE, F.VOICES, F.RESAMPLE, F.GATHER, F.BACKTRACK, F.PATH, F.PIN, F.TAKE_W, F.INIT_W,
                                 F.POSTERIOR) for c in t]
    assert len(set(names)) == len(names)


def test_sample_rolls_have_every_kind():
    kinds = set()
    for i, c in enumerate(F.SAMPLE):
        inp = F.sample_inputs(i)
        for g in range(inp['roll'].shape[0]):
            r = inp['roll'][g]
            kinds.add('free' if np.all(r == F.FREE) else 'clamped' if np.all(r <= 1) else 'mixed')
            forced = np.nonzero((r <= 1).any(axis=0))[0]
            q = inp['xhat'][g * c['P']][forced]
            if len(forced) and np.all((q <= SR.CLIP_LO) | (q >= SR.CLIP_HI)):
                kinds.add('clip points only')
    assert kinds == {'free', 'clamped', 'mixed', 'clip points only'}


def test_voices_frames_are_feasible_and_no_draw_is_near():
    worst, seen = np.inf, set()
    for i, c in enumerate(F.VOICES):
        inp = F.voices_inputs(i)
        assert F.voices_feasible(c, inp), c['name']
        seen |= {tuple(int(v) for v in p) for p in inp['voices'].reshape(-1, 2)}
        for k in range(c['nsteps']):
            x, ell, logb, margin = F.voices_want(i, k)
            assert margin >= 1e-9, (c['name'], k, margin)          # re-seed the case; never widen this
            worst = min(worst, margin)
            assert np.all(np.isfinite(ell)) and np.all(logb <= 0)
            rows, pairs, free = F.voices_rows(c, inp, k)
            n = x.sum(axis=1)
            assert np.all(free | ((n >= pairs[:, 0]) & (n <= pairs[:, 1])))
    print("smallest margin of the voices table: %.3g" % worst)
    assert set(F.NOT_COUNTED) <= seen and {(0, 0), (1, 1), (15, 15), (0, 15), VR.FREE_PAIR} <= seen
    assert any(p[0] == p[1] == c['D'] for c in F.VOICES if c['D'] <= 15 for p in F.voices_pairs(c['D']))


def test_free_and_counted_rows_share_a_group_of_four():
    hit = 0
    for i, c in enumerate(F.VOICES):
        if c['R'] < 4:
            continue
        _, _, free = F.voices_rows(c, F.voices_inputs(i), 0)
        groups = [free[g:g + 4] for g in range(0, c['R'], 4)]
        hit += any(g.any() and not g.all() for g in groups)
    assert hit >= 20


@pytest.mark.parametrize("conditional", [False, True])
def test_resample_table_guarantees(conditional):
    consecutive = never = 0
    for i, c in enumerate(F.RESAMPLE):
        ell = F.resample_script(i)
        ref, dist, uniform = F.reference_run(c, conditional, ell)
        assert not ref.near.any(), c['name']
        exact = uniform & (c['tau'] == 1.0)
        assert np.all(ref.ess.T[uniform] == float(c['P'])), c['name']       # uniform weights: exactly P
        assert not ref.resampled[uniform].any(), c['name']
        assert np.all(dist[~exact] >= 1e-9), (c['name'], dist[~exact].min())
        r = ref.resampled
        consecutive += bool((r[1:] & r[:-1]).any())
        never += not r.any()
        if c['script'] == 'dominant' and c['P'] > 1:
            assert np.any(np.exp(ref.logW) == 0.0) or r.any()
        if c['script'] == 'spread':
            assert not r.any(), c['name']
            assert c['P'] <= 3 or (np.exp(ref.logW) == 0.0).mean() > 0.5, c['name']           # most weights exactly 0
    assert consecutive >= 1 and never >= 1


def test_other_tables_have_no_near_draw():
    for i, c in enumerate(F.BACKTRACK):
        assert not F.backtrack_near(c, F.backtrack_inputs(i)), c['name']
    for i, c in enumerate(F.INIT_W):
        if c['mode'] == 0:
            assert not F.init_w_near(c, F.init_w_inputs(i)), c['name']
    filt = [F.backtrack_inputs(i)['anc'] for i, c in enumerate(F.BACKTRACK) if c['lineage'] == 'filter' and c['P'] >= 5]
    assert all(len(np.unique(a[0])) < a.shape[1] for a in filt)            # real lineages coalesce


# -------------------------------------------------------------------------------------------------- the bound's place --
@pytest.mark.parametrize("conditional", [False, True])
def test_kernel_order_stays_below_half_the_bound_and_fp32_exp_does_not(conditional):
    worst, caught = {}, 0
    for i, c in enumerate(F.RESAMPLE):
        ell = F.resample_script(i)
        rep = F.judge_resample(c['name'], c, conditional, ell, F.model_resample(c, conditional, ell))
        for k, v in rep.items():
            worst[k] = max(worst.get(k, 0.0), v)
            assert v <= 0.5, (c['name'], k, v)
        try:
            F.judge_resample(c['name'], c, conditional, ell, F.model_resample(c, conditional, ell, exp=F.exp32))
        except AssertionError:
            caught += 1
    print("kernel order against the reference, worst error / bound: %s; fp32 exp caught on %d of %d cases"
          % (worst, caught, len(F.RESAMPLE)))
    assert caught >= 1
    assert any(c['script'] == 'random' for c in F.RESAMPLE)


# -------------------------------------------------------------------------------------------------------- the mutants --
def test_mutant_float32_log_in_increment_is_caught():
    caught = 0
    for i, c in enumerate(F.SAMPLE):
        inp = F.sample_inputs(i)
        k = 1
        rows = np.repeat(inp['roll'][:, k], c['P'], axis=0)
        x = SR.sample_frame(inp['xhat'], inp['u'], rows).astype(np.float32)
        hist = np.full((c['nsteps'], c['R'], c['D']), FILL_U8, np.uint8)
        hist[k] = x
        good = dict(x=x, ell=SR.increment(inp['xhat'], rows), hist=hist)
        assert F.judge_sample(c['name'], c, inp, k, good)['ell'] == 0.0
        try:
            F.judge_sample(c['name'], c, inp, k, dict(good, ell=F.increment_log32(inp['xhat'], rows)))
        except AssertionError as e:
            assert ' ell' in str(e)
            caught += 1
    assert caught >= len(F.SAMPLE) // 2


def test_mutant_greater_or_equal_in_systematic_is_caught():
    """no table has a draw on a grid point, so the mutant passes them all: it takes the one input built to sit on one"""
    for i, c in enumerate(F.RESAMPLE[:10]):
        ell = F.resample_script(i)
        F.judge_resample(c['name'], c, False, ell, F.model_resample(c, False, ell, strict=False))
    lw, u0, seed, step = F.tie_case()
    idx, grid = SR.systematic(lw, 2, u0)
    assert grid[0] == u0 and idx[0] == 1                   # 2 C_0 > u0 is false: the first draw goes to particle 1
    cum = np.cumsum(np.exp(lw))[None]
    pts = (u0 + np.arange(2.0))[None]
    F.check_bits("tie, >", F._pick(cum, 2.0, pts)[0], idx)
    with pytest.raises(AssertionError):
        F.check_bits("tie, >=", F._pick(cum, 2.0, pts, strict=False)[0], idx)


def test_mutant_mask_bit_at_note_96_is_caught():
    caught = tried = 0
    for i, c in enumerate(F.VOICES):
        if c['D'] < 96 or c['R'] > 17:
            continue
        inp = F.voices_inputs(i)
        rows, pairs, free = F.voices_rows(c, inp, 0)
        want = F.voices_want(i, 0)
        for mutant in (False, True):
            x = want[0].copy()
            for r in np.nonzero(~free)[0]:
                x[r] = F.voices_bitmask_draw(inp['xhat'][r], inp['u'][r], int(pairs[r, 0]), int(pairs[r, 1]),
                                             None if rows is None else rows[r], mutant)
            got = dict(x=x.astype(np.float32), logb=want[2])
            if not mutant:                                 # the model itself is the reference's draw
                F.judge_voices(c['name'], c, inp, 0, got, want)
                continue
            tried += c['D'] > 96
            try:
                F.judge_voices(c['name'], c, inp, 0, got, want)
            except AssertionError as e:
                assert c['D'] > 96 and 'note' in str(e)
                caught += 1
    assert tried >= 4 and caught >= 1


# ------------------------------------------------------------------------------------------------ clamping references --
def test_clamps_change_nothing_in_range():
    rng = np.random.default_rng(0)
    for P in (1, 5, 70):
        G, n = 4, 5
        R = G * P
        anc = (np.arange(R)[None] // P * P + rng.integers(0, P, (n, R))).astype(np.int32)
        picks = rng.integers(0, P, G)
        assert np.array_equal(F.clamp_anc(anc, P), anc) and np.array_equal(F.clamp_picks(picks, P), picks)
        assert np.array_equal(F.clamp_picks([-1, P + 3, 0, P - 1], P), [0, P - 1, 0, P - 1])
    for i, c in enumerate(F.PATH):
        inp = F.path_inputs(i)
        P = c['P']
        out = inp['anc'] != F.clamp_anc(inp['anc'], P)
        assert out.any() == (c['G'] > 1), c['name']         # the table's out-of-range entries, and only those
        clean = np.where(out, F.clamp_anc(inp['anc'], P), inp['anc'])
        a = GR.backtrack_path(F.clamp_picks(inp['picks'], P), clean, inp['hist'], inp['zhist'], inp['brows'], P, c['S'])
        wx, wz, wb, wr = GR.backtrack_path(F.clamp_picks(inp['picks'], P), F.clamp_anc(inp['anc'], P), inp['hist'],
                                           inp['zhist'], inp['brows'], P, c['S'])
        got = dict(x_ref=wx, z_ref=wz, bridge_ref=wb, renewed=wr.astype(np.uint8))
        F.judge_path(c['name'], c, inp, got)
        assert all(np.array_equal(x, y) for x, y in zip(a, (wx, wz, wb, wr)))


def test_judges_accept_the_references_and_name_what_they_reject():
    c, inp = F.GATHER[5], F.gather_inputs(5)
    moved = np.repeat(inp['flag'], c['P']).astype(bool)
    good = [np.where(moved[:, None], o[inp['anc'][c['k']]], o) for o in inp['bufs']]
    F.judge_gather(c['name'], c, inp, c['k'], good)
    F.judge_gather(c['name'], c, inp, -1, inp['bufs'])
    if moved.any():
        with pytest.raises(AssertionError, match="buffer 0"):
            F.judge_gather(c['name'], c, inp, c['k'], inp['bufs'])
    with pytest.raises(AssertionError, match="row 1, note 2"):
        F.check_bits("x", np.array([[0, 0, 0], [0, 0, 1.0]], np.float32), np.zeros((2, 3)), ('row', 'note'))
    assert F.check_close("v", [1.0, 2.0], [1.0, 2.0 + 4e-16], [0.0, 8e-16]) == pytest.approx(0.5, rel=0.2)
    with pytest.raises(AssertionError):
        F.check_close("v", [1.0, np.nan], [1.0, 2.0], [1.0, 1.0])
    with pytest.raises(AssertionError):
        F.check_ell("ell", [0.0, -1.0 - 1e-11], [0.0, -1.0])
    with pytest.raises(AssertionError):
        F.check_ell("ell", [1e-300, -1.0], [0.0, -1.0])
