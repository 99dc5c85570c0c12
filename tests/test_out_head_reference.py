"""CPU: tests/out_head_reference.py, the fp64 reference of clv_out_head_train, against the oracle's formulas -- and the
sensitivity of the comparison tests/test_gpu_out_head.py makes (every output element within its own bound, rms(err / sigma)
<= 1 per tensor of at least 1000 elements, the single-product bound): an fp32 evaluation of the contract passes it with all
nine piece pairs and with the kernel's six, planted faults do not.

Which check rejects which planted fault (printed by each test; R = 300, measured here):
  per element (`violations`), and by the rms criterion as well: the symmetric clip, dl outside the clip, the bias left out
    of a tile, notes 80..87 left out of rownll, the sigmoid's wrong branch, the target from column j + 1 or from pitch 88
    at ldy = 92, scale applied twice, Wo for Wo^T, the last row left out of dWo, a row beyond R, a slab left out, a single
    bf16 piece (2^-9 of every product);
  per element alone: dbo from hs column 87 (dbo has 88 entries, below the rms criterion's 1000);
  by the single-product bound: 5 of 9 piece pairs (a0 b2 left out too), at every output the single-product cases define.
    On the random cases no ELEMENT betrays that fault where the 88 terms of a sum are of like size
    (test_five_of_nine_hides_in_a_dot_product: worst error / bound 0.69 .. 0.95 against 0.1 .. 0.17 unfaulted): what it adds,
    at most 2^-17 of each product with random signs, stays below the bound of an honest fp32 accumulation, KAPPA U
    sum|terms| sqrt(89 / 3) = 33 U sum|terms|.  The rms criterion does see it there (logits 1.08, dhs 1.15 against 0.08
    unfaulted) and so does the per-element bound where one term dominates its sum (dhs through the column scaled by 30:
    2.0), but neither is relied on: the single-product bound is the check for the piece arithmetic."""
import numpy as np
import pytest

from oracle import clvae_oracle as O
import out_head_reference as OR
import vae_reference as VR


# ---- the reference is the oracle ----
@pytest.mark.parametrize("R", [1, 5, 40])
def test_reference_is_the_oracle(R):
    case = OR.make_case(R, R)
    oclip = (O.LOGIT_CLIP_LO, O.LOGIT_CLIP_HI)
    r = OR.ref_case(case, clip=oclip)
    hs, Wo, bo, Y, s = case['hs'], case['Wo'], case['bo'], case['Y'], case['scale']
    a = hs @ Wo + bo                                           # the Dense layer
    loss, g = O.bce_from_logits_keras(a, Y)
    tol = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r['logits'], a, **tol)
    np.testing.assert_allclose(r['rownll'], loss, **tol)
    np.testing.assert_allclose(r['dl'], s * g, **tol)
    np.testing.assert_allclose(r['dhs'], (s * g) @ Wo.T, **tol)     # the Dense layer's gradients
    np.testing.assert_allclose(r['dWo'], hs.T @ (s * g), **tol)
    np.testing.assert_allclose(r['dbo'], (s * g).sum(0), **tol)
    assert (np.abs(a) > 16.2).any() or R == 1                   # the clip branches take part
    for k in OR.OUTPUTS:
        assert np.isfinite(r['b_' + k]).all() and (r['b_' + k] >= 0).all(), k


def test_the_clip_points_are_the_oracles_in_fp32():
    assert np.float32(O.LOGIT_CLIP_LO) == VR.CLIP_LO32 and np.float32(O.LOGIT_CLIP_HI) == VR.CLIP_HI32
    assert OR.CLIP == (float(VR.CLIP_LO32), float(VR.CLIP_HI32)) and -OR.CLIP[0] - OR.CLIP[1] > 0.17      # asymmetric


# ---- the piece emulation ----
def test_pieces_sum_to_x_exactly():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(200000) * np.exp(rng.uniform(-20, 20, 200000)), [0.0, -0.0, 1.0, -1.0, 1e-30, -3e-30],
                        np.exp(rng.uniform(np.log(1e-30), np.log(1e-20), 1000))]).astype(np.float32)
    p0, p1, p2 = OR.split3(x)
    assert np.array_equal(p0.astype(np.float64) + p1.astype(np.float64) + p2.astype(np.float64), x.astype(np.float64))
    for p in (p0, p1, p2):                                      # each piece is a bf16 value
        assert (p.view(np.uint32) & 0xffff == 0).all()
    one = [float(p[0]) for p in OR.split3(np.float32([1.0]))]
    assert one == [1.0, 0.0, 0.0]
    assert all(float(p[0]) == 0.0 for p in OR.split3(np.float32([0.0])))
    # the widths the docstring derives DROP from
    ax = np.abs(x.astype(np.float64))
    assert (np.abs(p1) <= 2.0 ** -8 * ax).all() and (np.abs(p2) <= 2.0 ** -17 * ax).all()
    assert (np.abs(p0) <= (1 + 2.0 ** -8) * ax).all()


def test_six_pair_product_is_within_the_derived_constant():
    rng = np.random.default_rng(1)
    n = 1 << 20
    worst = {}
    for rep in range(2):                                        # 2 M pairs, two distributions
        a = (rng.standard_normal(n) * (1 if rep else np.exp(rng.uniform(-8, 8, n)))).astype(np.float32)
        b = (np.tanh(rng.standard_normal(n)) if rep else rng.uniform(1, 2, n)).astype(np.float32)
        ab = np.abs(a.astype(np.float64) * b.astype(np.float64))
        for pieces in (6, 5):
            e = np.abs(OR.piece_product(a, b, pieces) - a.astype(np.float64) * b.astype(np.float64)) / ab
            worst[pieces] = max(worst.get(pieces, 0.0), float(e.max()))
            if pieces == 5 and rep:
                med5 = float(np.median(e))
    print("6 of 9 pairs: worst relative error %.3f * 2^-24 (derived %.4f); 5 of 9: worst %.1f, median %.1f * 2^-24"
          % (worst[6] / VR.U, OR.DROP / VR.U, worst[5] / VR.U, med5 / VR.U))
    assert worst[6] <= OR.DROP
    assert worst[6] > 0.5 * VR.U                                # the constant is not slack by more than 2
    assert worst[5] > OR.SINGLE['bf16'] and med5 > OR.SINGLE['bf16']      # what the single-product bound has to tell apart


# ---- fp32 evaluations against the criteria ----
def _accept(got, ref, name):
    bad = OR.violations(got, ref) + OR.rms_violations(got, ref)
    rt, rm = OR.ratios(got, ref), OR.rms(got, ref)
    print("%s: worst error / bound %.3g (%s), worst rms(err / sigma) %.3g (%s), flags %s"
          % (name, max(rt.values()), max(rt, key=rt.get), max(rm.values()), max(rm, key=rm.get), OR.flag_counts(ref)))
    assert not bad, "%s: %s" % (name, bad)


@pytest.mark.parametrize("R", [1, 17, 129, 1000, 32768 + 129])
def test_fp32_evaluation_stays_within_bounds(R):
    case = OR.make_case(3 * R + 1, R, ldy=92 if R % 2 else 88)
    refs = {9: OR.ref_case(case, dropped=False), 6: OR.ref_case(case)}
    for pieces in (9, 6):
        for seed in range(2):
            _accept(OR.evaluate32(case, seed, pieces), refs[pieces], "R=%d pieces=%d seed=%d" % (R, pieces, seed))


def test_edge_case_stays_within_bounds_and_flags_by_name():
    case = OR.edge_case(ldy=92)
    ref = OR.ref_case(case)
    fl = ref['flags']['clip_l']
    c0, near = OR.EDGE_COL0, OR.EDGE_NEAR
    assert fl[:2, c0:c0 + near].all()                            # on the clip points and one fp32 step outside them
    assert not fl[:2, c0 + near:c0 + OR.EDGE_PTS.size].any()       # 16.0, 16.1 (between HI and 16.118) and the rest
    assert int(fl.sum()) == 2 * near, np.argwhere(fl)
    lg = ref['logits'][0, c0:c0 + OR.EDGE_PTS.size]
    assert np.array_equal(lg, OR.EDGE_PTS.astype(np.float64))
    # on the points: inside; a step outside, between the two upper clips, far outside: no gradient
    want0 = np.array([0, 1, 0, 1, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0], bool)
    assert np.array_equal(ref['dl'][0, c0:c0 + lg.size] == 0, want0) and np.array_equal(ref['dl'][1, c0:c0 + lg.size] == 0, want0)
    assert (ref['logits'][2:4] == 0).all() and (ref['logits'][:, OR.EDGE_ZERO_COL] == 0).all()
    assert (np.abs(ref['logits'][5:, OR.EDGE_BIG_COL]) > 16.2).any()
    for pieces in (9, 6):
        _accept(OR.evaluate32(case, 1, pieces), OR.ref_case(case, dropped=pieces == 6), "edges pieces=%d" % pieces)


# ---- planted faults ----
def _rejected(got, ref, what, single=None):
    el, rm = OR.violations(got, ref), OR.rms_violations(got, ref)
    sp = OR.single_violations(single[0], got, single[1]) if single else []
    by = [n for n, b in (("per element", el), ("rms", rm), ("single product", sp)) if b]
    print("%s -> rejected by: %s %s" % (what, ", ".join(by) or "NOTHING", (el + rm + sp)[:3]))
    assert by, "planted fault not rejected: " + what
    return by


FAULT_R = 300


@pytest.mark.parametrize("fault", [f for f in OR.FAULTS if f not in ('sym_clip', 'y_pitch88')])
def test_planted_fault_is_rejected(fault):
    case = OR.make_case(11, FAULT_R, ldy=92)
    ref = OR.ref_case(case)
    _accept(OR.evaluate32(case, 0, 6), ref, "unfaulted")
    by = _rejected(OR.evaluate32(case, 0, 6, faults=(fault,)), ref, fault)
    assert "per element" in by


def test_planted_fault_target_pitch_88_at_ldy_92():
    for fill in (np.nan, 0.0):                                  # NaN padding as in the GPU test, and harmless padding
        case = OR.make_case(11, FAULT_R, ldy=92)
        case['Ypad'] = OR.pad_targets(case['Y'], 92, fill)
        by = _rejected(OR.evaluate32(case, 0, 6, faults=('y_pitch88',)), OR.ref_case(case), "y_pitch88 (padding %s)" % fill)
        assert "per element" in by


def test_planted_fault_symmetric_clip():
    case = OR.edge_case()
    ref = OR.ref_case(case)
    between = (ref['logits'] > OR.CLIP[1] + ref['b_logits']) & (ref['logits'] < -OR.CLIP[0] - ref['b_logits'])
    assert between.sum() >= 4                                    # 16.0 and 16.1 in rows 0 and 1
    by = _rejected(OR.evaluate32(case, 0, 6, faults=('sym_clip',)), ref, "sym_clip")
    assert "per element" in by


def test_planted_fault_single_bf16_piece():
    case = OR.make_case(11, FAULT_R)
    by = _rejected(OR.evaluate32(case, 0, 1), OR.ref_case(case), "1 of 9 piece pairs")
    assert "per element" in by


@pytest.mark.parametrize("R", [1, 200])
def test_single_product_cases_tell_six_pairs_from_five(R):
    case = OR.single_case(R, R)
    ref = OR.ref_case(case)
    assert ref['outside'] == 0 and not ref['flags']['clip_l'].any()
    for pieces, kernel in ((9, 'f32'), (9, 'bf16'), (6, 'bf16')):
        got = OR.evaluate32(case, 0, pieces)
        _accept(got, ref, "single R=%d pieces=%d" % (R, pieces))
        sr = OR.single_ratios(case, got, kernel)
        print("single R=%d pieces=%d against the %s bound: %s" % (R, pieces, kernel, sr))
        assert not OR.single_violations(case, got, kernel)
    got = OR.evaluate32(case, 0, 5)
    sr = OR.single_ratios(case, got, 'bf16')
    print("single R=%d pieces=5: %s" % (R, sr))
    assert all(v > 1.0 for k, v in sr.items() if k != 'dbo'), sr   # rejected at every output the case defines
    assert {'logits', 'dhs'} <= set(sr) and (R > 1 or 'dWo' in sr)
    if R == 1:
        assert sr['dbo'] == 0                                    # the ones column (1, 0, 0): no product is touched


def test_five_of_nine_hides_in_a_dot_product():
    """documented, not wished for: in a dot product of 88 terms of like size no element betrays the 5-of-9 fault"""
    case = OR.make_case(11, FAULT_R)
    case['Wo'][:, 3] = OR._f(case['Wo'][:, 3] / 30.0)            # no column that dominates its sums
    ref = OR.ref_case(case)
    for pieces in (6, 5):
        got = OR.evaluate32(case, 0, pieces)
        rt, rm = OR.ratios(got, ref), OR.rms(got, ref)
        print("%d of 9 on a random case: worst error / bound %s; rms %s" % (pieces, {k: round(v, 3) for k, v in rt.items()},
                                                                           {k: round(v, 3) for k, v in rm.items()}))
        assert max(rt.values()) <= 1.0


# ---- the GPU test's cases ----
def test_gpu_cases_cover_the_axes():
    for kernel in ('bf16', 'f32'):
        cs = [c for c in OR.GPU_CASES if c[1] == kernel]
        assert {c[0] for c in cs} == {1, 15, 16, 17, 127, 128, 129, 1000, 32767, 32768, 32769, 32768 + 129, 128 * 513 + 7}
        assert {c[4] for c in cs} == {'both', 'logits', 'dlogits', 'none'}
        assert {c[5] for c in cs} == {None, 1.0, OR.S_ODD}
        for lo, hi in ((127, 129), (32767, 32768 + 129)):
            assert set(''.join(c[6] for c in cs if lo <= c[0] <= hi)) == {'i', 'd'}
        assert any('d' in c[6] for c in cs if c[0] <= 128)        # a job that comes back empty
        if kernel == 'bf16':
            assert {c[3] for c in cs} == {88, 92, 96} and all(c[2] is None for c in cs)
        else:
            assert {c[3] for c in cs if c[2] == 'ldy'} == {89, 91}
            assert {c[2] for c in cs} == {'ldy', 'Y', 'dhs', 'logits', 'dlogits'}
            assert all(c[3] == 88 for c in cs if c[2] != 'ldy')
            assert all(c[4] in ('both', c[2]) for c in cs if c[2] in ('logits', 'dlogits'))


def test_gpu_cases_flag_at_most_1e_4_of_their_logits():
    """the cap that keeps the GPU test from hiding a failure behind widened bounds (the crafted edge case is exempt)"""
    seen = set()
    for R, kernel, how, ldy, stored, scale, red in OR.GPU_CASES:
        if (R, scale) in seen:
            continue
        seen.add((R, scale))
        ref = OR.ref_case(OR.gpu_case(R, 88, scale))
        share = OR.flag_counts(ref)['clip_l'] / ref['logits'].size
        print("R=%d scale=%s: clip_l %d of %d, outside the clip %.2f %%" % (R, scale, OR.flag_counts(ref)['clip_l'], ref['logits'].size,
                                                                         100.0 * ref['outside'] / ref['logits'].size))
        assert share <= 1e-4, (R, share)
        assert R < 100 or ref['outside'] > 0
