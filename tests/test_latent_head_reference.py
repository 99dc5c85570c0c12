"""CPU: tests/latent_head_reference.py, the fp64 reference of clv_latent_head_fwd / clv_latent_head_bwd, against the oracle's
formulas and a finite difference of the loss -- and the sensitivity of the comparison tests/test_gpu_latent_head.py makes
(every output element within its own bound, rms(err / sigma) <= 1 per tensor of at least 1000 elements): honest fp32
evaluations of the contract (sequential and chunked-pairwise sums, expf correctly rounded or perturbed within its budget) pass
it, planted faults do not.

Which criterion rejects which planted fault is printed by each test (-s); measured here: every fault of
latent_head_reference.FAULTS is rejected per element at both templates, by factors of 1e4 and more (a left-out wave, slab or
meeting round, a row beyond R, a stale hs tile, every wrong operand, pitch and arithmetic), and by the rms criterion as well
wherever the faulty tensor has 1000 elements; rows beyond R counted in dbz alone are seen per element only (dbz has 2L
entries).  The one marginal case is written down in test_stale_tile_at_the_kernels_grid: at R = 128 * 256 + 1 a stale tile
touches ONE row of 32769, a single wrong term in each dWz sum, about 10 times its bound.  No fault needed a case of its own.
Shapes: R = 300 (three blocks, a ragged tile of
12 rows) with L = 9 (pitches 12) and L = 32 (pitches 35); the persistent-loop faults with the grid capped at two workgroups
(the kernels cap it at 256: the same pattern at 1/128 of the rows).  Faults that a shape cannot show are run where they can:
'round2_dropped' needs L > 16, 'padded_col' an L that is no multiple of 16."""
import numpy as np
import pytest

from oracle import clvae_oracle as O
import latent_head_reference as LR
import vae_reference as VR


# ---- the reference is the oracle ----
@pytest.mark.parametrize("R,L", [(1, 1), (5, 2), (40, 9), (33, 32)])
def test_reference_is_the_oracle(R, L):
    """the Dense layer, the reparametrisation (O.vrnn_forward: Z_mean, Z_log_var, Z), O.kl_gauss and the gradients of
    O.vrnn_loss_and_grads (dZm, dZlv, the Z_* kernels and biases, d_enc_h) on this layer's tensors"""
    case = LR.make_case(R + L, R, L, wide=True)
    r = LR.ref_case(case, zargs=None)
    hs, Wz, bz, eps, dZ, kl = [case[k] for k in ('hs', 'Wz', 'bz', 'eps', 'dZ', 'kl')]
    zm, zlv = hs @ Wz[:, :L] + bz[:L], hs @ Wz[:, L:] + bz[L:]
    Z = zm + np.exp(zlv / 2) * eps
    klz, dzm_kl, dzlv_kl = O.kl_gauss(zm, zlv)
    tol = dict(rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r['zargs'], np.concatenate([zm, zlv], 1), **tol)
    np.testing.assert_allclose(r['Z'], Z, **tol)
    np.testing.assert_allclose(r['rowkl'], klz, **tol)
    # backward from the reference's own fp64 zargs (the fp32-rounded input is the entry point's, not the model's)
    b = LR.backward_reference(hs, Wz, r['zargs'], eps, dZ, kl)
    dZm = dZ + kl * dzm_kl
    dZlv = dZ * eps * 0.5 * np.exp(zlv / 2) + kl * dzlv_kl
    np.testing.assert_allclose(b['dzargs'], np.concatenate([dZm, dZlv], 1), **tol)
    np.testing.assert_allclose(b['dhs'], dZm @ Wz[:, :L].T + dZlv @ Wz[:, L:].T, **tol)
    np.testing.assert_allclose(b['dWz'], np.concatenate([hs.T @ dZm, hs.T @ dZlv], 1), **tol)
    np.testing.assert_allclose(b['dbz'], np.concatenate([dZm.sum(0), dZlv.sum(0)]), **tol)
    for k in LR.OUTPUTS:
        assert np.isfinite(r['b_' + k]).all() and (r['b_' + k] >= 0).all(), k


def test_gradients_match_a_finite_difference():
    """central differences of the fp64 loss sum(dZ Z) + kl sum(rowkl) in hs, Wz and bz"""
    R, L = 6, 3
    case = LR.make_case(3, R, L, kl=0.31)
    hs, Wz, bz, eps, dZ, kl = [case[k] for k in ('hs', 'Wz', 'bz', 'eps', 'dZ', 'kl')]

    def loss(hs, Wz, bz):
        f = LR.forward_values(LR.A64, hs, Wz, bz, eps)
        return (dZ * f['Z']).sum() + kl * f['rowkl'].sum()
    f = LR.forward_values(LR.A64, hs, Wz, bz, eps)
    b = LR.backward_reference(hs, Wz, f['zargs'], eps, dZ, kl)
    h = 1e-5             # the difference's own error: rounding |loss| 2^-52 / h ~ 1e-9, truncation h^2 f''' / 6 ~ 1e-9
    assert np.abs(b['dbz']).max() > 0.1
    for name, i, got in (('hs', 0, b['dhs']), ('Wz', 1, b['dWz']), ('bz', 2, b['dbz'])):
        args = [hs, Wz, bz]
        fd = np.zeros_like(args[i])
        for idx in np.ndindex(*args[i].shape):
            p, m = [a.copy() for a in args], [a.copy() for a in args]
            p[i][idx] += h
            m[i][idx] -= h
            fd[idx] = (loss(*p) - loss(*m)) / (2 * h)
        np.testing.assert_allclose(got, fd, rtol=1e-6, atol=3e-8, err_msg=name)


# ---- honest fp32 evaluations against the criteria ----
def _accept(got, ref, name):
    bad = LR.violations(got, ref) + LR.rms_violations(got, ref)
    rt, rm = LR.ratios(got, ref), LR.rms(got, ref)
    print("%s: worst error / bound %s | rms(err / sigma) %s" % (name, " ".join("%s %.3g" % kv for kv in rt.items()),
                                                                 " ".join("%s %.3g" % kv for kv in rm.items())))
    assert set(rt) == set(LR.OUTPUTS)
    assert not bad, "%s: %s" % (name, bad)


@pytest.mark.parametrize("R,L,wide", [(300, 9, True), (300, 32, False), (32769, 9, False), (32769, 32, True), (1, 1, False), (17, 16, True)])
def test_fp32_evaluation_stays_within_bounds(R, L, wide):
    case = LR.make_case(3 * R + L, R, L, wide, ldz=L + 3, lddz=L + 8)
    ref = LR.ref_case(case)
    for order, seed in (('seq', None), ('pair', None), ('pair', 1)):
        _accept(LR.evaluate32(case, order, seed, zargs=ref['zargs32']), ref, "R=%d L=%d %s%s" % (R, L, order, '' if seed is None else ' expf perturbed'))


@pytest.mark.parametrize("L,kl_zero", [(9, False), (9, True), (17, False), (1, False)])
def test_edge_case_stays_within_bounds(L, kl_zero):
    case = LR.edge_case(L, kl_zero, ldz=L + 3)
    ref = LR.ref_case(case)
    sd2 = np.exp(ref['zargs'][:, L])
    assert sd2.min() < 1e-17 and sd2.max() > 1e17 and np.isfinite(np.float32(sd2.max()))
    if L >= 2:
        assert (ref['zargs'][:, 1] == 0).all() and (ref['dzargs'][10:40, 1] == 0).all()       # mean = 0 and dZ = 0: no term left
    assert (ref['Z'][:20] == ref['zargs'][:20, :L]).all()                     # eps = 0
    if kl_zero:
        assert (ref['dzargs'][10:40] == 0).all()                              # neither term
    for order, seed in (('seq', None), ('pair', 2)):
        _accept(LR.evaluate32(case, order, seed, zargs=ref['zargs32']), ref, "edges L=%d kl_zero=%s %s" % (L, kl_zero, order))


def test_chained_evaluation_is_judged_from_its_own_zargs():
    """a step feeds the backward pass the forward pass's fp32 zargs: the reference then takes THOSE as its exact input"""
    case = LR.make_case(5, 300, 17, True)
    got = LR.evaluate32(case, 'pair')
    _accept(got, LR.ref_case(case, zargs=got['zargs']), "chained")


# ---- planted faults ----
def _rejected(got, ref, what):
    el, rm = LR.violations(got, ref), LR.rms_violations(got, ref)
    by = [n for n, b in (("per element", el), ("rms", rm)) if b]
    print("%s -> rejected by: %s %s" % (what, ", ".join(by) or "NOTHING", [(k, float("%.3g" % v)) for k, v in (el + rm)[:4]]))
    assert by, "planted fault not rejected: " + what
    return by


FAULT_R = 300
_CASES = {}


def _fault_case(L):
    if L not in _CASES:
        case = LR.make_case(11 + L, FAULT_R, L, wide=False, ldz=L + 3, lddz=L + 3)
        ref = LR.ref_case(case)
        _accept(LR.evaluate32(case, 'pair', 0, zargs=ref['zargs32'], grid=2), ref, "unfaulted L=%d" % L)
        _CASES[L] = (case, ref)
    return _CASES[L]


def _faults_for(L):
    return [f for f in LR.FAULTS if not (f == 'round2_dropped' and L <= 16) and not (f == 'padded_col' and L % 16 == 0)]


@pytest.mark.parametrize("L,fault", [(L, f) for L in (9, 32) for f in _faults_for(L)])
def test_planted_fault_is_rejected(L, fault):
    """every fault at both templates; grid = 2 puts two blocks on workgroup 0 (the stale-tile fault) and block 1 alone in
    a slab (the dropped slab)"""
    case, ref = _fault_case(L)
    by = _rejected(LR.evaluate32(case, 'pair', 0, faults=(fault,), zargs=ref['zargs32'], grid=2), ref, "L=%d %s" % (L, fault))
    assert "per element" in by


def test_planted_faults_with_harmless_padding():
    """the pitch faults do not need the NaN padding to show: zeros in the padding columns of dZ"""
    case, ref = _fault_case(9)
    case = dict(case, dZpad=LR.pad(case['dZ'], case['lddz'], 0.0))
    by = _rejected(LR.evaluate32(case, 'pair', 0, faults=('dZ_pitch_L',), zargs=ref['zargs32']), ref, "dZ_pitch_L (padding 0)")
    assert "per element" in by


def test_stale_tile_at_the_kernels_grid():
    """R = 128 * 256 + 1: ONE row (the single row of block 256) meets workgroup 0's earlier tile.  Forward: its zargs row is
    wrong, per element.  Backward: one wrong term among 32769 in every dWz entry"""
    R, L = LR.BLOCK * LR.GRID + 1, 9
    case = LR.make_case(77, R, L)
    ref = LR.ref_case(case)
    by = _rejected(LR.evaluate32(case, 'pair', faults=('stale_hs_fwd',), zargs=ref['zargs32']), ref, "R=%d stale_hs_fwd" % R)
    assert "per element" in by
    # (the GPU suite's R = 128 * 513 + 7 puts half of the rows behind an earlier tile; even the single row shows)
    by = _rejected(LR.evaluate32(case, 'pair', faults=('stale_hs_bwd',), zargs=ref['zargs32']), ref, "R=%d stale_hs_bwd, one row" % R)
    assert "rms" in by


# ---- the GPU test's cases ----
def test_gpu_cases_cover_the_axes():
    cs = LR.GPU_CASES
    assert 38 <= len(cs) <= 44 and len(set(cs)) == len(cs)
    assert {c[0] for c in cs} == {1, 15, 16, 17, 127, 128, 129, 300, 128 * 256 + 1, 128 * 513 + 7}
    assert {c[1] for c in cs} == {1, 2, 4, 9, 15, 16, 17, 24, 31, 32}
    assert {c[1] for c in cs if c[0] > 300} == {9, 16, 17, 32}
    for R in {c[0] for c in cs}:                                # every R with both templates
        assert {LR.lp16(c[1]) for c in cs if c[0] == R} == {1, 2}, R
    for t in (1, 2):
        ct = [c for c in cs if LR.lp16(c[1]) == t]
        assert {c[2] - c[1] for c in ct} == {0, 3, 8} and {c[3] - c[1] for c in ct} == {0, 3, 8}
        for axis in (4, 6, 7, 8):
            assert {c[axis] for c in ct} == {False, True}, (t, axis)
        assert {c[5] for c in ct} == {'i', 'd'}
        assert any(c[5] == 'd' and c[0] <= 128 for c in ct)       # a deferred job that comes back empty
        assert {c[5] for c in ct if c[0] > 300} == {'i', 'd'}
        assert any(not c[6] for c in ct if c[0] > 300) and any(c[8] for c in ct if c[0] > 300)


def test_bounds_follow_the_stated_rules():
    """one hand-computed element: R = 1, L = 1 -- zargs' variance, Z's and dhs's from the rules of the module docstring"""
    case = LR.make_case(0, 1, 1)
    r = LR.ref_case(case)
    U, sq = VR.U, np.square
    hs, Wz, bz, eps = case['hs'][0], case['Wz'], case['bz'], case['eps'][0, 0]
    v = [sq(U * (np.abs(hs * Wz[:, j]).sum() + abs(bz[j]))) * 89 / 3 + sq(U * r['zargs'][0, j]) for j in (0, 1)]
    np.testing.assert_allclose(r['s_zargs'][0], np.sqrt(v), rtol=1e-12)
    m, lv = r['zargs'][0]
    se = np.exp(lv / 2) * eps
    vz = v[0] + sq(se) * (0.25 * v[1] + sq((VR.EXP_ULP + abs(lv) / 2) * U)) + sq(U * se) + sq(U * (m + se))
    np.testing.assert_allclose(r['s_Z'][0, 0], np.sqrt(vz), rtol=1e-12)
    dz, vdz = r['dzargs'][0], sq(r['s_dzargs'][0])
    vh = vdz @ sq(Wz[0]) + sq(U * np.abs(dz * Wz[0]).sum()) * 2 / 3 + sq(U * r['dhs'][0, 0])
    np.testing.assert_allclose(r['s_dhs'][0, 0], np.sqrt(vh), rtol=1e-12)
    assert np.array_equal(r['b_dhs'], VR.KAPPA * r['s_dhs'])
