"""tests/pointwise_reference.py without a GPU: the reference is the oracle; an honest fp32 evaluation of every GPU case passes
with half of every bound to spare, in three summation orders; every planted fault is rejected by at least one GPU case; the
case tables reach the edges they are there for; the flags stay rare; and what the entry points refuse on the host."""
import numpy as np
import pytest

import clvae_amd  # noqa: F401
from clvae_amd import _lib
from oracle import clvae_oracle as O
import pointwise_reference as P

f32, f64 = np.float32, np.float64
ORDERED = ('label_fwd', 'label_bwd', 'gauss_fwd', 'bernoulli_nll') + P.REDUCTIONS


@pytest.fixture(scope="module")
def runs():
    """every (kernel, case, inputs, reference) of the tables, computed once and left unchanged"""
    return [(k, c, d, P.REF[k](**d)) for k, c, d in P.runs()]


def evaluate(k, d, order='forward', fault=None):
    kw = dict(order=order) if k in ORDERED else {}
    if fault is not None:
        kw['fault'] = fault
    return P.F32[k](**d, **kw)


# ------------------------------------------------------------------------------------------ the reference is the oracle --
def test_the_reference_is_the_oracle_on_the_shapes_of_the_one_shape_test():
    """tests/test_gpu_ops.py::test_label_gauss_bernoulli's shapes and expressions"""
    rng = np.random.default_rng(3)
    B, Cn, L, D, R = 37, 10, 3, 88, 101
    C1 = Cn - 1
    wargs, eps = P.r32(rng.standard_normal((B, 2 * C1)) * 0.7), P.r32(rng.standard_normal((B, C1)))
    y = np.eye(Cn)[rng.integers(0, Cn, B)]
    prior = float(f32(0.3))
    m, lv = wargs[:, :C1], wargs[:, C1:]
    w_ref = O.logistic_normal(m, lv, eps)
    klw, dm_kl, dlv_kl = O.kl_w_prior(m, lv, prior)
    wrec, _ = O.cce_keras(w_ref, y, C1)
    r = P.ref_label_fwd(m, lv, eps, y, prior)
    assert np.array_equal(r['w'][0], w_ref) and np.array_equal(r['rowloss'][0][:, 0], klw)
    assert np.array_equal(r['rowloss'][0][:, 1], wrec)
    assert np.array_equal(r['rowloss'][0][:, 2], (w_ref.argmax(1) == y.argmax(1)).astype(float))
    assert not P.ref_label_fwd(m, lv, eps, None, prior)['rowloss'][0][:, 1:].any()
    dw = P.r32(rng.standard_normal((B, Cn)))
    cw, wkl, inv = (float(f32(x)) for x in (0.7, 0.9, 1.0 / B))
    w_in = P.r32(w_ref)
    ds, dlv_s = O.logistic_normal_bwd(w_in, dw + cw * inv * O.cce_keras(w_in, y, C1)[1], lv, eps)
    r = P.ref_label_bwd(m, lv, eps, y, w_in, dw, prior, cw, wkl, inv)
    np.testing.assert_allclose(r['dmean'][0], ds + wkl * inv * dm_kl, rtol=1e-14, atol=1e-300)
    np.testing.assert_allclose(r['dlogvar'][0], dlv_s + wkl * inv * dlv_kl, rtol=1e-14, atol=1e-300)

    za, ez, dz = (P.r32(rng.standard_normal(s)) for s in ((R, 2 * L), (R, L), (R, L)))
    kl_ref, dzm, dzlv = O.kl_gauss(za[:, :L], za[:, L:])
    r = P.ref_gauss_fwd(za, ez)
    assert np.array_equal(r['z'][0], za[:, :L] + np.exp(za[:, L:] / 2) * ez) and np.array_equal(r['rowkl'][0], kl_ref)
    r = P.ref_gauss_bwd(za, ez, dz, 0.25)['dzargs'][0]
    np.testing.assert_allclose(r[:, :L], dz + 0.25 * dzm, rtol=1e-14)
    np.testing.assert_allclose(r[:, L:], dz * ez * 0.5 * np.exp(za[:, L:] / 2) + 0.25 * dzlv, rtol=1e-14, atol=1e-300)

    a = P.r32(rng.standard_normal((R, D)) * 6)
    a[0, :5] = P.r32([20.0, -20.0, 16.2, -16.2, 0.0])
    yy = (rng.random((R, D)) < 0.2).astype(f64)
    loss_ref, g_ref = O.bce_from_logits_keras(a, yy)
    r = P.ref_bernoulli_nll(a, yy, 0.5)
    assert np.array_equal(r['rownll'][0], loss_ref) and np.array_equal(r['dlogits'][0], 0.5 * g_ref)
    # the clip points are the oracle's: a logit just inside has a gradient, one just outside has none
    for clip in (O.LOGIT_CLIP_LO, O.LOGIT_CLIP_HI):
        pts = P.r32([[clip - 1e-3, clip + 1e-3]])
        g = P.ref_bernoulli_nll(pts, np.zeros((1, 2)), 1.0)['dlogits']
        assert (g[0][0] != 0).tolist() == [clip > 0, clip < 0] and not g[2].any()
    assert abs(O.LOGIT_CLIP_HI - 15.942385) < 1e-6 and abs(O.LOGIT_CLIP_LO + 16.118095) < 1e-6


def test_check_names_the_first_offending_index_and_honours_flags():
    want, bound = np.zeros((2, 3)), np.full((2, 3), 1e-6)
    got = want.copy()
    got[1, 0], got[1, 2] = 5e-7, 3e-6
    with pytest.raises(AssertionError, match=r"x\[1, 2\].*1 of 6"):
        P.check('x', got, want, bound)
    flags = np.zeros((2, 3), bool)
    flags[1, 2] = True
    assert P.check('x', got, want, bound, flags) == pytest.approx(0.5)
    got[1, 2] = np.nan                                        # a flagged element must still be a number
    with pytest.raises(AssertionError):
        P.check('x', got, want, bound, flags)
    with pytest.raises(AssertionError, match=r"x\[0\]"):
        P.check_bits('x', np.array([-0.0], f32), np.array([0.0], f32))
    with pytest.raises(AssertionError):
        P.check('x', np.array([1e-30]), np.array([0.0]), np.array([0.0]))
    for order in P.ORDERS:
        assert P.sum32(np.arange(1, 11), 0, order) == 55 and P.sum32(np.ones((3, 5)), 0, order).tolist() == [3] * 5


# ----------------------------------------------------------------------------------------------- honest fp32 passes --
def test_an_honest_fp32_evaluation_keeps_half_of_every_bound(runs):
    worst = {}
    for k, c, d, ref in runs:
        for order in (P.ORDERS if k in ORDERED else P.ORDERS[:1]):
            for o, v in P.check_all("%s %r %s" % (k, c, order), evaluate(k, d, order), ref).items():
                worst[k, o] = max(worst.get((k, o), 0.0), v)
    assert set(k for k, _ in worst) == set(P.REF)
    for ko, v in worst.items():
        assert v <= 0.5, (ko, v)


# ------------------------------------------------------------------------------------------ planted faults are rejected --
@pytest.mark.parametrize("kernel,fault", [(k, f) for k in sorted(P.FAULTS) for f in P.FAULTS[k]])
def test_a_planted_fault_is_rejected_by_some_gpu_case(runs, kernel, fault):
    rejected = []
    for k, c, d, ref in runs:
        if k != kernel:
            continue
        try:
            P.check_all(k, evaluate(k, d, fault=fault), ref)
        except AssertionError as e:
            assert "[" in str(e)                              # the first offending index is named
            rejected.append(c)
    assert rejected, "no case of %s notices: %s" % (kernel, fault)


def test_the_fault_table_lists_22_faults_over_known_kernels():
    assert sum(len(v) for v in P.FAULTS.values()) == 22 and set(P.FAULTS) <= set(P.F32)
    assert set(P.REF) == set(P.F32) == set(k for k, _, _ in P.runs())
    assert all(hasattr(_lib.lib(), 'clv_colsum_f32' if k == 'colsum' else 'clv_' + k) for k in P.REF) and len(P.REF) == 18


# ------------------------------------------------------------------------------------------- the cases reach the edges --
def _values(fam, key):
    return set(c[key] for c in P.CASES[fam])


def test_label_cases_reach_their_edges(runs):
    cs = P.CASES['label']
    assert _values('label', 'B') >= {1, 63, 64, 65, 130} and _values('label', 'C') >= {2, 3, 10, 32}
    assert _values('label', 'prior') >= {0.0, 0.3, -1.0}
    assert any(c['pad_in'] == 0 for c in cs) and any(c['pad_in'] > 0 for c in cs) and any(c['pad_in'] != c['pad_out'] for c in cs)
    assert any(not c['onehot'] for c in cs) and any(not c['rowloss'] for c in cs)
    h = P.LABEL_HAND_ROWS
    hand = [(c, d, ref) for k, c, d, ref in runs if k == 'label_fwd' and c['hand']]
    assert hand
    for c, d, ref in hand:
        W, y = ref['w'][0], d['onehot']
        q = W + O.W2_SHIFT
        n = q / q.sum(1, keepdims=True)
        r = h['clip_out']
        assert n[r][y[r] == 1][0] < 1e-7 and -d['mean'][r, 0] > 17          # the clip-out branch, from a logit gap > 17
        for r in (h['tie_hit'], h['tie_miss']):
            assert len(set(W[r].tolist())) == 1                                # an exact fp64 tie: not flagged
        rl, _, flags = ref['rowloss']
        assert rl[h['tie_hit'], 2] == 1 and rl[h['tie_miss'], 2] == 0
        assert np.flatnonzero(flags[:, 2]).tolist() == [h['near_tie']] and not flags[:, :2].any()
        # zero gradient through the clip: dmean / dlogvar of that row are those of dw alone
        bw = dict((k2, r2) for k2, c2, _, r2 in runs if k2 == 'label_bwd' and c2 is c)['label_bwd']
        alone = P.ref_label_bwd(**dict(d, class_weight=0.0))
        r = h['clip_out']
        assert np.array_equal(bw['dmean'][0][r], alone['dmean'][0][r])
        assert not bw['dmean'][2].any() and not bw['dlogvar'][2].any()       # no row of the backward is exempt from comparison
        assert not np.array_equal(bw['dmean'][0][r + 1], alone['dmean'][0][r + 1])


def test_gauss_and_bernoulli_cases_reach_their_edges():
    cs = P.CASES['gauss']
    lp = lambda L: 1 << (L - 1).bit_length()
    assert set(lp(c['L']) for c in cs) == {1, 2, 4, 8, 16, 32, 64}                 # every instantiation of the forward
    assert _values('gauss', 'L') >= {1, 2, 3, 5, 8, 17, 32, 33, 64} and _values('gauss', 'R') >= {1, 7, 257}
    for L in _values('gauss', 'L'):
        assert set(c['R'] for c in cs if c['L'] == L) >= {1, 7, 257}
    assert _values('gauss', 'pad_z') == {0, 2} and any(c['pad_dz'] for c in cs) and not all(c['rowkl'] for c in cs)
    assert _values('gauss', 'kl_scale') == {0.0, 0.25}
    assert any(33 <= c['L'] <= 64 and c['rowkl'] for c in cs)
    cs = P.CASES['bernoulli_nll']
    for D in (1, 63, 64, 65, 88, 130):
        assert set(c['R'] for c in cs if c['D'] == D) >= {1, 4, 5, 7}
    assert _values('bernoulli_nll', 'pad_y') == {0, 4} and _values('bernoulli_nll', 'scale') == {1.0, 0.5}
    assert any(not c['rownll'] for c in cs) and any(not c['dlogits'] for c in cs) and all(c['rownll'] or c['dlogits'] for c in cs)
    assert any(c['fractional'] for c in cs)
    pt = [c for c in cs if c['points']]
    d = P.bernoulli_inputs(pt[0])
    assert set(P.r32(P.BCE_POINTS)) <= set(d['logits'][0]) and set(d['y'][0]) == {0.0} and set(d['y'][1]) == {1.0}
    assert min(abs(p - clip) for p in P.BCE_POINTS for clip in (O.LOGIT_CLIP_LO, O.LOGIT_CLIP_HI)) >= 1e-3
    assert not P.ref_bernoulli_nll(**d)['dlogits'][2].any()                         # none of the hand-built points is flagged


def loss_route(kind, n):
    """what the launch does with a term: (passes of the unrolled float4 loop, of the single float4 loop, tail elements,
    passes of the unrolled scalar loop, of the single scalar loop), each the largest over the 1024 threads"""
    def loops(count, first):           # a thread starts at `first`: passes of `for (; i + 3072 < count; i += 4096)`, then of the rest
        i, a, b = first, 0, 0
        while i + 3072 < count:
            i, a = i + 4096, a + 1
        while i < count:
            i, b = i + 1024, b + 1
        return a, b
    if kind == 'c':
        n4 = n // 4
        v = [loops(n4, t) for t in (0, 1023)]
        s = [loops(n, 4 * n4 + t) for t in (0, 1023)]
        return max(x[0] for x in v), max(x[1] for x in v), n - 4 * n4, max(x[0] for x in s), max(x[1] for x in s)
    s = [loops(n, t) for t in (0, 1023)]
    return 0, 0, 0, max(x[0] for x in s), max(x[1] for x in s)


def test_reduction_cases_reach_their_edges():
    terms = set(t for launch in P.LOSS_LAUNCHES for t in launch)
    assert terms >= set(('c', n) for n in (1, 3, 4, 5, 4099, 12292, 28695)) | set(('s', n) for n in (29, 3073, 7200)) | {('m', 7201)}
    route = lambda kind, n: tuple(min(v, 2) if i in (0, 3) else v if i == 2 else min(v, 1) for i, v in enumerate(loss_route(kind, n)))
    assert route('c', 28695)[:3] == (2, 1, 3) and route('c', 12292)[:2] == (1, 1) and route('c', 4099)[:3] == (0, 1, 3)
    assert route('c', 5) == (0, 1, 1, 0, 1) and route('c', 3) == (0, 0, 3, 0, 1) and route('c', 4) == (0, 1, 0, 0, 0)
    assert route('s', 3073)[3:] == (1, 1) and route('s', 7200)[3:] == (2, 1) and route('m', 7201)[3:] == (2, 1)
    assert route('s', 29)[3:] == (0, 1)
    for launch in P.LOSS_LAUNCHES[:3]:
        assert len(launch) == 5 and len(set(k for k, _ in launch)) >= 2             # one launch holds different routes
    assert set((c['n'], c['stride']) for c in P.CASES['sum_strided']) >= set((n, s) for n in (1, 63, 1024, 1025, 5000) for s in (1, 3))
    cs = P.CASES['colsum']
    small, two = [c for c in cs if c['M'] <= 1024], [c for c in cs if c['M'] > 1024]
    assert set(c['M'] for c in small) >= {1, 15, 16, 17, 32, 33, 47, 1024}
    assert set((c['M'] + 63) // 64 for c in two) == {17, 20, 33, 34} and any(c['M'] % 64 for c in two)
    for path in (small, two):
        assert set(c['N'] for c in path) >= {1, 64, 65, 90} and set(c['beta'] for c in path) == {0.0, 1.0, 0.5}
        assert any(c['pad_x'] for c in path) and any(not c['pad_x'] for c in path)


def test_elementwise_and_copy_cases_reach_their_edges():
    for fam in ('axpy', 'act_grad', 'scale_temper', 'sigmoid_temper', 'bernoulli_sample'):
        assert _values(fam, 'n') >= {1, 255, 256, 257, 1000}, fam
    assert _values('act_grad', 'act') == {P.ACT_NONE, P.ACT_RELU, P.ACT_SIGMOID} == {_lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_SIGMOID}
    for c in P.CASES['act_grad']:
        y = P.elementwise_inputs('act_grad', c)['y']
        if c['n'] >= 3:
            assert y[0] == 0 and not np.signbit(y[0]) and y[1] == 0 and np.signbit(y[1]) and y[2] == 1
    assert 0.0 in _values('scale_temper', 'alpha')
    prods = np.concatenate([f32(c['alpha']) * P.elementwise_inputs('sigmoid_temper', c)['x'].astype(f32) for c in P.CASES['sigmoid_temper']])
    assert prods.max() > 30 and prods.min() < -30
    for c in P.CASES['bernoulli_sample']:
        d = P.elementwise_inputs('bernoulli_sample', c)
        assert (d['u'] == d['p']).any()
    cs = P.CASES['dropout_rows']
    assert set((c['T'], c['rate'], c['beta']) for c in cs) == set((T, r, b) for T in (1, 3) for r in (0.0, 0.25, 0.5) for b in (0.0, 1.0))
    assert any(all(c['pads']) for c in cs) and all(c['R'] * c['n'] > 256 for c in cs)
    for c in cs:
        d = P.dropout_inputs(c)
        assert (d['Um'] == f32(c['rate'])).any() and (c['rate'] == 0 or (d['Um'] == np.nextafter(f32(c['rate']), f32(0))).any())
        assert (d['X'] != 0).all()
    cs = P.CASES['bernoulli_sample_clamped']
    for D in (3, 88):
        assert set(c['counter'] - c['S'] for c in cs if c['D'] == D) == {-1, 0, 2, 3} and all(c['nsteps'] == 3 for c in cs)
    assert all(set(P.clamped_inputs(c)['clamp'].ravel().tolist()) == {0, 1, 2, 255} for c in cs)
    assert set((c['step'], c['T']) for c in P.CASES['take_frame']) == {(-1, 4), (0, 4), (3, 4), (4, 4)}
    assert _values('lerp_rows', 'n') == {1, 88, 257}
    d = P.lerp_inputs(P.CASES['lerp_rows'][1])
    assert set(d['alpha'].tolist()) >= set(P.r32([0.0, 1.0, 0.5, 1.0 / 3]).tolist())
    assert len(set(d['ia'].tolist())) < len(d['ia']) and (d['ia'] != d['ib']).any() and (d['ia'] == d['ib']).any()
    assert np.abs(d['a'][:4]).mean() > 1e6 * np.abs(d['b'][:5]).mean()
    inner = (d['alpha'] > 0) & (d['alpha'] < 1)
    like = np.abs(d['a'][d['ia']]).mean(1) < 10 * np.abs(d['b'][d['ib']]).mean(1)      # rows where both products count
    assert (inner & like).sum() >= 4 and (inner & ~like).sum() >= 4 and (~inner & like).sum() >= 2
    for c in P.CASES['lerp_rows']:          # the interior blend is held in every case, not only the exact ends
        di = P.lerp_inputs(c)
        with pytest.raises(AssertionError):
            P.check_all('lerp_rows', P.f32_lerp_rows(**di, fault='b dropped inside (0, 1)'), P.ref_lerp_rows(**di))
    vec = lambda c: (c['chunk'] or c['row_elems']) % 4 == 0 and (c['out_ld'] or c['row_elems']) % 4 == 0 and not c['misaligned']
    cs = P.CASES['gather_rows']
    assert any(vec(c) for c in cs) and any(c['chunk'] == 45 and c['out_ld'] == 48 and c['misaligned'] for c in cs)
    assert any(c['chunk'] == 0 and vec(c) for c in cs) and any(c['chunk'] == 0 and not vec(c) for c in cs)
    assert any(c['out_ld'] > c['chunk'] > 0 and vec(c) for c in cs) and any(c['perm'] for c in cs)
    assert any(len(set(P.gather_inputs(c)['idx'].tolist())) < c['rows'] for c in cs)
    assert any(c['rows'] * c['row_elems'] > 4 * 256 for c in cs)                     # more than one block


# ------------------------------------------------------------------------------------------------------ the flag cap --
def test_the_flags_stay_rare(runs):
    """at most 1e-4 of the elements of any random case may be flagged; the hand-built label rows are checked above"""
    for k, c, d, ref in runs:
        for o, (want, bound, flags) in ref.items():
            if flags is None or c.get('hand'):
                continue
            share = np.broadcast_to(flags, want.shape).mean()
            assert share <= 1e-4, (k, c, o, share)
    # the reference alone holds the cap on N(0, 6^2) logits: about 2e-7 of them lie within their bound of a clip point
    rng = np.random.default_rng(11)
    a = P.r32(rng.standard_normal((4000, 500)) * 6)
    flags = P.ref_bernoulli_nll(a, np.zeros(a.shape), 1.0, rownll=False)['dlogits'][2]
    assert flags.mean() <= 1e-4


# ------------------------------------------------------------------------------------------------------ host refusals --
EINVAL, EWORKSPACE = -1, -2
_buffer = np.zeros(64, np.float32)
BUF = _buffer.ctypes.data + (-_buffer.ctypes.data) % 16          # never dereferenced: every call below is refused on the host


def test_what_the_entry_points_refuse():
    L = _lib.lib()
    B = BUF
    for C in (1, 0, -1, 33, 100):
        assert L.clv_label_fwd(4, C, B, B, 2 * (C - 1), B, B, 0.3, B, B, None) == EINVAL
        assert L.clv_label_bwd(4, C, B, B, 2 * (C - 1), B, B, B, B, 0.3, 0.7, 0.9, 0.25, B, B, 2 * (C - 1), None) == EINVAL
    assert L.clv_label_fwd(0, 10, B, B, 18, B, B, 0.3, B, B, None) == EINVAL
    assert L.clv_label_bwd(-1, 10, B, B, 18, B, B, B, B, 0.3, 0.7, 0.9, 0.25, B, B, 18, None) == EINVAL
    assert L.clv_label_bwd(4, 10, B, B, 18, B, None, B, B, 0.3, 0.7, 0.9, 0.25, B, B, 18, None) == EINVAL      # needs onehot
    for R, Ld in ((4, 65), (4, 0), (0, 3), (-2, 3)):
        assert L.clv_gauss_fwd(R, Ld, B, B, B, max(Ld, 1), B, None) == EINVAL
    for R, Ld in ((4, 0), (0, 3)):
        assert L.clv_gauss_bwd(R, Ld, B, B, B, 3, 0.25, B, None) == EINVAL
    for R, D in ((0, 88), (4, 0), (-1, 88)):
        assert L.clv_bernoulli_nll(R, D, B, B, 88, 1.0, B, B, None) == EINVAL
    assert L.clv_bernoulli_nll(4, 88, None, B, 88, 1.0, B, B, None) == EINVAL
    # n % D != 0
    assert L.clv_take_frame(10, 4, 3, B, B, B, None) == EINVAL and L.clv_take_frame(0, 4, 3, B, B, B, None) == EINVAL
    assert L.clv_take_frame(9, 0, 3, B, B, B, None) == EINVAL and L.clv_take_frame(9, 4, 0, B, B, B, None) == EINVAL
    assert L.clv_bernoulli_sample_clamped(10, 3, 2, 1, B, B, B, B, B, None) == EINVAL
    for n, D, nsteps, S in ((0, 3, 2, 1), (9, 0, 2, 1), (9, 3, 0, 1), (9, 3, 2, -1)):
        assert L.clv_bernoulli_sample_clamped(n, D, nsteps, S, B, B, B, B, B, None) == EINVAL
    assert L.clv_bernoulli_sample(0, B, B, B, None) == EINVAL and L.clv_bernoulli_sample(-5, B, B, B, None) == EINVAL
    # dropout: rate in [0, 1) and leading dimensions that hold a row
    for rate in (1.0, -0.25, 1.5, float('nan')):
        assert L.clv_dropout_rows(6, 3, 8, B, 8, B, 8, rate, 0.0, B, 8, None) == EINVAL
    for lds in ((7, 8, 8), (8, 7, 8), (8, 8, 7)):
        assert L.clv_dropout_rows(6, 3, 8, B, lds[0], B, lds[1], 0.25, 0.0, B, lds[2], None) == EINVAL
    for R, T, n in ((0, 3, 8), (6, 0, 8), (6, 3, 0)):
        assert L.clv_dropout_rows(R, T, n, B, 8, B, 8, 0.25, 0.0, B, 8, None) == EINVAL
    # gather_rows: whole pieces, and room for a piece
    assert L.clv_gather_rows(4, 90, B, B, B, 45 + 1, 48, None) == EINVAL              # row_elems % chunk != 0
    assert L.clv_gather_rows(4, 90, B, B, B, 45, 44, None) == EINVAL                  # out_ld < chunk
    assert L.clv_gather_rows(0, 90, B, B, B, 45, 48, None) == EINVAL and L.clv_gather_rows(4, 0, B, B, B, 0, 0, None) == EINVAL
    # colsum: the workspace is required on both paths
    for M in (100, 3000):
        need = L.clv_colsum_workspace_bytes(M, 90)
        assert need == (M + 63) // 64 * 90 * 4
        assert L.clv_colsum_f32(M, 90, B, 90, 0.0, B, None, need, None) == EWORKSPACE
        assert L.clv_colsum_f32(M, 90, B, 90, 0.0, B, B, need - 1, None) == EWORKSPACE
        assert L.clv_colsum_f32(M, 90, B, 90, 0.0, B, B, 0, None) == EWORKSPACE
    assert L.clv_colsum_f32(0, 90, B, 90, 0.0, B, B, 1 << 20, None) == EINVAL
    assert L.clv_colsum_f32(100, 0, B, 90, 0.0, B, B, 1 << 20, None) == EINVAL
    assert L.clv_sum_strided(0, B, 1, 1.0, B, None) == EINVAL and L.clv_sum_strided(-3, B, 1, 1.0, B, None) == EINVAL
    for k in range(5):
        ns = [8] * 5
        ns[k] = 0
        args = [v for n in ns for v in (B, n, 1)]
        assert L.clv_loss_sums(*args, B, None) == EINVAL
    assert L.clv_loss_sums(*([B, 8, 1] * 4 + [None, 8, 1]), B, None) == EINVAL
    # elementwise
    assert L.clv_axpy(0, 1.0, B, B, None) == EINVAL and L.clv_axpy(-1, 1.0, B, B, None) == EINVAL
    for act in (3, -1, 17):
        assert L.clv_act_grad(8, act, B, B, B, None) == EINVAL
    assert L.clv_act_grad(0, _lib.ACT_RELU, B, B, B, None) == EINVAL
    inf, nan = float('inf'), float('nan')
    for v in (0.0, -1.0, inf, -inf, nan):
        assert L.clv_sigmoid_temper(8, B, v, None) == EINVAL, v
    for v in (-1.0, -1e-30, inf, nan):
        assert L.clv_scale_temper(8, B, v, None) == EINVAL, v
    assert L.clv_sigmoid_temper(0, B, 1.0, None) == EINVAL and L.clv_scale_temper(0, B, 1.0, None) == EINVAL
    for R, n in ((0, 8), (8, 0), (-1, 8)):
        assert L.clv_lerp_rows(R, n, B, B, B, B, B, B, None) == EINVAL
    assert L.clv_lerp_rows(1 << 40, 1 << 40, B, B, B, B, B, B, None) == EINVAL
