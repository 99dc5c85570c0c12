"""tests/window_reference.py without a GPU: the reference is a plain fp64 matrix product; an honest fp32 evaluation of every
GPU case passes with half of every bound to spare, in three summation orders (forward, reversed, and the kernels' own split:
16 partial sums for sparse_dense, 32-row stages for the outer products, 32-input stages inside the window forward's chunks);
every planted fault is rejected by the cases that are there for it; the case tables reach the edges they name; and what the
six entry points refuse on the host."""
import numpy as np
import pytest

import clvae_amd  # noqa: F401
from clvae_amd import _lib
import window_reference as W

f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def runs():
    """every (kernel, case, inputs, reference) of the tables, computed once and left unchanged"""
    return [(k, c, d, W.REF[k](**d)) for k, c, d in W.runs()]


# ----------------------------------------------------------------------------------- the reference is a plain product --
def test_the_reference_is_the_plain_fp64_product_on_the_shapes_of_the_one_shape_tests():
    """the shapes and expressions of tests/test_gpu_ops.py's tests of these kernels (the 1024 x 22528 ones left out)"""
    f8 = lambda a: np.asarray(a, f32).astype(f64)
    rng = np.random.default_rng(5)
    for R, nx, Nn, ldx, dense in ((1, 88, 352, 88, False), (7, 88, 352, 92, False), (33, 90, 352, 92, True), (515, 16, 64, 16, True)):
        X = np.full((R, ldx), 7.0)
        X[:, :nx] = f8(rng.standard_normal((R, nx))) if dense else rng.random((R, nx)) < 0.05
        K = f8(rng.standard_normal((nx, Nn)))
        want = f8(X[:, :nx]) @ K
        assert np.array_equal(W.ref_sparse_proj(X, nx, Nn, K, exact=False)['out'][0], want)
        ex = W.ref_sparse_proj(X, nx, Nn, K)['out']
        assert (ex[1] is None) == (not dense) and np.allclose(ex[0], want, rtol=1e-5, atol=1e-5)
    for R, nx, Nn, dense, relu in ((5, 11264, 88, False, True), (3, 200, 18, True, False), (2, 64, 128, True, True)):
        X = f8(rng.standard_normal((R, nx))) if dense else (rng.random((R, nx)) < 0.0443).astype(f64)
        K, bias = f8(rng.standard_normal((nx, Nn)) * 0.1), f8(rng.standard_normal(Nn))
        want = X @ K + bias
        got = W.ref_sparse_dense(X, nx, Nn, K, bias, W.ACT_RELU if relu else W.ACT_NONE)['out'][0]
        assert np.array_equal(got, np.maximum(want, 0.0) if relu else want)
    for Bn, nx, Nn, kind in ((100, 130, 88, 'notes'), (300, 70, 18, 'dense'), (1, 64, 2, 'dense'), (100, 132, 88, 'bytes'),
                             (37, 96, 20, 'notes'), (1, 4, 4, 'bytes'), (33, 200, 96, 'bytes')):
        X = f8(rng.standard_normal((Bn, nx))) if kind == 'dense' else W.frames(rng, Bn, nx, nx, kind)
        G, H, hb = f8(rng.standard_normal((Bn, Nn))), f8(np.maximum(rng.standard_normal((Bn, Nn)), 0)), f8(rng.standard_normal(Nn))
        r = W.ref_outer(X, nx, Nn, G, colsum=True, H=H, hb=hb)
        assert np.array_equal(r['out'][0], f8(X).T @ G) and np.array_equal(r['colsum'][0], G.sum(0))
        assert np.array_equal(r['gdot'][0], ((H - hb) * G).sum(0))
        assert set(W.ref_outer(X, nx, Nn, G)) == {'out'}
    for Bn, nx, Nn, kind in ((100, 136, 88, 'bytes'), (37, 96, 20, 'notes'), (1, 8, 4, 'bytes'), (70, 2000, 96, 'bytes')):
        X, K = W.frames(rng, Bn, nx, nx, kind), f8(rng.standard_normal((nx, Nn)))
        r = W.ref_dense_window_fwd_bf16(X, nx, Nn, K)
        assert np.array_equal(r['sum'][0], f8(X) @ K)
        np.testing.assert_allclose(r['part'][0].sum(0), f8(X) @ K, rtol=1e-12, atol=1e-9)
        assert np.allclose(r['part'][1].sum(0), r['sum'][1], rtol=1e-12)               # the chunks' bounds add up to the row's
        L = _lib.lib()
        splits, chunk = W.window_split(Bn, nx)
        assert splits == L.clv_dense_window_fwd_bf16_splits(Bn, nx) == r['part'][0].shape[0]
        assert L.clv_dense_window_fwd_bf16_workspace_bytes(Bn, nx, Nn) == splits * Bn * Nn * 4
    assert (W.ACT_NONE, W.ACT_RELU) == (_lib.ACT_NONE, _lib.ACT_RELU)


def test_the_window_split_is_the_librarys_on_every_case_and_beyond():
    L = _lib.lib()
    for Bn in (1, 15, 16, 17, 63, 64, 65, 130, 256, 1024, 4100, 16384, 20000):
        for nx in (8, 32, 40, 64, 120, 128, 136, 200, 520, 2000, 11264, 22528):
            splits, chunk = W.window_split(Bn, nx)
            assert splits == L.clv_dense_window_fwd_bf16_splits(Bn, nx), (Bn, nx)
            assert chunk % 32 == 0 and (splits - 1) * chunk < nx <= splits * chunk
            for Nn in (4, 96):
                assert L.clv_dense_window_fwd_bf16_workspace_bytes(Bn, nx, Nn) == splits * Bn * Nn * 4


def test_check_names_the_worst_index_and_its_multiple_of_the_bound():
    want, bound = np.zeros((2, 3)), np.full((2, 3), 1e-6)
    got = want.copy()
    got[0, 1], got[1, 2] = 2e-6, 3e-6
    with pytest.raises(AssertionError, match=r"x\[1, 2\].* = 3 x its bound.*2 of 6"):
        W.check('x', got, want, bound)
    got[1, 2] = np.nan
    with pytest.raises(AssertionError, match=r"x\[1, 2\]"):
        W.check('x', got, want, bound)
    with pytest.raises(AssertionError):
        W.check('x', np.array([1e-30]), np.array([0.0]), np.array([0.0]))          # bound 0: equal as numbers
    assert W.check('x', np.array([-0.0]), np.array([0.0]), np.array([0.0])) == 0
    with pytest.raises(AssertionError, match=r"x\[0\]"):
        W.check_bits('x', np.array([-0.0], f32), np.array([0.0], f32))
    t = lambda i: np.array([i + 1], f32)
    for order in W.ORDERS:
        assert W.acc32(10, t, (1,), order, lambda i: i % 3)[0] == 55
    assert W.bf16(np.array([1.0, 255.0, 257.0, 1.00390625], f32)).tolist() == [1.0, 255.0, 256.0, 1.0]
    assert W.seven_bits(np.array([0.0, 1.0, 128.0, 129.0, 255.0], f32)).tolist() == [0.0, 1.0, 128.0, 128.0, 254.0]
    g = np.array([np.pi, -1e-3 / 3, 12345.678], f32)
    assert np.all(W.two_pieces(g) != g) and np.allclose(W.two_pieces(g), g, rtol=2.0 ** -15)


# ----------------------------------------------------------------------------------------------- honest fp32 passes --
def test_an_honest_fp32_evaluation_keeps_half_of_every_bound(runs):
    worst = {}
    for k, c, d, ref in runs:
        bounded = None
        for order in W.ORDERS:
            r = ref
            if order != 'forward' and any(v[1] is None for v in ref.values()):          # exact: in the documented order only
                r = bounded = bounded or W.REF[k](**d, exact=False)
            for o, v in W.check_all("%s %r %s" % (k, c, order), W.F32[k](**d, order=order), r).items():
                worst[k, o] = max(worst.get((k, o), 0.0), v)
    assert set(k for k, _ in worst) == set(W.REF)
    for ko, v in worst.items():
        assert v <= 0.5, (ko, v)


def test_the_gdot_identity_holds_in_the_reference(runs):
    """gdot = sum_j K dK where H = relu(X K + hb) and G is masked by H > 0: what the optimizer relies on"""
    seen = 0
    for k, c, d, ref in runs:
        if k in ('sparse_outer', 'dense_outer_bf16') and c.get('chain'):
            seen += 1
            K = W.r32(d['K'])
            want = (K * ref['out'][0]).sum(0)
            bound = ref['gdot'][1] + (np.abs(K) * ref['out'][1]).sum(0)
            assert W.check('gdot against sum K dK', ref['gdot'][0], want, bound) <= 0.5
            assert (W.used(d['G'], d['N']) == 0).mean() > 0.2 and (W.used(d['G'], d['N']) != 0).mean() > 0.2
    assert seen >= 2


# ------------------------------------------------------------------------------------------ planted faults are rejected --
@pytest.mark.parametrize("kernel,fault", [(k, f) for k in W.FAULTS for f in W.FAULTS[k]])
def test_a_planted_fault_is_rejected_by_the_cases_that_are_there_for_it(runs, kernel, fault):
    must, harmless = W.FAULTS[kernel][fault], W.HARMLESS.get(fault, lambda c: False)
    expected = 0
    if must is None:                                          # a fault that the kernel's contract makes harmless on every case
        must, harmless, expected = (lambda c: False), (lambda c: True), 1
    for k, c, d, ref in runs:
        if k != kernel:
            continue
        try:
            W.check_all(k, W.F32[k](**d, fault=fault), ref)
            rejected = False
        except AssertionError as e:
            assert "[" in str(e)                              # the offending index is named
            rejected = True
        if must(c):
            expected += 1
            assert rejected, "%s %r does not notice: %s" % (kernel, c, fault)
        if harmless(c):
            assert not rejected, "%s %r rejects what changes nothing for it: %s" % (kernel, c, fault)
    assert expected, "no case of %s is there for: %s" % (kernel, fault)


def test_the_fault_table_covers_the_list():
    assert set(W.FAULTS) == set(W.REF) == set(W.F32) == set(W.CASES) == set(k for k, _, _ in W.runs())
    every = set(f for v in W.FAULTS.values() for f in v)
    assert every >= {W.F_LAST, W.F_LASTCH, W.F_FIFTH, W.F_IN_LAST, W.F_IN64, W.F_IN65, W.F_PAD, W.F_ROW, W.F_CLAMP, W.F_GLOW,
                     W.F_KLOW, W.F_XBF16, W.F_X7, W.F_TWICE, W.F_NONE, W.F_LDX, W.F_LDG, W.F_LDK, W.F_LDH, W.F_HB, W.F_NOBIAS,
                     W.F_COL_LAST, W.F_COL64, W.F_NX2}
    assert sum(len(v) for v in W.FAULTS.values()) == 65
    L = _lib.lib()
    assert all(hasattr(L, 'clv_' + k) for k in W.REF)
    # every uint8 value is a bf16 number: rounding X to bf16 cannot show on byte frames, one bit fewer does
    b = np.arange(256).astype(f32)
    assert np.array_equal(W.bf16(b), b) and not np.array_equal(W.seven_bits(b), b) and np.array_equal(W.seven_bits(b[:2]), b[:2])


# ------------------------------------------------------------------------------------------- the cases reach the edges --
def _values(k, key):
    return set(c[key] for c in W.CASES[k])


def _strided(k, *pairs):
    """a kernel's table holds a padded and (where the old tests' shapes are kept) an unpadded case of every stride"""
    for ld, n in pairs:
        assert any(c[ld] > c[n] for c in W.CASES[k]), (k, ld)


def test_every_table_has_an_all_zero_and_an_all_ones_row(runs):
    for kernel in W.CASES:
        found = set()
        for k, c, d, ref in runs:
            if k == kernel:
                for s in d.get('sets', [d]):
                    x = W.used(s['X'], s['nx'])
                    found |= set(v for v in (0, 1) if (x == v).all(1).any())
        assert found == {0, 1}, kernel
    kinds = dict(sparse_proj={'notes', 'bytes', 'dense'}, sparse_proj2={'notes', 'bytes', 'dense'}, sparse_dense={'notes', 'dense'},
                 sparse_outer={'notes', 'dense'}, dense_outer_bf16={'notes', 'bytes'}, dense_window_fwd_bf16={'notes', 'bytes'})
    for k, want in kinds.items():
        assert _values(k, 'kind') == want, k
    for k, c, d, ref in runs:
        for s in d.get('sets', [d]):
            x = W.used(s['X'], s['nx'])
            if c['kind'] == 'dense' and x.size > 500:
                assert (x == 0).any() and np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
            pad = np.asarray(s['X'])[:, s['nx']:]
            assert (pad == (W.PAD_F if c['kind'] == 'dense' else W.PAD_U8)).all()
    for k, c, d, ref in runs:                                          # all-zero inputs: bound 0 (or the exact +0)
        if k in ('sparse_outer', 'dense_outer_bf16') and c['nx'] > 3 and c['seed'] % 2 == 0:
            assert (ref['out'][0][2] == 0).all() and (ref['out'][1][2] == 0).all()
        if k == 'sparse_dense' and c['R'] >= 3 and not c['hand'] and not c['bias']:
            assert (ref['out'][1][0] == 0).all()
        if k == 'dense_window_fwd_bf16' and c['Bn'] >= 3:
            assert (ref['part'][1][:, 0] == 0).all() and (ref['sum'][1][0] == 0).all() and (ref['sum'][1][1] > 0).all()


def test_sparse_proj_cases_reach_their_edges(runs):
    L = _lib.lib()
    shapes = set((c['nx'], c['N']) for c in W.CASES['sparse_proj'])
    assert shapes >= {(88, 352), (1, 4), (4, 1), (64, 64), (65, 64), (128, 300), (100, 384), (4, 63), (4, 65), (90, 352), (16, 64)}
    assert all(L.clv_sparse_proj_supported(nx, Nn) for nx, Nn in shapes)
    assert L.clv_sparse_proj_lds_bytes(100, 384) == 150 * 1024                       # the exact LDS limit
    for nx, Nn in ((128, 384), (129, 4), (3, 3), (4, 385)):
        assert not L.clv_sparse_proj_supported(nx, Nn), (nx, Nn)
    assert _values('sparse_proj', 'R') >= {1, 15, 16, 17, 4095, 4096, 4097} and _values('sparse_proj2', 'R') >= {2047, 2048, 2049}
    # the row split: below, at and over the cap of 256 workgroups (128 per projection of a pair); workgroups without a frame
    wg = lambda k, n: dict((c['R'], W.proj_workgroups(c['R'], n)) for c in W.CASES[k])
    one, two = wg('sparse_proj', 1), wg('sparse_proj2', 2)
    assert one[4095][:2] == (256, 16) and one[4096][:2] == (256, 16) and one[4097][:2] == (256, 17) and one[4097][2] > 0
    assert one[17][:2] == (2, 9) and one[1][:2] == (1, 1) and one[15][0] == 1 and one[16][0] == 1
    assert two[2047][:2] == (128, 16) and two[2048][:2] == (128, 16) and two[2049][:2] == (128, 17) and two[2049][2] > 0
    # the staging loop moves 4 float4 per thread and pass: fewer than one pass's 4096, and no multiple of it
    nv = set(c['nx'] * c['N'] // 4 for c in W.CASES['sparse_proj'])
    assert min(nv) == 1 and any(v < 4096 for v in nv) and any(v > 4096 and v % 4096 for v in nv)
    _strided('sparse_proj', ('ldx', 'nx'), ('ldo', 'N'))
    assert any(c['ldx'] == c['nx'] and c['ldo'] == c['N'] for c in W.CASES['sparse_proj'])
    for kind in ('notes', 'bytes', 'dense'):
        assert any(c['kind'] == kind and c['ldx'] > c['nx'] for c in W.CASES['sparse_proj']), kind
    cs = W.CASES['sparse_proj2']
    assert any(a != b and la != lb and la == a and lb > b for (a, la), (b, lb) in (c['sets'] for c in cs))          # 88 / 88 and 70 / 92
    assert any(a < b for (a, _), (b, _) in (c['sets'] for c in cs)) and any(a > b for (a, _), (b, _) in (c['sets'] for c in cs))
    assert any(c['ldo'] > c['N'] for c in cs) and any(max(a, b) * c['N'] * 4 == 150 * 1024 for c in cs for (a, _), (b, _) in [c['sets']])
    # 0 / 1 frames are compared bit for bit, the others are not
    for k, c, d, ref in runs:
        if k in ('sparse_proj', 'sparse_proj2'):
            assert all((v[1] is None) == (c['kind'] == 'notes') for v in ref.values()), c


def test_sparse_dense_and_sparse_outer_cases_reach_their_edges(runs):
    cs = W.CASES['sparse_dense']
    assert _values('sparse_dense', 'N') >= {2, 18, 88, 128} and _values('sparse_dense', 'R') >= {1, 5}
    assert _values('sparse_dense', 'nx') >= {1, 63, 64, 65, 200, 1024, 1030, 11264}
    chunks = set(-(-c['nx'] // 64) for c in cs)
    assert min(chunks) == 1 and 16 in chunks and 17 in chunks and max(chunks) == 176 and any(c['nx'] % 64 for c in cs)
    assert set((c['bias'], c['act']) for c in cs) == {(True, W.ACT_RELU), (True, W.ACT_NONE), (False, W.ACT_RELU), (False, W.ACT_NONE)}
    _strided('sparse_dense', ('ldx', 'nx'), ('ldo', 'N'))
    for k, c, d, ref in runs:
        if k != 'sparse_dense':
            continue
        if c['act'] == W.ACT_RELU:                                        # pre-activations of both signs
            pre = W.ref_sparse_dense(**dict(d, act=W.ACT_NONE))['out'][0]
            assert (pre < 0).any() and (pre > 0).any(), c
        if c['hand']:
            x = W.used(d['X'], d['nx'])
            assert (x[:, :64] != 0).sum(1).tolist() == list(W.HAND_COUNTS) and ((x[:, 64:128] != 0).sum(1) == 64).all()
    assert sum(c['hand'] for c in cs) >= 2 and set(c['kind'] for c in cs if c['hand']) == {'notes', 'dense'}
    cs = W.CASES['sparse_outer']
    assert _values('sparse_outer', 'Bn') >= {1, 127, 128, 129, 257} and _values('sparse_outer', 'nx') >= {1, 63, 64, 65, 130}
    assert _values('sparse_outer', 'N') >= {2, 18, 88, 128}
    assert set((c['colsum'], c['gdot']) for c in cs) == {(False, False), (True, False), (False, True), (True, True)}
    _strided('sparse_outer', ('ldx', 'nx'), ('ldg', 'N'), ('ldo', 'N'), ('ldh', 'N'))
    assert all(c['ldg'] % 2 == 0 and c['ldh'] % 2 == 0 for c in cs) and any(c['ldo'] % 2 for c in cs) and any(c['ldx'] % 2 for c in cs)
    assert any(c['gdot'] and c['Bn'] % 128 for c in cs) and any(c['gdot'] and c['Bn'] % 16 for c in cs)
    assert any(c['chain'] and c['gdot'] and c['colsum'] for c in cs)


def test_dense_outer_cases_reach_their_edges():
    L = _lib.lib()
    cs = W.CASES['dense_outer_bf16']
    assert _values('dense_outer_bf16', 'Bn') >= {1, 31, 32, 33, 96, 128, 129, 161} | {2, 3, 7, 25, 49}
    assert set(-(-c['Bn'] // 32) for c in cs) >= {1, 2, 3, 4, 5, 6}                      # stages: around the pipeline's period of 4
    assert _values('dense_outer_bf16', 'nx') >= {4, 44, 48, 52, 100, 9504, 9508, 9600} and _values('dense_outer_bf16', 'N') >= {4, 20, 92, 96}
    # both wave counts, by the launch rule: 6 waves (96 inputs a workgroup) from 100 such tiles on
    waves = dict((c['nx'], W.outer_waves(c['nx'])) for c in cs)
    assert waves[9504] == 3 and -(-9504 // 96) == 99 and waves[9508] == 6 and 9508 % 96 and waves[9600] == 6 and 9600 % 96 == 0
    assert all(w == 3 for nx, w in waves.items() if nx <= 100) and all(c['Bn'] <= 33 for c in cs if c['nx'] > 9000)
    # the extra workgroup's rounds of 8 rows per wave: fewer rows than waves, and one row more than 8 rounds
    assert any(c['Bn'] < 3 for c in cs) and any(c['Bn'] == 8 * 3 + 1 and W.outer_waves(c['nx']) == 3 for c in cs)
    assert any(c['Bn'] == 4 * 6 + 1 and W.outer_waves(c['nx']) == 6 for c in cs) and any(c['Bn'] == 8 * 6 + 1 for c in cs)
    for nx in (9504, 9508, 9600):
        assert all(c['colsum'] and c['gdot'] for c in cs if c['nx'] == nx)
    assert set((c['colsum'], c['gdot']) for c in cs) == {(False, False), (True, False), (False, True), (True, True)}
    _strided('dense_outer_bf16', ('ldx', 'nx'), ('ldg', 'N'), ('ldo', 'N'), ('ldh', 'N'))
    assert all(c['ldx'] % 4 == 0 and c['ldg'] % 4 == 0 and c['ldh'] % 2 == 0 for c in cs) and any(c['ldo'] % 2 for c in cs)
    for kind in ('notes', 'bytes'):
        assert any(c['kind'] == kind and c['ldx'] > c['nx'] and c['ldg'] > c['N'] for c in cs)
    assert all(L.clv_dense_outer_bf16_supported(c['Bn'], c['nx'], c['N'], c['ldx'], c['ldg']) for c in cs)
    for Bn, nx, Nn, ldx, ldg in ((33, 48, 100, 48, 100), (33, 48, 2, 48, 4), (33, 6, 4, 8, 4), (33, 48, 4, 50, 4), (33, 48, 4, 48, 6)):
        assert not L.clv_dense_outer_bf16_supported(Bn, nx, Nn, ldx, ldg), (Bn, nx, Nn, ldx, ldg)


def test_window_fwd_cases_reach_their_edges():
    L = _lib.lib()
    cs = W.CASES['dense_window_fwd_bf16']
    assert _values('dense_window_fwd_bf16', 'Bn') >= {1, 15, 16, 17, 63, 64, 65, 130}
    assert _values('dense_window_fwd_bf16', 'nx') >= {8, 32, 40, 64, 128, 136, 200, 520, 2000} and _values('dense_window_fwd_bf16', 'N') >= {4, 20, 92, 96}
    st = [W.window_stages(c['Bn'], c['nx']) for c in cs]
    assert ([1], [8], [8]) in st                                                     # a single partial stage: 8 of 32 inputs
    assert any(n[-1] > 1 and last[-1] == 8 for n, last, _ in st)                   # a chunk whose last stage holds 8 of 32
    assert any(len(n) > 1 and size[-1] < size[0] for n, _, size in st)             # a last chunk shorter than the others
    assert set(v for n, _, _ in st for v in n) >= {1, 2, 3, 4, 5}                    # stages per chunk, around the period of 4
    assert any(len(n) > 1 and n[0] == 5 for n, _, _ in st) and max(len(n) for n, _, _ in st) >= 21
    _strided('dense_window_fwd_bf16', ('ldx', 'nx'), ('ldk', 'N'))
    for kind in ('notes', 'bytes'):
        assert any(c['kind'] == kind and c['ldx'] > c['nx'] for c in cs) and any(c['kind'] == kind and c['ldk'] > c['N'] for c in cs)
    assert all(L.clv_dense_window_fwd_bf16_supported(c['Bn'], c['nx'], c['N'], c['ldx'], c['ldk']) for c in cs)
    for Bn, nx, Nn, ldx, ldk in ((17, 12, 4, 12, 4), (17, 64, 98, 64, 100), (17, 64, 4, 64, 6)):
        assert not L.clv_dense_window_fwd_bf16_supported(Bn, nx, Nn, ldx, ldk), (Bn, nx, Nn, ldx, ldk)


# ------------------------------------------------------------------------------------------------------ host refusals --
EINVAL, EWORKSPACE = -1, -2
_buffer = np.zeros(64, np.float32)
BUF = _buffer.ctypes.data + (-_buffer.ctypes.data) % 16          # never dereferenced: every call below is refused on the host


def test_what_the_entry_points_refuse():
    L = _lib.lib()
    B, B4, B8 = BUF, BUF + 4, BUF + 8
    # sparse_proj(R, nx, N, X, x_u8, ldx, K, out, ldo)
    ok = dict(R=7, nx=88, N=352, X=B, u8=0, ldx=88, K=B, out=B, ldo=352)
    proj = lambda **kw: L.clv_sparse_proj(*dict(ok, **kw).values(), None)
    for kw in (dict(ldx=87), dict(ldo=351), dict(R=0), dict(R=-3), dict(K=B4), dict(K=B8), dict(nx=128, ldx=128, N=384, ldo=384),
               dict(nx=129, ldx=129), dict(nx=3, ldx=3, N=3), dict(N=385, ldo=385), dict(X=None), dict(K=None), dict(out=None),
               dict(u8=1, ldx=87)):
        assert proj(**kw) == EINVAL, kw
    pair = lambda **kw: L.clv_sparse_proj2(*dict(dict(R=7, N=352, ldo=352, u8=0, nx0=88, X0=B, ldx0=88, K0=B, out0=B, nx1=70, X1=B,
                                                      ldx1=92, K1=B, out1=B), **kw).values(), None)
    for kw in (dict(ldx1=69), dict(ldx0=87), dict(ldo=351), dict(R=0), dict(K1=B4), dict(nx1=129, ldx1=132), dict(out1=None)):
        assert pair(**kw) == EINVAL, kw
    # sparse_dense(R, nx, N, X, ldx, K, bias, act, out, ldo)
    ok = dict(R=5, nx=200, N=18, X=B, ldx=200, K=B, bias=None, act=_lib.ACT_RELU, out=B, ldo=18)
    dense = lambda **kw: L.clv_sparse_dense(*dict(ok, **kw).values(), None)
    for kw in (dict(ldx=199), dict(ldo=17), dict(N=17), dict(N=130, ldo=130), dict(N=0), dict(act=_lib.ACT_SIGMOID), dict(act=-1),
               dict(act=7), dict(R=0), dict(R=-1), dict(nx=0), dict(K=B4), dict(X=None), dict(out=None)):
        assert dense(**kw) == EINVAL, kw
    # sparse_outer / dense_outer_bf16(Bn, nx, N, X, [x_u8,] ldx, G, ldg, out, ldo, colsum, Hact, ldh, hbias, gdot)
    ok = dict(Bn=33, nx=48, N=20, X=B, u8=0, ldx=48, G=B, ldg=20, out=B, ldo=20, colsum=B, H=B, ldh=20, hb=B, gdot=B)
    def souter(**kw):
        a = dict(ok, **kw)
        del a['u8']
        return L.clv_sparse_outer(*a.values(), None)
    bouter = lambda **kw: L.clv_dense_outer_bf16(*dict(ok, **kw).values(), None)
    both = (dict(ldx=47), dict(ldo=19), dict(ldg=19), dict(ldg=18), dict(ldg=21), dict(ldh=21), dict(ldh=18), dict(H=None), dict(hb=None),
            dict(H=B4), dict(G=B4), dict(Bn=0), dict(nx=0), dict(X=None), dict(G=None), dict(out=None), dict(N=19, ldg=20))
    for kw in both:
        assert souter(**kw) == EINVAL, kw
        assert bouter(**kw) == EINVAL, kw
    assert souter(N=130, ldg=130, ldo=130, ldh=130) == EINVAL
    for kw in (dict(N=100, ldg=100, ldo=100, ldh=100), dict(N=2, ldg=4), dict(nx=6, ldx=8), dict(ldx=50), dict(ldg=22), dict(G=B8),
               dict(X=B4), dict(X=B8), dict(u8=1, X=B + 1), dict(u8=1, X=B + 2), dict(u8=1, ldx=50)):
        assert bouter(**kw) == EINVAL, kw
    # dense_window_fwd_bf16(Bn, nx, N, X, x_u8, ldx, K, ldk, part, part_bytes)
    need = L.clv_dense_window_fwd_bf16_workspace_bytes(17, 200, 20)
    assert need == 3 * 17 * 20 * 4
    ok = dict(Bn=17, nx=200, N=20, X=B, u8=0, ldx=200, K=B, ldk=20, part=B, nbytes=need)
    win = lambda **kw: L.clv_dense_window_fwd_bf16(*dict(ok, **kw).values(), None)
    for kw in (dict(nx=12, ldx=12), dict(N=98, ldk=100), dict(ldk=22), dict(ldk=16), dict(ldx=196), dict(ldx=202), dict(Bn=0),
               dict(X=B4), dict(X=B8), dict(K=B4), dict(K=B8), dict(u8=1, X=B + 2), dict(u8=1, X=B + 1), dict(X=None), dict(K=None)):
        assert win(**kw) == EINVAL, kw
    for kw in (dict(nbytes=need - 1), dict(nbytes=0), dict(part=None)):
        assert win(**kw) == EWORKSPACE, kw


def test_a_pair_launch_refuses_to_mix_byte_and_float_frames():
    torch = pytest.importorskip("torch")
    from clvae_amd import ops
    xf, xb, k, o = torch.zeros(4, 8), torch.zeros(4, 8, dtype=torch.uint8), torch.zeros(8, 4), torch.zeros(4, 4)
    with pytest.raises(TypeError):
        ops.sparse_proj2(4, 4, (8, xf, 8, k, o), (8, xb, 8, k, o))
    with pytest.raises(TypeError):
        ops.sparse_proj2(4, 4, (8, xb, 8, k, o), (8, xf, 8, k, o))
