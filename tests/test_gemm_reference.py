"""CPU: tests/gemm_reference.py, the fp64 reference of the fp32 GEMM family, against independent numpy and oracle
expressions -- and the sensitivity of the comparisons tests/test_gpu_gemm.py makes (integer cases bit for bit, per-element
bounds, the exact fp32 fma chain), so that the GPU test is known to catch subtle faults without a GPU."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import clvae_oracle as O
import gemm_reference as GR


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


# ---- the reference is the contract ----
@pytest.mark.parametrize("act", [GR.ACT_NONE, GR.ACT_RELU, GR.ACT_SIGMOID, GR.ACT_MASKPOS])
def test_gemm_reference_is_the_contract(act):
    rng = np.random.default_rng(act)
    M, N, K = 7, 5, 9
    A, B = f32(rng.standard_normal((M, K))), f32(rng.standard_normal((K, N)))
    bias, C0, aux = f32(rng.standard_normal(N)), f32(rng.standard_normal((M, N))), f32(rng.standard_normal((M, N)))
    r = GR.gemm(A, B, -0.75, bias, 0.5, C0, act, aux)
    pre = np.einsum('mk,kn->mn', A, B) * -0.75 + bias + 0.5 * C0
    want = {GR.ACT_NONE: pre, GR.ACT_RELU: np.where(pre > 0, pre, 0.0), GR.ACT_SIGMOID: O.sigmoid(pre),
            GR.ACT_MASKPOS: pre * (aux > 0)}[act]
    np.testing.assert_allclose(r['out'], want, rtol=1e-12, atol=1e-12)
    mag = 0.75 * np.einsum('mk,kn->mn', np.abs(A), np.abs(B)) + np.abs(bias) + 0.5 * np.abs(C0)
    if act in (GR.ACT_NONE, GR.ACT_RELU):
        np.testing.assert_allclose(r['bound'], GR.BOUND_K * GR.U * mag, rtol=1e-12)
    assert (r['bound'] >= 0).all()


def test_grouped_reference_is_the_contract():
    rng = np.random.default_rng(5)
    K, N, T = 12, 6, 4
    X = f32(rng.standard_normal((K, 3)))
    H = f32(rng.standard_normal((K, 5)))
    D = f32(rng.standard_normal((K, 2)))
    B = f32(rng.standard_normal((K, N)))
    C0 = [f32(rng.standard_normal((m, N))) for m in (3, 5, 1, 3)]
    probs = [dict(A=X, M=3), dict(A=H, M=5, shift=1, zero_period=T), dict(M=1, ones=1), dict(A=D, M=3, ones=2)]
    for p, c in zip(probs, C0):
        p['C0'] = c
    res = GR.grouped(probs, B, beta=0.5)
    Hs = np.zeros_like(H)
    for k in range(K):                               # h_{t-1}: shifted by one step, zero at every window start
        if k % T:
            Hs[k] = H[k - 1]
    want = [X.T @ B, Hs.T @ B, B.sum(0, keepdims=True), np.concatenate([D.T @ B, B.sum(0, keepdims=True)])]
    for r, w, c in zip(res, want, C0):
        np.testing.assert_allclose(r['out'], w + 0.5 * c, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        GR.grouped_operand(H, K, 5, shift=1)          # row -1 outside the zero-period rows


def test_bce_reference_is_the_oracle():
    rng = np.random.default_rng(7)
    M, N, K = 6, 40, 9
    for scale_ab, clipped in ((0.9, False), (3.0, True)):
        A, B = f32(rng.standard_normal((M, K)) * scale_ab), f32(rng.standard_normal((K, N)) * scale_ab)
        bias = f32(rng.standard_normal(N))
        Y = (rng.random((M, N)) < 0.3).astype(np.float64)
        r = GR.bce(A, B, bias, Y, 0.25)
        a = A @ B + bias
        out = (a > GR.CLIP_HI) | (a < GR.CLIP_LO)
        assert out.any() == clipped and (not clipped or ((a > 16.2).any() and (a < -16.2).any()))
        assert (np.minimum(np.abs(a - GR.CLIP_HI), np.abs(a - GR.CLIP_LO)) > 1e-3).all()      # none near a clip point
        loss, g = O.bce_from_logits_keras(a, Y)
        np.testing.assert_allclose(r['logits'], a, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(r['dlogits'], 0.25 * g, rtol=1e-12, atol=1e-12)
        # a clipped element's loss moves by the difference of the fp32 and fp64 clip points (< 1e-6) times |1 - y|
        tol = (out * 1e-6 * 2).sum(1) + 1e-12 * np.abs(loss)
        assert (np.abs(r['rownll'] - loss) <= tol).all()
        assert not r['clip_edge'].any()
    # the clip points are the fp32 constants of the kernels (csrc/common.h), the oracle's float32-Keras points rounded
    assert np.float32(GR.CLIP_HI) == np.float32(15.94238503) and np.float32(GR.CLIP_LO) == np.float32(-16.11809555)


# ---- an fp32 evaluation of the contract stays within the bounds ----
def test_fp32_evaluation_within_bounds():
    rng = np.random.default_rng(9)
    worst = {}
    for act in range(4):
        for (M, N, K) in [(33, 17, 5), (64, 96, 700), (5, 176, 4099)]:
            A32 = rng.standard_normal((M, K)).astype(np.float32)
            B32 = rng.standard_normal((K, N)).astype(np.float32)
            b32 = rng.standard_normal(N).astype(np.float32)
            C32 = rng.standard_normal((M, N)).astype(np.float32)
            aux = rng.standard_normal((M, N))
            r = GR.gemm(A32, B32, 0.75, b32, 0.5, C32, act, aux)
            v = np.float32(0.75) * (A32 @ B32) + b32 + np.float32(0.5) * C32
            v = {0: v, 1: np.maximum(v, np.float32(0)), 2: (1 / (1 + np.exp(-v.astype(np.float64)))).astype(np.float32),
                 3: np.where(aux > 0, v, np.float32(0))}[act]
            worst[act] = max(worst.get(act, 0.0), GR.within(v, r['out'], r['bound'], "act %d" % act))
    K, N = 3000, 88
    B32 = rng.standard_normal((K, N)).astype(np.float32)
    H32 = rng.standard_normal((K, 40)).astype(np.float32)
    g = GR.grouped([dict(A=H32, M=40, shift=1, zero_period=30)], B32)[0]
    Hs = np.zeros_like(H32)
    Hs[1:] = H32[:-1]
    Hs[np.arange(K) % 30 == 0] = 0
    worst['grouped'] = GR.within(Hs.T @ B32, g['out'], g['bound'], "grouped")
    A32 = (rng.standard_normal((50, 88)) * 2).astype(np.float32)
    W32 = (rng.standard_normal((88, 96)) * 0.5).astype(np.float32)
    bo = rng.standard_normal(96).astype(np.float32)
    Y = (rng.random((50, 96)) < 0.1).astype(np.float32)
    r = GR.bce(A32, W32, bo, Y, 0.5)
    a = A32 @ W32 + bo
    l = np.clip(a, np.float32(GR.CLIP_LO), np.float32(GR.CLIP_HI))
    e = np.exp(-np.abs(l))
    nll = (np.maximum(l, 0) + np.log(np.float32(1) + e) - l * Y).sum(1, dtype=np.float32)
    sg = np.where(l >= 0, 1 / (1 + e), e / (1 + e)).astype(np.float32)
    dl = np.where((a >= GR.CLIP_LO) & (a <= GR.CLIP_HI), np.float32(0.5) * (sg - Y), 0)
    worst['bce logits'] = GR.within(a, r['logits'], r['b_logits'], "logits")
    worst['bce rownll'] = GR.within(nll, r['rownll'], r['b_rownll'], "rownll")
    worst['bce dlogits'] = GR.within(dl, r['dlogits'], r['b_dlogits'], "dlogits", r['dl_alt'], r['clip_edge'])
    print("\nfp32 numpy evaluation, worst error / bound: %s" % ", ".join("%s %.3g" % kv for kv in worst.items()))
    assert max(worst.values()) < 0.5


# ---- planted faults are rejected ----
def _rejected(got, r, what):
    """a faulted result must fail the comparison the GPU test makes: bit for bit on the integer cases, else the bound"""
    with pytest.raises(AssertionError):
        GR.exact(got, r['out'], what)
    with pytest.raises(AssertionError):
        GR.exact(np.where(np.isnan(got), np.inf, got), r['out'], what)


@pytest.mark.parametrize("K", [37, 32768])
def test_int_case_rejects_a_dropped_k_term(K):
    rng = np.random.default_rng(K)
    M, N = 3, 4
    A, B = GR.int_operands(rng, M, K), GR.int_operands(rng, K, N)
    bias, C0 = GR.int_operands(rng, N), GR.int_operands(rng, M, N)
    r = GR.gemm(A, B, GR.INT_ALPHA, bias, GR.INT_BETA, C0)
    # any order of fp32 additions is exact on these operands: a shuffled fp32 sum matches bit for bit
    perm = rng.permutation(K)
    acc = np.zeros((M, N), np.float32)
    for s in np.array_split(perm, 7):
        acc += (A[:, s].astype(np.float32) @ B[s].astype(np.float32))
    ok = np.float32(GR.INT_ALPHA) * acc + bias.astype(np.float32) + np.float32(GR.INT_BETA) * C0.astype(np.float32)
    GR.exact(ok, r['out'], "shuffled")
    k = int(np.argmax(np.abs(A[1] * B[:, 2])))      # a nonzero product
    bad = ok.astype(np.float64).copy()
    bad[1, 2] -= GR.INT_ALPHA * A[1, k] * B[k, 2]
    _rejected(bad, r, "dropped k term")


def _grouped_int(rng, K=64, N=20, T=7):
    H = GR.int_operands(rng, K, 9)
    B = GR.int_operands(rng, K, N)
    return H, B, T


def test_int_case_rejects_shift_and_zero_period_faults():
    rng = np.random.default_rng(3)
    H, B, T = _grouped_int(rng)
    K = B.shape[0]
    r = GR.grouped([dict(A=H, M=9, shift=1, zero_period=T)], B)[0]
    GR.exact(GR.grouped_operand(H, K, 9, 1, T).T @ B, r['out'])
    off_k = np.zeros((K, 9))                        # k off by one: row k - 2 instead of k - 1
    for k in range(K):
        if k % T and k >= 2:
            off_k[k] = H[k - 2]
    _rejected(off_k.T @ B, r, "k off by one")
    phase = np.zeros((K, 9))                        # zero rows at k % T == 1 instead of 0
    for k in range(1, K):
        if k % T != 1:
            phase[k] = H[k - 1]
    _rejected(phase.T @ B, r, "zero-period phase")


def test_int_case_rejects_tile_faults():
    rng = np.random.default_rng(4)
    M, N, K, BN = 20, 40, 30, 16                    # last column tile: columns 32..39
    A, B = GR.int_operands(rng, M, K), GR.int_operands(rng, K, N)
    bias, C0 = GR.int_operands(rng, N), GR.int_operands(rng, M, N)
    bias[-8:] = np.where(bias[-8:] == 0, 1.0, bias[-8:])
    r = GR.gemm(A, B, GR.INT_ALPHA, bias, GR.INT_BETA, C0)
    twice = r['out'].copy()
    twice[:, (N // BN) * BN:] += bias[(N // BN) * BN:]
    _rejected(twice, r, "bias twice on the last column tile")
    sw = r['out'].copy()
    c = next(j for j in range(BN - 1) if (sw[:, j] != sw[:, j + 1]).any())
    sw[:, [c, c + 1]] = sw[:, [c + 1, c]]
    _rejected(sw, r, "two columns of a tile swapped")
    _rejected(GR.gemm(A, B, GR.INT_ALPHA ** 2, bias, GR.INT_BETA, C0)['out'], r, "alpha applied twice")
    # beta = 0: C is never read -- reading it (NaN-filled in the GPU tests) poisons the output
    r0 = GR.gemm(A, B, GR.INT_ALPHA, bias, 0.0, None)
    with np.errstate(invalid='ignore'):
        _rejected(r0['out'] + 0.0 * np.full((M, N), np.nan), r0, "beta C added at beta = 0")


def test_int_case_rejects_a_missing_ones_row():
    rng = np.random.default_rng(6)
    K, N = 50, 24
    D, B = GR.int_operands(rng, K, 5), GR.int_operands(rng, K, N)
    r = GR.grouped([dict(A=D, M=6, ones=2)], B)[0]
    miss = r['out'].copy()
    miss[5] = 0.0
    _rejected(miss, r, "ones row missing")
    miss[5] = B[1:].sum(0)                          # one k of the column sums lost
    _rejected(miss, r, "ones row short by a term")


def test_bound_rejects_faults_on_float_data():
    rng = np.random.default_rng(8)
    M, N, K = 40, 48, 200
    A, B = f32(rng.standard_normal((M, K))), f32(rng.standard_normal((K, N)))
    bias = f32(rng.standard_normal(N))
    r = GR.gemm(A, B, 0.75, bias, 0.0, None, GR.ACT_SIGMOID)
    with pytest.raises(AssertionError):
        GR.within(GR.gemm(A, B, 0.75 ** 2, bias, 0.0, None, GR.ACT_SIGMOID)['out'], r['out'], r['bound'])
    sw = r['out'].copy()
    sw[:, [3, 4]] = sw[:, [4, 3]]
    with pytest.raises(AssertionError):
        GR.within(sw, r['out'], r['bound'])
    k = int(np.argmax(np.abs(A[2] * B[:, 7])))
    bad = GR.gemm(A, B, 0.75, bias)['out']
    bad[2, 7] -= 0.75 * A[2, k] * B[k, 7]           # the largest product of one output dropped
    rn = GR.gemm(A, B, 0.75, bias)
    with pytest.raises(AssertionError):
        GR.within(bad, rn['out'], rn['bound'])


def test_bce_bound_rejects_faults_and_accepts_clip_edges():
    Y = np.array([[0.0, 1.0, 0.0, 1.0, 0.0]])
    a_pts = np.array([[GR.CLIP_HI, GR.CLIP_LO, 3.0, -2.0, 16.5]])
    A = np.eye(1)
    r = GR.bce(A, a_pts, np.zeros(5), Y, 1.0)
    assert r['clip_edge'][0, :2].all() and not r['clip_edge'][0, 2:].any()
    # on a clip edge either side is accepted
    GR.within(r['dl_alt'] * r['clip_edge'] + r['dlogits'] * ~r['clip_edge'], r['dlogits'], r['b_dlogits'], "edge",
              r['dl_alt'], r['clip_edge'])
    with pytest.raises(AssertionError):             # not elsewhere: 16.5 is clipped, its gradient is 0
        GR.within(r['dl_alt'], r['dlogits'], r['b_dlogits'], "no edge", r['dl_alt'], r['clip_edge'] & False)
    with pytest.raises(AssertionError):             # the NLL of an element with the wrong target
        nll = r['rownll'] - r['logits'][0, 2]
        GR.within(nll, r['rownll'], r['b_rownll'])


# ---- the exact fp32 fma chain ----
def _fp32_round(x):
    """round a Fraction to fp32, nearest even (normal range)"""
    if x == 0:
        return 0.0
    s = -1 if x < 0 else 1
    x = abs(x)
    e = int(np.floor(np.log2(float(x))))
    while Fraction(2) ** e > x:
        e -= 1
    while Fraction(2) ** (e + 1) <= x:
        e += 1
    ulp = Fraction(2) ** (e - 23)
    q = x / ulp
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return s * float(n * ulp)


def _fma_exact(a, b, c):
    return _fp32_round(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def test_fmaf_emulation_matches_exact_rational_rounding():
    rng = np.random.default_rng(12)
    n = 3000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(np.float32)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)).astype(np.float32)
    c[:500] = (-(a[:500].astype(np.float64) * b[:500]) * (1 + 2.0 ** -20 * rng.standard_normal(500))).astype(np.float32)
    got = GR.fmaf(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], np.float32)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    # the naive fp64 evaluation rounded to fp32 (two roundings) is not an fma: the samples must include such cases or the
    # comparison above would prove little -- the constructed midpoints below do
    e = 2.0 ** -23
    cases = [  # a, b, c, fma, what two roundings give
        (1 + e, (1 - e) * 2.0 ** -24, 1 + e, 1 + e, 1 + 2 * e),      # just below the midpoint: down (two roundings: even, up)
        (-(1 + e), (1 - e) * 2.0 ** -24, 1 + e, 1 + e, 1.0),          # just above the midpoint: up
        (1.0, 2.0 ** -24, 1 + e, 1 + 2 * e, 1 + 2 * e),               # a true tie: to even
        (1.0, 2.0 ** -24, 1.0, 1.0, 1.0),
    ]
    for sc in (1.0, 2.0 ** -30, 2.0 ** 40):
        for x, y, z, f, naive in cases:
            x, y, z = np.float32(x), np.float32(y * sc), np.float32(z * sc)
            assert float(GR.fmaf(x, y, z)) == f * sc == _fma_exact(x, y, z)
            assert float(np.float32(float(x) * float(y) + float(z))) == naive * sc
            assert float(GR.fmaf(-x, -y, z)) == f * sc
            assert float(GR.fmaf(x, -y, -z)) == -f * sc


def test_fma_chain_is_a_k_ordered_chain():
    rng = np.random.default_rng(13)
    A = rng.standard_normal((3, 21)).astype(np.float32)
    B = rng.standard_normal((21, 4)).astype(np.float32)
    got = GR.fma_chain(A, B)
    for i in range(3):
        for j in range(4):
            acc = 0.0
            for k in range(21):
                acc = _fma_exact(A[i, k], B[k, j], acc)
            assert got[i, j] == np.float32(acc)
    # a different order (or a separate multiply and add) gives different bits somewhere on a longer chain
    A = rng.standard_normal((16, 300)).astype(np.float32)
    B = rng.standard_normal((300, 16)).astype(np.float32)
    ref = GR.fma_chain(A, B)
    rev = GR.fma_chain(A[:, ::-1], B[::-1])
    sep = np.zeros((16, 16), np.float32)
    for k in range(300):
        sep = sep + A[:, k:k + 1] * B[k:k + 1]
    assert (ref != rev).any() and (ref != sep).any()
