"""-m gpu: the fp32 GEMM family (csrc/gemm.hip) called through the ops wrappers, every output against the fp64 reference of
tests/gemm_reference.py: integer-valued cases bit for bit, fma-chain cases bit for bit against the exact fp32 emulation, the
rest per element within its own rounding bound.  Outputs are NaN inside with canaries behind them and in their ldc > N padding
columns; operand padding columns are NaN.

  a  clv_gemm_f32, all 28 tile x transpose instances (pick_tile: 128x16, 64x32, 64x64, 32x96, 96x96, 64x96, 64x176) at M, N
     and K one below, at and one above the tile's multiple, K < 16, K % 4 != 0 and K = 0
  b  split-K: 1, auto, a split without the XCD remap (% 8 != 0) and one with it; bias / beta / sigmoid / maskpos in the
     reduction; its float4 and scalar forms; every split case deferred to a ReduceQueue, bit for bit the immediate one
  c  operand layouts: ld > K with NaN padding, bases 1 .. 3 floats off with ld % 4 == 0, a column block whose last row ends
     the allocation
  d  clv_gemm_grouped_tn: 1 .. 4 ragged problems, the 128x16 / 64x32 / 128x96 / 96x96 tiles, the in-workgroup split-K with
     two tiles in flight and without, shift 1 with zero periods < 16 and not dividing the k-chunk, ones 1 and 2, beta = 1,
     the skinny VALU kernel at and just past its limits; clv_gemm_grouped_tn_small2
  e  clv_gemm_bce_f32 at N 1 .. 176 with ldc != N and ldy != N, each output left out in turn, logits across both clip points
  f  determinism, one flush of several jobs (unsplit ones among them), the host-side argument checks
The worst error / bound ratio of every path and the number of flagged elements are printed at the end (run with -s)."""
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import gemm_reference as GR
from helpers import CANARY, TAIL

pytestmark = pytest.mark.gpu

_REPORT = dict(ratios={}, flagged={}, fma_bitwise=0, exact=0)


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    yield torch.device("cuda:0")
    r = _REPORT
    print("\ngemm: worst error / bound per path: %s" % ", ".join("%s %.3g" % kv for kv in sorted(r['ratios'].items())))
    print("gemm: flagged elements: %s" % (", ".join("%s %d" % kv for kv in sorted(r['flagged'].items())) or "none"))
    print("gemm: %d outputs bit for bit against the fp32 fma chain, %d integer-valued outputs bit for bit"
          % (r['fma_bitwise'], r['exact']))


@pytest.fixture(scope="module")
def ops_ws(dev):
    from clvae_amd import ops
    return ops, ops.Workspace(dev)


def _note(path, ratio, flagged=0):
    R = _REPORT
    R['ratios'][path] = max(R['ratios'].get(path, 0.0), ratio)
    R['flagged'][path] = R['flagged'].get(path, 0) + int(flagged)



def place(dev, X, ld, off=0, fill=float('nan')):
    """X [rows, cols] at float offset `off` of its own allocation, row stride ld, padding columns `fill`; the allocation
    ends with the last row (so a column block with off + cols == ld ends it exactly)"""
    X = np.asarray(X, np.float64)
    rows, cols = X.shape
    rows_a = max(rows, 1)
    flat = torch.full((rows_a * ld,), fill, dtype=torch.float32, device=dev)
    if rows and cols:
        flat.view(rows_a, ld)[:rows, off:off + cols] = torch.as_tensor(X.astype(np.float32), device=dev)
    return flat[off:]


class Out:
    """an output [M, ldc] at float offset off: NaN (or C0) in its N columns, canaries before, behind and in the padding"""

    def __init__(self, dev, M, N, ldc, off=0, C0=None):
        self.M, self.N, self.ldc, self.off = M, N, ldc, off
        self.flat = torch.full((off + M * ldc + TAIL,), CANARY, dtype=torch.float32, device=dev)
        v = self.flat[off:off + M * ldc].view(M, ldc)
        v[:, :N] = float('nan') if C0 is None else torch.as_tensor(np.asarray(C0, np.float32), device=dev)
        self.t = self.flat[off:]

    def get(self):
        f = self.flat.cpu().numpy()
        o, M, N, ldc = self.off, self.M, self.N, self.ldc
        assert (f[:o] == CANARY).all(), "write before the output"
        assert (f[o + M * ldc:] == CANARY).all(), "write behind the output"
        v = f[o:o + M * ldc].reshape(M, ldc)
        assert (v[:, N:] == CANARY).all(), "padding column written"
        return v[:, :N].astype(np.float64)


def _operands(rng, mode, *shape):
    if mode == 'int':
        return GR.int_operands(rng, *shape)
    return rng.standard_normal(shape).astype(np.float32).astype(np.float64)


def judge(path, got, r, mode, act=GR.ACT_NONE, opA=None, opB=None):
    """integer cases (acts none / relu / maskpos) bit for bit; fma mode bit for bit against the emulated chain; else the
    per-element bound"""
    if mode == 'fma':
        want = GR.fma_chain(opA, opB).astype(np.float64)
        GR.exact(got, want, path + " (fp32 fma chain)")
        _REPORT['fma_bitwise'] += got.size
        mode = 'float'
    if mode == 'int' and act != GR.ACT_SIGMOID:
        GR.exact(got, r['out'], path)
        _REPORT['exact'] += got.size
        return
    _note(path, GR.within(got, r['out'], r['bound'], path), r['relu_edge'].sum())


def gemm_case(dev, ops_ws, rng, M, N, K, ta=0, tb=0, mode='int', act=GR.ACT_NONE, bias=False, beta=0.0, split=None,
              lda=None, ldb=None, ldc=None, offA=0, offB=0, offC=0, defer_check=True, path=None):
    """one clv_gemm_f32 call against the reference; a split product also deferred to a ReduceQueue (bit for bit)"""
    ops, ws = ops_ws
    path = path or "gemm %s%s" % ('T' if ta else 'N', 'T' if tb else 'N')
    if mode == 'fma':
        alpha, bias, beta, act = 1.0, False, 0.0, GR.ACT_NONE
    else:
        alpha = GR.INT_ALPHA if mode == 'int' else 0.75
        beta = GR.INT_BETA if (mode == 'int' and beta) else beta
    opA, opB = _operands(rng, mode, M, K), _operands(rng, mode, K, N)
    b = _operands(rng, mode, N) if bias else None
    C0 = _operands(rng, mode, M, N) if beta else None
    aux = _operands(rng, 'int', M, N) if act == GR.ACT_MASKPOS else None
    physA, physB = (opA.T if ta else opA), (opB.T if tb else opB)
    lda = lda or max(physA.shape[1], 1)
    ldb = ldb or max(physB.shape[1], 1)
    ldc = ldc or N
    A = place(dev, physA, lda, offA)
    B = place(dev, physB, ldb, offB)
    bt = None if b is None else torch.as_tensor(b.astype(np.float32), device=dev)
    auxt = None if aux is None else place(dev, aux, ldc)
    r = GR.gemm(opA, opB, alpha, b, beta, C0, act, aux)
    if split is None:
        split = ops._lib.lib().clv_gemm_auto_split(M, N, K)
    kw = dict(ta=bool(ta), tb=bool(tb), lda=lda, ldb=ldb, ldc=ldc, alpha=alpha, beta=beta, bias=bt, act=act, aux=auxt,
              split_k=split)
    out = Out(dev, M, N, ldc, offC, C0)
    ops.gemm(A, B, out.t, M, N, K, ws=ws, **kw)
    torch.cuda.synchronize()
    got = out.get()
    judge(path, got, r, mode, act, opA, opB)
    if split > 1 and defer_check:
        q = ops.ReduceQueue(dev)
        out2 = Out(dev, M, N, ldc, offC, C0)
        ops.gemm(A, B, out2.t, M, N, K, defer=q, **kw)
        q.flush()
        torch.cuda.synchronize()
        GR.exact(out2.get(), got, path + " deferred")
    return got


# ---------------------------------------------------------------- a: tiles --
# (tile, [(M, N, K), ...]): pick_tile's choice at one below / at / one above the tile's multiples
TILE_SHAPES = [
    ("128x16", [(127, 16, 3), (128, 15, 17), (129, 16, 0), (257, 1, 13)]),
    ("64x32", [(63, 32, 16), (64, 31, 33), (65, 17, 47)]),
    ("64x64", [(63, 64, 15), (64, 33, 64), (65, 63, 65), (130, 129, 31)]),
    ("32x96", [(8192, 96, 17), (8193, 95, 31), (8223, 65, 0)]),
    ("96x96", [(95, 96, 13), (96, 95, 48), (96, 176, 33), (50, 257, 7)]),
    ("64x96", [(127, 96, 15), (128, 65, 16), (129, 95, 49)]),
    ("64x176", [(128, 176, 13), (129, 352, 16), (97, 257, 33)]),
]


@pytest.mark.parametrize("tile,shapes", TILE_SHAPES, ids=[t for t, _ in TILE_SHAPES])
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_gemm_tile_instances(dev, ops_ws, tile, shapes, ta, tb):
    """every tile x transpose instance: integer operands with alpha, bias, beta and relu / maskpos (bit for bit), then float
    operands as a bare product (bit for bit against the fp32 fma chain).  The k-contiguous operand has ld > K with NaN in
    the padding whenever K % 4 != 0 (the fast path's float4 reaches into it)."""
    rng = np.random.default_rng(zlib.crc32(('%s %d %d' % (tile, ta, tb)).encode()))
    for i, (M, N, K) in enumerate(shapes):
        pad = lambda n: ((n + 3) // 4 * 4 + 4 * (i % 2)) if n % 4 else None       # ld % 4 == 0 past the row's end
        lda = pad(M) if ta else pad(K)
        ldb = pad(K) if tb else pad(N)
        act = (GR.ACT_RELU, GR.ACT_MASKPOS, GR.ACT_NONE)[i % 3]
        path = "gemm %s %s%s" % (tile, 'T' if ta else 'N', 'T' if tb else 'N')
        gemm_case(dev, ops_ws, rng, M, N, K, ta, tb, 'int', act, bias=True, beta=0.5, split=1, lda=lda, ldb=ldb,
                  ldc=N + (i % 2) * 3, path=path)
        if K:
            gemm_case(dev, ops_ws, rng, M, N, K, ta, tb, 'fma', split=1, lda=lda, ldb=ldb, path=path)


@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1)])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 6, 7, 13, 18, 35, 90])
def test_gemm_k_tail_ignores_nan_padding(dev, ops_ws, K, ta, tb):
    """the fast path's last float4 of a k-contiguous row covers the padding columns K .. ld-1 when K % 4 != 0: NaN there
    must not reach a stored output (the mask has to clear the bits, not multiply by 0)"""
    rng = np.random.default_rng(K)
    ld = (K + 3) // 4 * 4 + 4
    for M, N in [(70, 16), (40, 88), (100, 176)]:
        gemm_case(dev, ops_ws, rng, M, N, K, ta, tb, 'int', GR.ACT_NONE, bias=True, split=1,
                  lda=None if ta else ld, ldb=ld if tb else None, path="gemm k tail")
        gemm_case(dev, ops_ws, rng, M, N, K, ta, tb, 'float', GR.ACT_SIGMOID, bias=True, split=1,
                  lda=None if ta else ld, ldb=ld if tb else None, path="gemm k tail")


# ---------------------------------------------------------------- b: split-K --
SPLIT_CASES = [
    # M, N, K, ta, tb, split, act, bias, beta, ldc, offC
    (100, 88, 2000, 0, 0, None, GR.ACT_RELU, True, 0.5, None, 0),      # auto split (31: no remap), float4 reduction
    (100, 88, 2000, 0, 0, 8, GR.ACT_MASKPOS, True, 0.5, None, 0),      # % 8 == 0: XCD remap
    (88, 352, 1999, 1, 0, 5, GR.ACT_NONE, False, 0.5, None, 0),
    (88, 352, 3000, 1, 0, 16, GR.ACT_SIGMOID, True, 0.0, None, 0),
    (45, 70, 777, 1, 1, 7, GR.ACT_MASKPOS, True, 0.5, 73, 0),          # N % 4 != 0: scalar reduction
    (60, 64, 1024, 0, 1, 8, GR.ACT_RELU, True, 0.5, 64, 1),            # unaligned C: scalar reduction
    (60, 64, 1024, 0, 0, 3, GR.ACT_NONE, True, 0.5, 66, 0),            # ldc % 4 != 0: scalar reduction
    (2, 352, 600, 1, 0, 4, GR.ACT_NONE, False, 0.0, None, 0),
    (256, 88, 1408, 0, 0, 11, GR.ACT_SIGMOID, True, 0.0, 96, 0),
]


@pytest.mark.parametrize("M,N,K,ta,tb,split,act,bias,beta,ldc,offC", SPLIT_CASES)
def test_gemm_split_k(dev, ops_ws, M, N, K, ta, tb, split, act, bias, beta, ldc, offC):
    """the epilogue runs in the reduction: bias, beta, sigmoid and maskpos there; deferred == immediate bit for bit"""
    rng = np.random.default_rng(M * 7 + N + K)
    for mode in ('int', 'float'):
        gemm_case(dev, ops_ws, rng, M, N, K, ta, tb, mode, act, bias, beta, split, ldc=ldc, offC=offC,
                  path="gemm split-K")
    if split is None:
        assert ops_ws[0]._lib.lib().clv_gemm_auto_split(M, N, K) > 1


# ---------------------------------------------------------------- c: layouts --
def test_gemm_operand_layouts(dev, ops_ws):
    rng = np.random.default_rng(21)
    # bases 1 .. 3 floats off with ld % 4 == 0: the scalar load path
    for off in (1, 2, 3):
        for ta, tb in [(0, 0), (1, 1), (0, 1)]:
            lda, ldb = (72 if ta else 48), (48 if tb else 96)
            gemm_case(dev, ops_ws, rng, 67, 90, 45, ta, tb, 'int', GR.ACT_RELU, True, 0.5, 1,
                      lda=lda, ldb=ldb, offA=off, offB=(off * 3) % 4, path="gemm layouts")
            gemm_case(dev, ops_ws, rng, 67, 90, 45, ta, tb, 'fma', split=1, lda=lda, ldb=ldb, offA=off, offB=off,
                      path="gemm layouts")
    # ld > K with NaN padding, split as well
    gemm_case(dev, ops_ws, rng, 130, 100, 301, 0, 1, 'int', GR.ACT_NONE, True, 0.5, 4, lda=308, ldb=312,
              path="gemm layouts")
    # a column block of a wider matrix whose last row ends the allocation (M = 4, K = 88, lda = 352, fourth block)
    ops, ws = ops_ws
    for M, K, N in [(4, 88, 88), (33, 88, 17)]:
        W = GR.int_operands(rng, M, 4 * K)
        Bm = GR.int_operands(rng, K, N)
        A = place(dev, W, 4 * K)[3 * K:]
        assert A.storage_offset() + (M - 1) * 4 * K + K == A.untyped_storage().nbytes() // 4
        out = Out(dev, M, N, N)
        ops.gemm(A, torch.as_tensor(Bm.astype(np.float32), device=dev), out.t, M, N, K, lda=4 * K, split_k=1, ws=ws)
        torch.cuda.synchronize()
        GR.exact(out.get(), W[:, 3 * K:] @ Bm, "column block")


# ---------------------------------------------------------------- d: grouped TN --
def grouped_case(dev, ops_ws, rng, N, K, probs, mode='int', beta=0.0, split=None, ldb=None, path="grouped",
                 defer_check=True, expect_kernel=None):
    """probs: list of dict(M, shift, zero_period, ones, lda, ldc); A_p [K, lda] with NaN padding"""
    ops, ws = ops_ws
    B = _operands(rng, mode, K, N)
    ldb = ldb or N
    Bt = place(dev, B, ldb)
    refp, dp = [], []
    for p in probs:
        M, ones = p['M'], p.get('ones', 0)
        ncol = M - 1 if ones == 2 else M
        A = _operands(rng, mode, K, ncol) if ones != 1 else None
        C0 = _operands(rng, mode, M, N) if beta else None
        ldc = p.get('ldc', N)
        lda = p.get('lda', (ncol + 3) // 4 * 4 if ones != 1 else 1)
        refp.append(dict(A=A, M=M, shift=p.get('shift', 0), zero_period=p.get('zero_period', 0), ones=ones, C0=C0))
        out = Out(dev, M, N, ldc, 0, C0)
        dp.append(dict(A=None if A is None else place(dev, A, lda, p.get('offA', 0)), lda=lda, M=M, C=out.t, ldc=ldc,
                       shift=p.get('shift', 0), zero_period=p.get('zero_period', 0), ones=ones, out=out))
    refs = GR.grouped(refp, B, beta)
    ops.gemm_grouped_tn(dp, N, K, Bt, ws, ldb=ldb, beta=beta, split_k=split)
    torch.cuda.synchronize()
    gots = [p['out'].get() for p in dp]
    for i, (g, r) in enumerate(zip(gots, refs)):
        judge(path, g, r, mode)
    if defer_check and split is not None and split > 1:
        q = ops.ReduceQueue(dev)
        for p, r in zip(dp, refp):
            p['out'] = Out(dev, p['M'], N, p['ldc'], 0, r['C0'])
            p['C'] = p['out'].t
        ops.gemm_grouped_tn(dp, N, K, Bt, None, ldb=ldb, beta=beta, split_k=split, defer=q)
        q.flush()
        torch.cuda.synchronize()
        for p, g in zip(dp, gots):
            GR.exact(p['out'].get(), g, path + " deferred")
    return gots


GROUPED_CASES = [
    # name, N, K, probs, split, beta
    ("128x16", 13, 300, [dict(M=40), dict(M=17, shift=1, zero_period=7), dict(M=1, ones=1), dict(M=9, ones=2)], 3, 0.0),
    ("64x32", 30, 257, [dict(M=70), dict(M=5, shift=1, zero_period=17)], 1, 1.0),
    ("128x96", 88, 500, [dict(M=120), dict(M=88, shift=1, zero_period=40)], 4, 0.0),     # 2 tiles of 128 < 3 of 96
    ("96x96", 100, 333, [dict(M=90, ldc=104), dict(M=33, shift=1, zero_period=10), dict(M=1, ones=1),
                         dict(M=89, ones=2)], 5, 1.0),
    ("96x96 beta", 352, 128, [dict(M=88), dict(M=88, shift=1, zero_period=16), dict(M=2)], 1, 1.0),
    # in-workgroup split-K (1024 threads, 4 k-groups): >= 16 splits, % 4 == 0, >= 256 workgroups after the division
    ("kg4 pf2", 352, 3072, [dict(M=88), dict(M=88, shift=1, zero_period=32), dict(M=88)], 96, 0.0),
    ("kg4 K % kc", 352, 3070, [dict(M=88), dict(M=88, shift=1, zero_period=40), dict(M=88)], 96, 1.0),
    ("kg4 zp < 16", 352, 3072, [dict(M=88), dict(M=88, shift=1, zero_period=7), dict(M=88)], 96, 0.0),
    ("kg4 ones", 352, 3072, [dict(M=88), dict(M=88), dict(M=88), dict(M=1, ones=1)], 96, 0.0),
    ("kg4 ones2", 352, 3072, [dict(M=89, ones=2), dict(M=88, shift=1, zero_period=24), dict(M=88)], 96, 0.0),
]


@pytest.mark.parametrize("name,N,K,probs,split,beta", GROUPED_CASES, ids=[c[0] for c in GROUPED_CASES])
def test_gemm_grouped_tn(dev, ops_ws, name, N, K, probs, split, beta):
    rng = np.random.default_rng(len(name) * 1000 + K)
    modes = ('int', 'float') if K < 3000 else ('int',)
    for mode in modes:
        grouped_case(dev, ops_ws, rng, N, K, probs, mode, beta, split, path="grouped " + name.split()[0])


def test_gemm_grouped_tn_auto_split_and_skinny(dev, ops_ws):
    """the skinny VALU kernel at 16 rows / K 4096, and just past either limit (the MFMA path); the auto split"""
    rng = np.random.default_rng(31)
    ops = ops_ws[0]
    for rows, K in [(16, 4096), (17, 4096), (16, 4097), (3, 50)]:
        probs = [dict(M=rows - 1, shift=1, zero_period=9), dict(M=1, ones=1)]
        arr = (ops._lib.GemmProb * 2)(*[ops._lib.GemmProb(None, 0, p['M'], None, 0, 0, 0, p.get('ones', 0))
                                        for p in probs])
        split = ops._lib.lib().clv_gemm_grouped_auto_split(arr, 2, 200, K)
        assert split == 1 or rows > 16 or K > 4096
        for mode in ('int', 'float'):
            grouped_case(dev, ops_ws, rng, 200, K, probs, mode, 0.0 if rows > 3 else 1.0, split,
                         path="grouped skinny" if rows <= 16 and K <= 4096 else "grouped auto")


def test_gemm_grouped_tn_small2(dev, ops_ws):
    """two few-row products with different B operands in one launch, ragged in N and K"""
    ops, _ = ops_ws
    rng = np.random.default_rng(41)
    N, K = 100, 333
    for mode in ('int', 'float'):
        sets, refs = [], []
        for q, pl in enumerate([[dict(M=3), dict(M=1, ones=1)], [dict(M=5, shift=1, zero_period=10), dict(M=10)]]):
            B = _operands(rng, mode, K, N)
            dp, rp = [], []
            for p in pl:
                M, ones = p['M'], p.get('ones', 0)
                A = _operands(rng, mode, K, M) if not ones else None
                lda = M + 3
                out = Out(dev, M, N, N + 2)
                rp.append(dict(A=A, M=M, shift=p.get('shift', 0), zero_period=p.get('zero_period', 0), ones=ones))
                dp.append(dict(A=None if A is None else place(dev, A, lda), lda=lda, M=M, C=out.t, ldc=N + 2,
                               shift=p.get('shift', 0), zero_period=p.get('zero_period', 0), ones=ones, out=out))
            sets.append((dp, place(dev, B, N)))
            refs.append(GR.grouped(rp, B))
        ops.gemm_grouped_tn_small2(sets[0][0], sets[0][1], sets[1][0], sets[1][1], N, K)
        torch.cuda.synchronize()
        for (dp, _), rr in zip(sets, refs):
            for p, r in zip(dp, rr):
                judge("grouped small2", p['out'].get(), r, mode)


def test_gemm_grouped_ones2_needs_aligned_a(dev, ops_ws):
    ops, ws = ops_ws
    from clvae_amd import _lib
    A = place(dev, np.ones((64, 8)), 12, 1)          # lda % 4 == 0, the base 4 bytes past a 16-byte boundary
    C = torch.empty(9, 40, device=dev)
    with pytest.raises(_lib.ClvError, match=r"\(-1\)"):
        ops.gemm_grouped_tn([dict(A=A, lda=12, M=9, C=C, ones=2)], 40, 64, torch.ones(64, 40, device=dev), ws)


# ---------------------------------------------------------------- e: gemm_bce --
@pytest.mark.parametrize("N", [1, 16, 17, 32, 33, 96, 97, 176])
def test_gemm_bce(dev, ops_ws, N):
    ops, _ = ops_ws
    rng = np.random.default_rng(N)
    M, K = 300, 45
    A = rng.standard_normal((M, K)).astype(np.float32).astype(np.float64)
    B = (rng.standard_normal((K, N)) * 1.6).astype(np.float32).astype(np.float64)
    A[0] = 0.0
    A[0, 0] = 1.0                                   # row 0: the logits are row 0 of B (exactly), across both clip points
    pts = np.array([GR.CLIP_HI, np.nextafter(np.float32(GR.CLIP_HI), np.float32(99)), -16.2, GR.CLIP_LO, 16.0, -16.0, 15.9, 0.0])
    B[0, :min(N, pts.size)] = pts[:N]
    bias = rng.standard_normal(N).astype(np.float32).astype(np.float64)
    bias[:min(N, pts.size)] = 0.0
    ldy, ldc, scale = N + 5, N + 3, 0.37
    Y = (rng.random((M, N)) < 0.3).astype(np.float64)
    r = GR.bce(A, B, bias, Y, scale)
    assert (r['logits'] > GR.CLIP_HI).any() and (r['logits'] < GR.CLIP_LO).any()
    At, Bt, bt, Yt = place(dev, A, K), place(dev, B, N), place(dev, bias[None], N)[:N], place(dev, Y, ldy)
    for omit in (None, 'logits', 'dlogits', 'rownll'):
        lg, dl = Out(dev, M, N, ldc), Out(dev, M, N, ldc)
        rn = Out(dev, M, 1, 1)
        t = lambda o, name: None if omit == name else o.t
        ops.gemm_bce(At, Bt, bt, Yt, scale, t(lg, 'logits'), t(dl, 'dlogits'), t(rn, 'rownll'), M, N, K, ldy=ldy, ldc=ldc)
        torch.cuda.synchronize()
        for name, o in (('logits', lg), ('dlogits', dl), ('rownll', rn)):
            got = o.get()
            if omit == name:
                assert np.isnan(got).all(), name + " written although NULL"
                continue
            if name == 'logits':
                _note("bce logits", GR.within(got, r['logits'], r['b_logits'], "logits"))
            elif name == 'rownll':
                _note("bce rownll", GR.within(got[:, 0], r['rownll'], r['b_rownll'], "rownll"))
            else:
                _note("bce dlogits", GR.within(got, r['dlogits'], r['b_dlogits'], "dlogits", r['dl_alt'], r['clip_edge']),
                      r['clip_edge'].sum())


# ---------------------------------------------------------------- f: determinism, deferral, checks --
def test_gemm_determinism_and_one_flush(dev, ops_ws):
    """two identical calls give identical bits; one flush of several jobs (an unsplit one among them, which the flush
    skips) gives the bits of each job reduced alone"""
    ops, ws = ops_ws
    rng = np.random.default_rng(51)
    jobs = [(100, 88, 2000, 0, 0, 8, GR.ACT_RELU), (45, 70, 777, 1, 1, 7, GR.ACT_SIGMOID),
            (64, 32, 16, 0, 0, 2, GR.ACT_NONE),          # split 2 of K = 16: one chunk, the job stays empty
            (88, 352, 1000, 1, 0, 5, GR.ACT_NONE)]
    args, alone = [], []
    for M, N, K, ta, tb, split, act in jobs:
        A = place(dev, rng.standard_normal((K, M) if ta else (M, K)), M if ta else K)
        B = place(dev, rng.standard_normal((N, K) if tb else (K, N)), K if tb else N)
        bias = torch.as_tensor(rng.standard_normal(N).astype(np.float32), device=dev)
        aux = None
        kw = dict(ta=bool(ta), tb=bool(tb), alpha=0.75, bias=bias, act=act, split_k=split)
        args.append((A, B, M, N, K, kw))
        res = []
        for _ in range(2):
            out = Out(dev, M, N, N)
            ops.gemm(A, B, out.t, M, N, K, ws=ws, aux=aux, **kw)
            torch.cuda.synchronize()
            res.append(out.get())
        GR.exact(res[1], res[0], "repeat")
        alone.append(res[0])
    probs = [dict(M=88), dict(M=88, shift=1, zero_period=40), dict(M=88)]
    Bg = place(dev, rng.standard_normal((3072, 352)), 352)
    Ag = [place(dev, rng.standard_normal((3072, 88)), 88) for _ in probs]
    def grouped(defer):
        outs = [Out(dev, 88, 352, 352) for _ in probs]
        dp = [dict(A=a, lda=88, M=88, C=o.t, shift=p.get('shift', 0), zero_period=p.get('zero_period', 0))
              for a, o, p in zip(Ag, outs, probs)]
        ops.gemm_grouped_tn(dp, 352, 3072, Bg, ws, split_k=96, defer=defer)
        return outs
    g1 = [o for o in grouped(None)]
    torch.cuda.synchronize()
    g1 = [o.get() for o in g1]
    g2 = [o.get() for o in grouped(None)]
    for a, b in zip(g1, g2):
        GR.exact(b, a, "grouped repeat")
    q = ops.ReduceQueue(dev)
    outs = []
    for A, B, M, N, K, kw in args:
        out = Out(dev, M, N, N)
        ops.gemm(A, B, out.t, M, N, K, defer=q, **kw)
        outs.append(out)
    gq = grouped(q)
    assert q.n == len(jobs) + 1
    q.flush()
    torch.cuda.synchronize()
    for o, a in zip(outs, alone):
        GR.exact(o.get(), a, "one flush")
    for o, a in zip(gq, g1):
        GR.exact(o.get(), a, "one flush (grouped)")


def test_gemm_host_checks(dev, ops_ws):
    """the documented CLV_EINVAL of the argument checks"""
    from clvae_amd import _lib
    ops, ws = ops_ws
    A, B, C = torch.ones(8, 8, device=dev), torch.ones(8, 8, device=dev), torch.zeros(8, 8, device=dev)
    for act, aux in [(4, None), (-1, None), (GR.ACT_MASKPOS, None)]:
        with pytest.raises(_lib.ClvError, match=r"\(-1\)"):
            ops.gemm(A, B, C, 8, 8, 8, act=act, aux=aux, split_k=1, ws=ws)
    p = lambda M: dict(A=torch.ones(64, 32, device=dev), lda=32, M=M, C=torch.zeros(32, 16, device=dev))
    Bs = torch.ones(5000, 16, device=dev)
    with pytest.raises(_lib.ClvError, match=r"\(-1\)"):           # more than 16 rows
        ops.gemm_grouped_tn_small2([p(10), p(7)], Bs, [p(2)], Bs, 16, 64)
    with pytest.raises(_lib.ClvError, match=r"\(-1\)"):           # K > 4096
        ops.gemm_grouped_tn_small2([p(2)], Bs, [p(2)], Bs, 16, 4097)
    torch.cuda.synchronize()
