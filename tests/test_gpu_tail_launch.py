"""-m gpu: the launch that ends the backward pass (csrc/tail_launch.hip, clv_splitk_reduce_multi_outer): the hW kernel
gradient's workgroups in front of the split-K reduction's, against the two launches it replaces.

Nothing here has a tolerance: the merged launch runs the product's own workgroup body (a row's sum does not depend on the
wave count; the extra workgroup keeps the batch-row order of the wave count the product's own launch takes) and the
reduction's additions in the reduction's order, so every output is BIT FOR BIT what clv_dense_outer_bf16 followed by
clv_splitk_reduce_multi leaves -- op by op (every role of the launch, slab counts on both sides of every loop bound of the
two reduce forms) and for captured training steps with the engine switch on and off.
"""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import clvae_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def F(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# slab counts on both sides of every loop bound of reduce_block (4 slab lanes, rounds of 32) and reduce_block_v4 (16 slab
# lanes, rounds of 128): 1 = not split at all (the product finishes itself, the job is skipped)
SLABS = (1, 15, 16, 17, 64, 113, 256)


def job_splits(rq, i):
    """the slab count inside the opaque job i (csrc/reduce_job.h: partial, M, N, splits)"""
    return int.from_bytes(bytes(rq.jobs[i].opaque[16:20]), 'little')


class Case:
    """Inputs of one launch: pending jobs of the wanted kind, five means, two rider products, the hW product."""

    def __init__(self, dev, B, Tn, kind, multi, with_jobs=True):
        rng = np.random.default_rng(1000 * B + Tn + (7 if multi else 0))
        self.dev, self.B, self.multi, self.with_jobs = dev, B, multi, with_jobs
        self.nx, self.N = Tn * 88, 88
        X = (rng.random((B, self.nx)) < 0.0443).astype(np.uint8)
        self.X = torch.as_tensor(X, device=dev) if kind == 'u8' else F(X, dev)
        self.G = F(rng.standard_normal((B, self.N)) * np.exp(rng.standard_normal((B, 1))), dev)
        self.H = F(np.maximum(rng.standard_normal((B, self.N)), 0), dev)
        self.hb = F(rng.standard_normal(self.N), dev)
        # the jobs' operands: K = 16 S gives exactly S slabs (chunks are multiples of 16)
        self.M, self.Nv, self.Ns = 24, 32, 30            # Nv: the float4 form; Ns (30 % 4 != 0): the scalar form
        Kmax = 16 * max(SLABS)
        self.A = F(rng.standard_normal((Kmax, 2 * self.M)) * np.exp(rng.standard_normal((Kmax, 1))), dev)
        self.Bv, self.Bs = F(rng.standard_normal((Kmax, self.Nv)), dev), F(rng.standard_normal((Kmax, self.Ns)), dev)
        self.bias = F(rng.standard_normal(self.Nv), dev)
        self.C0 = F(rng.standard_normal((2 * self.M + 1, self.Nv)), dev)
        # means: contiguous (float4 path and its ragged end), strided columns of a [B, 3] array
        self.m1, self.m2 = F(rng.standard_normal(B * Tn), dev), F(rng.standard_normal(4 * 1031 + 3), dev)
        self.m3 = F(rng.standard_normal((B, 3)), dev)
        # riders: the label rows + bias row of two LSTM input-kernel gradients
        self.Cn = 10
        self.W = F(rng.standard_normal((B, self.Cn)), dev)
        self.dz = [F(rng.standard_normal((B, 352)), dev) for _ in range(2)]

    def run(self, merged, via_entry_point=False):
        from clvae_amd import _lib, ops
        dev, M, B = self.dev, self.M, self.B
        z = lambda *sh: torch.full(sh, -7.0, dtype=torch.float32, device=dev)
        rq, ws, outs, want = ops.ReduceQueue(dev), ops.Workspace(dev), [], []
        if self.with_jobs:
            for S in SLABS:
                K = 16 * S
                if not self.multi:
                    # plain products as the steps use them: bias + relu on top of beta * C (float4 form), bare (scalar form)
                    c1, c2 = self.C0[:M].clone(), z(M, self.Ns)
                    ops.gemm(self.A, self.Bv, c1, M, self.Nv, K, ta=True, lda=2 * M, beta=0.5, bias=self.bias, act=ops.ACT_RELU,
                             split_k=S, ws=ws, defer=rq)
                    ops.gemm(self.A, self.Bs, c2, M, self.Ns, K, ta=True, lda=2 * M, alpha=0.25, split_k=S, ws=ws, defer=rq)
                    outs += [c1, c2]
                else:
                    # grouped products: two problems and an implicit row of ones (a Dense layer's kernel + bias), with beta
                    c1, c1b, c2, c2b = self.C0[:M].clone(), self.C0[M:2 * M + 1].clone(), z(M, self.Ns), z(1, self.Ns)
                    ops.gemm_grouped_tn([dict(A=self.A, lda=2 * M, M=M, C=c1), dict(A=self.A[:, M:], lda=2 * M, M=M + 1, C=c1b, ones=2)],
                                        self.Nv, K, self.Bv, ws, beta=1.0, split_k=S, defer=rq)
                    ops.gemm_grouped_tn([dict(A=self.A, lda=2 * M, M=M, C=c2), dict(A=None, M=1, C=c2b, ones=1)],
                                        self.Ns, K, self.Bs, ws, split_k=S, defer=rq)
                    outs += [c1, c1b, c2, c2b]
                want += [S, S] if S > 1 else []
            assert [job_splits(rq, i) for i in range(rq.n)] == want
        dK, cs, gd = z(self.nx, self.N), z(self.N), z(self.N)
        outer = dict(Bn=B, nx=self.nx, N=self.N, X=self.X, ldx=self.nx, G=self.G, ldg=self.N, out=dK, colsum=cs,
                     gdot=(self.H, self.N, self.hb, gd))
        means = [(self.m1, self.m1.numel(), 1), (self.m2, self.m2.numel(), 1), (self.m3, B, 3), (self.m3[:, 1:], B, 3),
                 (self.m3[:, 2:], B, 3)]
        scal = z(8)
        rows = [z(self.Cn, 352) for _ in range(2)]
        brow = [z(352) for _ in range(2)]
        skinny = [dict(A=self.W, lda=self.Cn, rows=self.Cn, B=self.dz[i], ldb=352, N=352, K=B, C=rows[i], ldc=352, bias_row=brow[i])
                  for i in range(2)]
        if not self.with_jobs:
            means, skinny = None, None
        if merged:
            assert ops.reduce_outer_supported(B, self.nx, self.N, self.nx, self.N)
            rq.flush(means=means, out=scal, skinny=skinny, outer=outer)
        else:
            ops.dense_outer_bf16(B, self.nx, self.N, self.X, self.nx, self.G, self.N, dK, colsum=cs, gdot=outer['gdot'])
            rq.flush(means=means, out=scal, skinny=skinny)
        torch.cuda.synchronize()
        return [dK, cs, gd, scal] + rows + brow + outs


SHAPES = [(256, 128), (1024, 256), (768, 5), (64, 16), (7, 3)]


@pytest.mark.parametrize("multi", [False, True], ids=["single", "grouped"])
@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("B,Tn", SHAPES)
def test_merged_launch_equals_the_two_launches(dev, B, Tn, kind, multi):
    """hW kernel gradient, colsum, gdot, every reduced job (single problem / grouped, float4 / scalar form, every slab count of
    SLABS, bias + relu + beta epilogues), the five means and both rider products: merged launch == two launches, bit for bit."""
    case = Case(dev, B, Tn, kind, multi)
    two, one = case.run(merged=False), case.run(merged=True)
    assert len(two) == len(one) and len(one) > 8
    for i, (a, b) in enumerate(zip(two, one)):
        assert not torch.any(a[:1] == -7.0) or i == 3, i          # written (the scalars' tail stays as filled)
        assert bits_equal(a, b), (i, float((a - b).abs().max()))
    assert torch.isfinite(one[0]).all() and float(one[0].abs().max()) > 0


@pytest.mark.parametrize("kind", ["f32", "u8"])
@pytest.mark.parametrize("B,Tn", SHAPES)
def test_product_alone_in_the_merged_launch(dev, B, Tn, kind):
    """zero pending jobs, no means, no riders: the launch is the product's workgroups only"""
    case = Case(dev, B, Tn, kind, False, with_jobs=False)
    two, one = case.run(merged=False), case.run(merged=True)
    for i in range(3):
        assert bits_equal(two[i], one[i]), i
    # float frames and byte frames promise the same bits: the merged launch keeps that promise too
    other = Case(dev, B, Tn, 'f32' if kind == 'u8' else 'u8', False, with_jobs=False).run(merged=True)
    for i in range(3):
        assert bits_equal(other[i], one[i]), i


@pytest.mark.parametrize("multi", [False, True], ids=["single", "grouped"])
def test_pending_jobs_without_a_product(dev, multi):
    """clv_splitk_reduce_multi_outer without a product: the reduce roles alone in their low-occupancy form == clv_splitk_reduce_multi"""
    from clvae_amd import _lib, ops
    case = Case(dev, 64, 16, 'f32', multi)
    two = case.run(merged=False)

    def flush_lo(self, means=None, out=None, skinny=None):
        k = len(means)
        xs = (C.c_void_p * k)(*[t.data_ptr() for t, _, _ in means])
        ns = (C.c_int * k)(*[int(n) for _, n, _ in means])
        st = (C.c_int * k)(*[int(s) for _, _, s in means])
        riders = (_lib.SkinnyProduct * len(skinny))()
        for i, p in enumerate(skinny):
            riders[i] = _lib.SkinnyProduct(p['A'].data_ptr(), p['lda'], p['rows'], p['B'].data_ptr(), p['ldb'], p['N'], p['K'],
                                           p['C'].data_ptr(), p['ldc'], p['bias_row'].data_ptr())
        _lib.check(_lib.lib().clv_splitk_reduce_multi_outer(self.jobs, self.n, xs, ns, st, k, out.data_ptr(), riders, len(skinny),
                                                            0, 0, 0, None, 0, 0, None, 0, None, 0, None, None, 0, None, None,
                                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        self.n = 0

    plain = ops.ReduceQueue.flush
    ops.ReduceQueue.flush = flush_lo
    try:
        one = case.run(merged=False)
    finally:
        ops.ReduceQueue.flush = plain
    for i, (a, b) in enumerate(zip(two, one)):
        assert bits_equal(a, b), i


def test_entry_point_rejects_what_the_product_rejects(dev):
    from clvae_amd import _lib, ops
    L = _lib.lib()
    assert not ops.reduce_outer_supported(16, 90, 88, 90, 88)          # nx % 4
    assert not ops.reduce_outer_supported(16, 96, 100, 96, 100)        # N > 96
    x = torch.zeros(16, 96, device=dev)
    g = torch.zeros(16, 88, device=dev)
    out = torch.zeros(96, 88, device=dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    # ldo < N; a product without its output; gdot without Hact
    assert L.clv_splitk_reduce_multi_outer(None, 0, None, None, None, 0, None, None, 0, 16, 96, 88, p(x), 0, 96, p(g), 88, p(out), 80,
                                           None, None, 0, None, None, s) != 0
    assert L.clv_splitk_reduce_multi_outer(None, 0, None, None, None, 0, None, None, 0, 16, 96, 88, p(x), 0, 96, p(g), 88, None, 88,
                                           None, None, 0, None, None, s) != 0
    assert L.clv_splitk_reduce_multi_outer(None, 0, None, None, None, 0, None, None, 0, 16, 96, 88, p(x), 0, 96, p(g), 88, p(out), 88,
                                           None, None, 0, None, p(g), s) != 0
    assert L.clv_splitk_reduce_multi_outer(None, 0, None, None, None, 0, None, None, 0, 0, 0, 0, None, 0, 0, None, 0, None, 0,
                                           None, None, 0, None, None, s) == 0
    torch.cuda.synchronize()


def _steps(dev, B, Tn, L, Cn, steps, bound):
    """`steps` captured TrainStep steps with CLV_TAIL_LAUNCH = 1 and = 0 from the same start; returns both runs' (losses,
    parameters + optimizer state) and how many reduce launches carried the product in each."""
    from clvae_amd import ops
    from clvae_amd.engine import VrnnEngine
    from clvae_amd.trainer import TrainStep
    cfg = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=Cn, use_x_prev=True)
    rng = np.random.default_rng(B + Tn)
    p0 = {k: np.asarray(v, np.float32) for k, v in O.vrnn_init_params(cfg, seed=8).items()}
    nb = 4
    n = nb * B
    win = rng.random((n, Tn + 1, 88)) < 0.0443
    u8 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint8), device=dev)
    cur, hist = u8(win[:, 1:].reshape(n, -1)), u8(win[:, :-1].reshape(n, -1))
    keys = torch.as_tensor(np.eye(Cn, dtype=np.float32)[rng.integers(0, Cn, n)], device=dev)
    idx = torch.as_tensor(rng.permutation(n).astype(np.int64), device=dev)
    plain = ops.ReduceQueue.flush
    runs = []
    for flag in ('1', '0'):
        carried = [0]

        def counting(self, *a, **kw):
            carried[0] += kw.get('outer') is not None
            return plain(self, *a, **kw)

        os.environ['CLV_TAIL_LAUNCH'] = flag
        ops.ReduceQueue.flush = counting
        try:
            eng = VrnnEngine(cfg, B, dev)
            assert eng.tail_launch == (flag == '1')
            eng.P.set_weights(p0)
            ts = TrainStep(eng, seed=21, use_graph=True)
            if bound:
                ts.bind_batches(cur, hist, keys, idx=idx, period=nb, stride=B)
            for it in range(steps):
                if not bound:
                    ts.gather_batch(cur, hist, keys, idx[(it % nb) * B:(it % nb + 1) * B])
                ts.step()
            torch.cuda.synchronize()
            assert eng.frames_exact_bf16
            state = [t.detach().cpu().numpy().copy() for t in eng.P.state_tensors()]
            runs.append((dict(eng.losses()), {k: v.copy() for k, v in eng.P.get_weights().items()}, state, carried[0]))
        finally:
            ops.ReduceQueue.flush = plain
            os.environ.pop('CLV_TAIL_LAUNCH', None)
    return runs


@pytest.mark.parametrize("bound", [False, True], ids=["gathered", "bound-cursor"])
@pytest.mark.parametrize("B,Tn,L", [(256, 128, 2), (64, 16, 32)])
def test_captured_steps_switch_on_equals_switch_off(dev, B, Tn, L, bound):
    """50 replayed steps of TrainStep with the merged launch against 50 with the two launches: losses, parameters and
    optimizer state bit for bit (an optimizer that amplifies a one-ulp difference over 50 steps), staged by a gather launch
    per step and through the bound-batch cursor."""
    on, off = _steps(dev, B, Tn, L, 10, 50, bound)
    assert on[3] >= 2 and off[3] == 0, (on[3], off[3])       # the eager first step and the capture carried the product
    assert all(np.isfinite(v) for v in on[0].values())
    assert on[0] == off[0], (on[0], off[0])
    for k in on[1]:
        np.testing.assert_array_equal(on[1][k], off[1][k], err_msg=k)
    assert len(on[2]) == len(off[2]) > 0
    for a, b in zip(on[2], off[2]):
        np.testing.assert_array_equal(a, b)


def test_data_parallel_schedule_keeps_the_two_launches(dev, monkeypatch):
    """With an all-reduce to start between the halves (here the forced one-GPU form) the product stays a launch of its own:
    the hW bucket must be complete before grads_tail()."""
    monkeypatch.setenv('CLV_FORCE_DP_GRAPHS', '1')
    on, off = _steps(dev, 64, 16, 2, 10, 3, True)
    assert on[3] == 0 and off[3] == 0
    for k in on[1]:
        np.testing.assert_array_equal(on[1][k], off[1][k], err_msg=k)
