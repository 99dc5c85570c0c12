"""-m gpu: the entry points of csrc/pointwise.hip (clv_gather_rows_multi: tests/test_gpu_gather.py) against the fp64 reference of
tests/pointwise_reference.py, over its case tables: EVERY output of every call, element by element, within its own bound
(bit for bit where the reference says so), flagged elements excepted.

Buffers: every output is a helpers.Bufs buffer -- NaN inside, a canary tail, the canary in the padding columns of strided
outputs -- and check_canaries() runs after every case; the padding columns of strided INPUTS, the elements that a
stride-3 term of sum_strided / loss_sums skips and the float in front of a misaligned term hold NaN, so a read of one shows.  clv_colsum_f32 gets exactly clv_colsum_workspace_bytes plus a canary tail.  The reductions (sum_strided, loss_sums,
colsum) are called twice on the same inputs: no atomics in the file, so the results must be bitwise equal.  A test goes
through all its cases and reports every failure, not the first.

Measured on an MI355X (the module's report, -s), worst error / bound per kernel and output (the honest fp32 evaluation of
tests/test_pointwise_reference.py stays below 0.5 everywhere):
  label_fwd      w 0.056, rowloss 0.076        label_bwd     dmean 0.13, dlogvar 0.27
  gauss_fwd      z 0.46, rowkl 0.053           gauss_bwd     dzargs 0.48
  bernoulli_nll  rownll 0.21, dlogits 0.58     sum_strided   0.027      loss_sums  0.025      colsum  0.10
  axpy           0.47                          act_grad      0.38       sigmoid_temper  0.75  lerp_rows  0.39
  dropout_rows   0.25 (beta 1; beta 0 exact)
  scale_temper, bernoulli_sample, bernoulli_sample_clamped, take_frame, gather_rows: bit for bit
The two derived budgets that the intrinsics spend most of: dlogits (v_exp_f32, v_rcp_f32) and sigmoid_temper (the same pair
at |x| up to 30, where the rounded exponent alone is 30 of the 38 units).  No kernel exceeded a bound; no defect was found.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import pointwise_reference as P
from helpers import CANARY, TAIL, Bufs

pytestmark = pytest.mark.gpu

_REPORT = {}
f32 = np.float32


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    yield torch.device("cuda:0")
    for k in sorted(_REPORT):
        print("\n%-26s worst error / bound: %s" % (k, ", ".join("%s %.3g" % kv for kv in sorted(_REPORT[k].items()))), end="")
    print()


def T(a, dev, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev).to(dtype).contiguous()


def padded(a, pad, dev):
    """a [rows, cols] on the device with `pad` columns of NaN behind every row; returns (the whole buffer, its ld)"""
    a = np.asarray(a, f32)
    full = np.full((a.shape[0], a.shape[1] + pad), np.nan, f32)
    full[:, :a.shape[1]] = a
    return T(full, dev), a.shape[1] + pad


def N(t):
    return t.detach().cpu().numpy()


class Cases:
    """runs a kernel's cases, collects the ratios and every failure"""

    def __init__(self, kernel):
        self.kernel, self.fails, self.n = kernel, [], 0

    def compare(self, case, got, ref, bufs=None, kernel=None):
        k = kernel or self.kernel
        self.n += 1
        rep = _REPORT.setdefault(k, {})
        for o in sorted(ref):
            try:
                v = P.check_all("%s %r" % (k, case), {o: got[o]}, {o: ref[o]})[o]
                rep[o] = max(rep.get(o, 0.0), v)
            except AssertionError as e:
                rep[o] = float('inf')
                self.fails.append(str(e))
        assert set(got) == set(ref)
        if bufs is not None:
            try:
                torch.cuda.synchronize()
                bufs.check_canaries()
            except AssertionError as e:
                self.fails.append("%s %r: %s" % (k, case, e))

    def same_bits(self, case, a, b):
        try:
            P.check_bits("%s %r, called twice" % (self.kernel, case), N(a), N(b))
        except AssertionError as e:
            self.fails.append(str(e))

    def done(self):
        assert self.n > 0
        assert not self.fails, "%d failures:\n%s" % (len(self.fails), "\n".join(self.fails[:40]))


def test_label_fwd_and_bwd(dev):
    from clvae_amd import ops
    run = Cases('label_fwd')
    for c in P.CASES['label']:
        d = P.label_inputs(c)
        B, C = c['B'], c['C']
        C1 = C - 1
        wd, ld_in = padded(np.concatenate([d['mean'], d['logvar']], 1), c['pad_in'], dev)
        eps, onehot = T(d['eps'], dev), T(d['onehot'], dev)
        bufs = Bufs(dev)
        w = bufs.out(B, C)
        rl = bufs.out(B, 3) if c['rowloss'] else None
        ops.label_fwd(B, C, wd, wd[:, C1:], ld_in, eps, onehot, d['prior'], w, rl)
        got = dict(w=N(w))
        if rl is not None:
            got['rowloss'] = N(rl)
        run.compare(c, got, P.ref_label_fwd(**d), bufs)
        if not c['onehot']:
            assert not got['rowloss'][:, 1:].any()                 # without onehot: w_rec and hit are zero
            continue
        bufs = Bufs(dev)
        ld_out = 2 * C1 + c['pad_out']
        dout = bufs.out(B, ld_out, pad_cols=c['pad_out'])
        ops.label_bwd(B, C, wd, wd[:, C1:], ld_in, eps, onehot, T(d['w'], dev), T(d['dw'], dev), d['prior'], d['class_weight'],
                      d['w_kl_weight'], d['inv_b'], dout, dout[:, C1:], ld_out)
        g = N(dout)
        run.compare(c, dict(dmean=g[:, :C1], dlogvar=g[:, C1:2 * C1]), P.ref_label_bwd(**d), bufs, kernel='label_bwd')
    run.done()


def test_gauss_fwd_and_bwd(dev):
    from clvae_amd import ops
    run = Cases('gauss_fwd')
    for c in P.CASES['gauss']:
        d = P.gauss_inputs(c)
        R, L = c['R'], c['L']
        za, eps = T(d['zargs'], dev), T(d['eps'], dev)
        bufs = Bufs(dev)
        z = bufs.out(R, L + c['pad_z'], pad_cols=c['pad_z'])
        kl = bufs.out(R) if c['rowkl'] else None
        ops.gauss_fwd(R, L, za, eps, z, L + c['pad_z'], kl)
        got = dict(z=N(z)[:, :L])
        if kl is not None:
            got['rowkl'] = N(kl)
        run.compare(c, got, P.ref_gauss_fwd(**d), bufs)
        bufs = Bufs(dev)
        dz, lddz = padded(d['dz'], c['pad_dz'], dev)
        dza = bufs.out(R, 2 * L)
        ops.gauss_bwd(R, L, za, eps, dz, lddz, d['kl_scale'], dza)
        run.compare(c, dict(dzargs=N(dza)), P.ref_gauss_bwd(**d), bufs, kernel='gauss_bwd')
    run.done()


def test_bernoulli_nll(dev):
    from clvae_amd import ops
    run = Cases('bernoulli_nll')
    for c in P.CASES['bernoulli_nll']:
        d = P.bernoulli_inputs(c)
        R, D = c['R'], c['D']
        y, ldy = padded(d['y'], c['pad_y'], dev)
        bufs = Bufs(dev)
        nll = bufs.out(R) if c['rownll'] else None
        dl = bufs.out(R, D) if c['dlogits'] else None
        ops.bernoulli_nll(R, D, T(d['logits'], dev), y, ldy, d['scale'], nll, dl)
        got = {}
        if nll is not None:
            got['rownll'] = N(nll)
        if dl is not None:
            got['dlogits'] = N(dl)
        run.compare(c, got, P.ref_bernoulli_nll(**d), bufs)
    run.done()


def test_sum_strided(dev):
    from clvae_amd import ops
    run = Cases('sum_strided')
    for c in P.CASES['sum_strided']:
        d = P.sum_strided_inputs(c)
        x = T(d['x'], dev)
        bufs = Bufs(dev)
        out, again = bufs.out(1), bufs.out(1)
        ops.sum_strided(d['n'], x, d['stride'], d['scale'], out)
        ops.sum_strided(d['n'], x, d['stride'], d['scale'], again)
        run.compare(c, dict(out=N(out)), P.ref_sum_strided(**d), bufs)
        run.same_bits(c, out, again)
    run.done()


def test_loss_sums(dev):
    from clvae_amd import ops
    run = Cases('loss_sums')
    for c in P.CASES['loss_sums']:
        d = P.loss_terms(c)
        terms = []
        for (kind, n), (x, _, st) in zip(c['terms'], d['terms']):
            if kind == 'm':                                      # contiguous, one float off the 16-byte alignment
                t = T(np.concatenate([[np.nan], x]), dev)[1:]
                assert t.data_ptr() % 16 == 4
            else:
                t = T(x, dev)
                assert t.data_ptr() % 16 == 0
            terms.append((t, n, st))
        bufs = Bufs(dev)
        out, again = bufs.out(5), bufs.out(5)
        ops.loss_sums(terms, out)
        ops.loss_sums(terms, again)
        run.compare(c, dict(out=N(out)), P.ref_loss_sums(**d), bufs)
        run.same_bits(c, out, again)
    run.done()


def test_colsum(dev):
    from clvae_amd import _lib, ops
    L = _lib.lib()
    run = Cases('colsum')
    for c in P.CASES['colsum']:
        d = P.colsum_inputs(c)
        M, Nn = c['M'], c['N']
        X, ldx = padded(d['X'], c['pad_x'], dev)
        need = L.clv_colsum_workspace_bytes(M, Nn)
        assert need == (M + 63) // 64 * Nn * 4
        bufs = Bufs(dev)
        outs = []
        for _ in range(2):
            out = bufs.out(Nn)
            if c['beta'] != 0:
                out.copy_(T(d['out0'], dev))                     # beta 0: NaN inside, which the kernel must not read
            ws = torch.full((need // 4 + TAIL,), CANARY, dtype=torch.float32, device=dev)
            ws[:need // 4] = float('nan')
            code = L.clv_colsum_f32(M, Nn, ops._ptr(X), ldx, float(c['beta']), ops._ptr(out), ops._ptr(ws), need, ops._stream())
            assert code == 0, code
            torch.cuda.synchronize()
            assert (N(ws)[need // 4:] == CANARY).all(), ("write behind the workspace", c)
            outs.append(out)
        run.compare(c, dict(out=N(outs[0])), P.ref_colsum(**d), bufs)
        run.same_bits(c, outs[0], outs[1])
    run.done()


@pytest.mark.parametrize("kernel", ['axpy', 'act_grad', 'scale_temper', 'sigmoid_temper', 'bernoulli_sample'])
def test_elementwise(dev, kernel):
    from clvae_amd import ops
    run = Cases(kernel)
    for c in P.CASES[kernel]:
        d = P.elementwise_inputs(kernel, c)
        n = c['n']
        bufs = Bufs(dev)
        if kernel == 'axpy':
            y = bufs.inp(d['y'])
            ops.axpy(n, d['alpha'], T(d['x'], dev), y)
            got = dict(y=N(y))
        elif kernel == 'act_grad':
            out = bufs.out(n)
            ops.act_grad(n, d['act'], T(d['y'], dev), T(d['dy'], dev), out)
            got = dict(dpre=N(out))
        elif kernel in ('scale_temper', 'sigmoid_temper'):
            x = bufs.inp(d['x'])
            getattr(ops, kernel)(n, x, d['alpha'])
            got = dict(x=N(x))
        else:
            x = bufs.out(n)
            ops.bernoulli_sample(n, T(d['p'], dev), T(d['u'], dev), x)
            got = dict(x=N(x))
        run.compare(c, got, P.REF[kernel](**d), bufs)
    run.done()


def test_dropout_rows(dev):
    from clvae_amd import ops
    run = Cases('dropout_rows')
    for c in P.CASES['dropout_rows']:
        d = P.dropout_inputs(c)
        R, n = c['R'], c['n']
        X, ldx = padded(d['X'], c['pads'][0], dev)
        Um, ldu = padded(d['Um'], c['pads'][1], dev)
        bufs = Bufs(dev)
        out = bufs.out(R, n + c['pads'][2], pad_cols=c['pads'][2])
        if c['beta'] != 0:
            out[:, :n] = T(d['out0'], dev)                       # beta 0: over NaN
        ops.dropout_rows(R, c['T'], n, X, ldx, Um, ldu, d['rate'], out, n + c['pads'][2], beta=d['beta'])
        run.compare(c, dict(out=N(out)[:, :n]), P.ref_dropout_rows(**d), bufs)
    run.done()


def test_bernoulli_sample_clamped(dev):
    from clvae_amd import ops
    run = Cases('bernoulli_sample_clamped')
    for c in P.CASES['bernoulli_sample_clamped']:
        d = P.clamped_inputs(c)
        R, D = c['R'], c['D']
        bufs = Bufs(dev)
        x = bufs.out(R, D)
        step = torch.tensor([d['counter']], dtype=torch.int32, device=dev)
        ops.bernoulli_sample_clamped(R * D, D, c['nsteps'], d['S'], T(d['p'], dev), T(d['u'], dev), T(d['clamp'], dev, torch.uint8), step, x)
        run.compare(c, dict(x=N(x)), P.ref_bernoulli_sample_clamped(**d), bufs)
        assert int(step.item()) == d['counter']
    run.done()


def test_take_frame(dev):
    from clvae_amd import ops
    run = Cases('take_frame')
    for c in P.CASES['take_frame']:
        d = P.take_frame_inputs(c)
        bufs = Bufs(dev)
        out = bufs.out(c['R'], c['D'])
        out.copy_(T(d['out0'], dev))
        step = torch.tensor([d['step']], dtype=torch.int32, device=dev)
        ops.take_frame(c['R'], c['T'], c['D'], T(d['src'], dev), step, out)
        run.compare(c, dict(out=N(out)), P.ref_take_frame(**d), bufs)          # outside [0, T): bitwise as it was
    run.done()


def test_lerp_rows(dev):
    from clvae_amd import ops
    run = Cases('lerp_rows')
    for c in P.CASES['lerp_rows']:
        d = P.lerp_inputs(c)
        R, n = len(d['alpha']), c['n']
        bufs = Bufs(dev)
        out = bufs.out(R, n)
        ops.lerp_rows(R, n, T(d['a'], dev), T(d['ia'], dev, torch.int32), T(d['b'], dev), T(d['ib'], dev, torch.int32),
                      T(d['alpha'], dev), out)
        ref = P.ref_lerp_rows(**d)
        run.compare(c, dict(out=N(out)), ref, bufs)
        ends = (d['alpha'] == 0) | (d['alpha'] == 1)                # a's row and b's row, bit for bit
        assert ends.sum() >= 6
        run.same_bits(c, out[torch.as_tensor(ends, device=dev)], T(ref['out'][0][ends], dev))
    run.done()


def test_gather_rows(dev):
    from clvae_amd import ops
    run = Cases('gather_rows')
    for c in P.CASES['gather_rows']:
        d = P.gather_inputs(c)
        chunk, out_ld = (c['chunk'], c['out_ld']) if c['chunk'] > 0 else (c['row_elems'], c['row_elems'])
        rows_out = c['rows'] * (c['row_elems'] // chunk)
        off = 1 if c['misaligned'] else 0
        bufs = Bufs(dev)
        flat = bufs.out(off + rows_out * out_ld)
        out = flat[off:].view(rows_out, out_ld)
        out[:, chunk:] = CANARY                                      # the columns a gather leaves alone
        src = T(d['src'], dev)
        assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 4 * off
        ops.gather_rows(c['rows'], c['row_elems'], src, T(d['idx'], dev, torch.int64), out, c['chunk'], c['out_ld'])
        run.compare(c, dict(out=N(out)), P.ref_gather_rows(**d), bufs)
        assert off == 0 or bool(torch.isnan(flat[0]))
    run.done()
