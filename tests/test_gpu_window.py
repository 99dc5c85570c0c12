"""-m gpu: the kernels that multiply piano-roll frames -- clv_sparse_proj, clv_sparse_proj2, clv_sparse_dense, clv_sparse_outer
(csrc/sparse_proj.hip), clv_dense_outer_bf16 and clv_dense_window_fwd_bf16 (csrc/outer_bf16.hip) -- against the fp64 reference
of tests/window_reference.py, over its case tables: EVERY output of every call, element by element, within its own bound
(bit for bit where the reference says so).

Buffers: every output is a helpers.Bufs buffer -- NaN inside, a canary tail, the canary in the padding columns of strided
outputs -- so an element left unwritten shows as a NaN and a write outside as a changed canary; the padding columns of
strided inputs hold 7.0 (255 in byte frames), so a read of one shows.  The window forward gets exactly
clv_dense_window_fwd_bf16_workspace_bytes plus a canary tail.  Byte frames: the float launch and the byte launch run on the
same case and must agree bit for bit in every output (torch.equal); the byte launch is the one checked against the
reference.  clv_sparse_proj2 must agree bit for bit with the two single launches.  A test goes through its case and reports
every failing output, each with the case, the output, the worst element's index and its error as a multiple of its bound.

Measured on an MI355X (the module's report, -s), cases and worst error / bound per entry point and output (the honest fp32
evaluations of tests/test_window_reference.py stay below 0.5 everywhere; the bounds are derived, these only record the margin):
  sparse_proj            13 cases   out 0.19 (bytes and dense frames; 0 / 1 frames bit for bit)
  sparse_proj2            5 cases   out0 0.19, out1 0.16; bit for bit the two single launches
  sparse_dense           12 cases   out 0.092
  sparse_outer           10 cases   out 0.14, colsum 0.045, gdot 0.072
  dense_outer_bf16       16 cases   out 0.089, colsum 0.048, gdot 0.056; byte launch = float launch bit for bit
  dense_window_fwd_bf16  12 cases   part 0.11, sum 0.083; byte launch = float launch bit for bit
No kernel exceeded a bound, left an element unwritten or touched a canary; no defect was found.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import window_reference as W
from helpers import Bufs

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
        print("\n%-24s %2d cases, worst error / bound: %s" % (k, _REPORT[k].pop('cases'), ", ".join("%s %.3g" % kv for kv in sorted(_REPORT[k].items()))),
              end="")
    print()


def F(a, dev):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=f32), device=dev)


def U8(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint8), device=dev)


def N(t):
    return t.detach().cpu().numpy()


def launches(X, kernel, dev):
    """the frames of a case on the device, once per launch it gets: the float copy, and the bytes themselves where the frames
    are bytes and the entry point takes them -- that launch last: it is the one compared with the reference"""
    X = np.asarray(X)
    return [F(X, dev)] + ([U8(X, dev)] if X.dtype == np.uint8 and kernel in W.BYTE_KERNELS else [])


def compare(kernel, case, got, ref, bufs, twins=()):
    """got {output: array} against the reference; `twins`: (what, {output: tensor}, {output: tensor}) that must be equal bit
    for bit.  Every failure of the case is reported."""
    fails = []
    rep = _REPORT.setdefault(kernel, dict(cases=0))
    rep['cases'] += 1
    assert set(got) == set(ref), (sorted(got), sorted(ref))
    for o in sorted(ref):
        if np.isnan(got[o]).any():
            fails.append("%s %r %s: %d elements of the written region are NaN" % (kernel, case, o, int(np.isnan(got[o]).sum())))
        try:
            v = W.check_all("%s %r" % (kernel, case), {o: got[o]}, {o: ref[o]})[o]
            rep[o] = max(rep.get(o, 0.0), v)
        except AssertionError as e:
            rep[o] = float('inf')
            fails.append(str(e))
    for what, a, b in twins:
        assert set(a) == set(b)
        for o in sorted(a):
            if not torch.equal(a[o], b[o]):
                n = int((a[o] != b[o]).sum())
                fails.append("%s %r %s: %s differ in %d of %d elements" % (kernel, case, o, what, n, a[o].numel()))
    try:
        torch.cuda.synchronize()
        bufs.check_canaries()
    except AssertionError as e:
        fails.append("%s %r: %s" % (kernel, case, e))
    assert not fails, "%d failures:\n%s" % (len(fails), "\n".join(fails[:20]))


def ids(kernel):
    return ["-".join("%s" % (v,) for k, v in c.items() if k != 'seed').replace(' ', '') for c in W.CASES[kernel]]


@pytest.mark.parametrize("c", W.CASES['sparse_proj'], ids=ids('sparse_proj'))
def test_sparse_proj(dev, c):
    from clvae_amd import ops
    d = W.proj_inputs(c)
    R, nx, Nn = c['R'], c['nx'], c['N']
    assert ops.sparse_proj_supported(nx, Nn)
    K = F(d['K'], dev)
    bufs, outs = Bufs(dev), []
    for Xd in launches(d['X'], 'sparse_proj', dev):
        out = bufs.out(R, c['ldo'], pad_cols=c['ldo'] - Nn)
        ops.sparse_proj(R, nx, Nn, Xd, c['ldx'], K, out, c['ldo'])
        outs.append(dict(out=out[:, :Nn]))
    twins = [("the float and the byte launch", outs[0], outs[1])] if len(outs) == 2 else []
    assert (len(outs) == 2) == (c['kind'] != 'dense')
    compare('sparse_proj', c, dict(out=N(outs[-1]['out'])), W.ref_sparse_proj(**d), bufs, twins)


@pytest.mark.parametrize("c", W.CASES['sparse_proj2'], ids=ids('sparse_proj2'))
def test_sparse_proj2(dev, c):
    from clvae_amd import ops
    d = W.proj2_inputs(c)
    R, Nn, ldo = c['R'], c['N'], c['ldo']
    Ks = [F(s['K'], dev) for s in d['sets']]
    bufs, outs = Bufs(dev), []
    for Xa, Xb in zip(*[launches(s['X'], 'sparse_proj2', dev) for s in d['sets']]):
        pair = [bufs.out(R, ldo, pad_cols=ldo - Nn) for _ in range(2)]
        single = [bufs.out(R, ldo, pad_cols=ldo - Nn) for _ in range(2)]
        args = [(s['nx'], Xd, ldx, K) for s, Xd, (_, ldx), K in zip(d['sets'], (Xa, Xb), c['sets'], Ks)]
        ops.sparse_proj2(R, Nn, args[0] + (pair[0],), args[1] + (pair[1],), ldo)
        for (nx, Xd, ldx, K), o in zip(args, single):
            ops.sparse_proj(R, nx, Nn, Xd, ldx, K, o, ldo)
        outs.append((dict(out0=pair[0][:, :Nn], out1=pair[1][:, :Nn]), dict(out0=single[0][:, :Nn], out1=single[1][:, :Nn])))
    twins = [("the pair launch and the two single launches", p, s) for p, s in outs]
    if len(outs) == 2:
        twins.append(("the float and the byte launch", outs[0][0], outs[1][0]))
    compare('sparse_proj2', c, {o: N(v) for o, v in outs[-1][0].items()}, W.ref_sparse_proj2(**d), bufs, twins)


@pytest.mark.parametrize("c", W.CASES['sparse_dense'], ids=ids('sparse_dense'))
def test_sparse_dense(dev, c):
    from clvae_amd import ops
    d = W.dense_inputs(c)
    R, nx, Nn = c['R'], c['nx'], c['N']
    assert ops.sparse_dense_supported(Nn)
    bufs = Bufs(dev)
    out = bufs.out(R, c['ldo'], pad_cols=c['ldo'] - Nn)
    ops.sparse_dense(R, nx, Nn, F(d['X'], dev), c['ldx'], F(d['K'], dev), F(d['bias'], dev), c['act'], out, c['ldo'])
    compare('sparse_dense', c, dict(out=N(out)[:, :Nn]), W.ref_sparse_dense(**d), bufs)


def run_outer(kernel, fn, dev, c):
    d = W.outer_inputs(c)
    Bn, nx, Nn = c['Bn'], c['nx'], c['N']
    G, H, hb = F(d['G'], dev), F(d.get('H'), dev), F(d.get('hb'), dev)
    bufs, outs = Bufs(dev), []
    for Xd in launches(d['X'], kernel, dev):
        o = dict(out=bufs.out(nx, c['ldo'], pad_cols=c['ldo'] - Nn))
        cs = bufs.out(Nn) if c['colsum'] else None
        gd = bufs.out(Nn) if c['gdot'] else None
        fn(Bn, nx, Nn, Xd, c['ldx'], G, c['ldg'], o['out'], c['ldo'], colsum=cs, gdot=(H, c['ldh'], hb, gd) if c['gdot'] else None)
        o['out'] = o['out'][:, :Nn]
        if cs is not None:
            o['colsum'] = cs
        if gd is not None:
            o['gdot'] = gd
        outs.append(o)
    twins = [("the float and the byte launch", outs[0], outs[1])] if len(outs) == 2 else []
    got = {o: N(v) for o, v in outs[-1].items()}
    ref = W.ref_outer(**d)
    compare(kernel, c, got, ref, bufs, twins)
    if c.get('chain'):          # gdot = sum_j K dK, what the optimizer takes it for: within the sum of both bounds
        K = W.r32(d['K'])
        W.check("%s %r gdot against sum_j K dK" % (kernel, c), got['gdot'], (K * ref['out'][0]).sum(0),
                ref['gdot'][1] + (np.abs(K) * ref['out'][1]).sum(0))


@pytest.mark.parametrize("c", W.CASES['sparse_outer'], ids=ids('sparse_outer'))
def test_sparse_outer(dev, c):
    from clvae_amd import ops
    run_outer('sparse_outer', ops.sparse_outer, dev, c)


@pytest.mark.parametrize("c", W.CASES['dense_outer_bf16'], ids=ids('dense_outer_bf16'))
def test_dense_outer_bf16(dev, c):
    from clvae_amd import ops
    assert ops.dense_outer_bf16_supported(c['Bn'], c['nx'], c['N'], c['ldx'], c['ldg'])
    run_outer('dense_outer_bf16', ops.dense_outer_bf16, dev, c)


@pytest.mark.parametrize("c", W.CASES['dense_window_fwd_bf16'], ids=ids('dense_window_fwd_bf16'))
def test_dense_window_fwd_bf16(dev, c):
    from clvae_amd import _lib, ops
    L = _lib.lib()
    d = W.window_inputs(c)
    Bn, nx, Nn = c['Bn'], c['nx'], c['N']
    assert ops.dense_window_fwd_bf16_supported(Bn, nx, Nn, c['ldx'], c['ldk'])
    splits, chunk = W.window_split(Bn, nx)
    need = L.clv_dense_window_fwd_bf16_workspace_bytes(Bn, nx, Nn)
    assert splits == L.clv_dense_window_fwd_bf16_splits(Bn, nx) and need == splits * Bn * Nn * 4
    K = F(d['K'], dev)
    bufs, outs = Bufs(dev), []
    for Xd in launches(d['X'], 'dense_window_fwd_bf16', dev):
        part = bufs.out(splits, Bn, Nn)                                     # exactly the workspace, the canary tail behind it
        code = L.clv_dense_window_fwd_bf16(Bn, nx, Nn, ops._ptr(Xd), ops._is_u8(Xd), c['ldx'], ops._ptr(K), c['ldk'], ops._ptr(part),
                                           need, ops._stream())
        assert code == 0, code
        outs.append(dict(part=part))
    assert len(outs) == 2
    compare('dense_window_fwd_bf16', c, W.window_outputs(N(outs[-1]['part'])), W.ref_dense_window_fwd_bf16(**d), bufs,
            [("the float and the byte launch", outs[0], outs[1])])
