"""-m gpu: clv_lstm_wgrad and clv_lstm_wgrad_pair (csrc/wgrad_bf16.hip) element by element against the fp64 reference and the
per-element bound of tests/wgrad_reference.py (its derivation, the planted faults it rejects: tests/test_wgrad_reference.py).

The C entry points are called directly (`_lib.lib()`, `_lib.WgradProblem`), so that what `ops.lstm_wgrad` fixes is free: beta,
every row stride (ldx, ldh, ldz, lddz, ld_kx, ld_u, ld_kz), h_shift in {0, 1, 2}, h_zero_period = 0, nx in {4, 64, 88, 96} and
the (nh, nz) of both kernel forms up to their boundaries ((88, 8) | (88, 9), (96, 1), (64, 32), (96, 32)).  Every operand is a
view into an allocation that is NaN (bytes: 255) in 64 guard rows on either side and in its padding columns; every output
sits in a tests/helpers.py buffer with a canary tail and canaries in the stride padding, NaN inside (beta == 0) or the known
finite C (beta != 0).  Every case runs four times -- reduced at once and through a clv_reduce_job + clv_splitk_reduce_multi,
each twice -- and the four results must agree bit for bit (the header: "bit-identical either way").

Which instance a case launches (wide = nh + nz > 96 or nz > 8; the tables hold all of them, single and pair:
test_the_tables_reach_every_instance_and_every_contract_value):
  <6, 3>      narrow, general float frames      <6, 1>      narrow, exact float frames      <6, 1, u8>  narrow, byte frames
  <8, 1>      wide, exact float frames          <8, 1, u8>  wide, byte frames               (<8, 3> is refused: no room in LDS)

Measured on one MI355X run (worst |err| / bound per output over the tables; the module's wall time):
  instance     single (dKx, dU, dKz)      pair (dKx, dU, dKz)
  <6, 3>       0.168  0.156  0.154        0.197  0.164  0.140
  <6, 1>       0.124  0.191  0.119        0.082  0.161  0.123
  <6, 1, u8>   0.183  0.143  -            0.115  0.156  0.104
  <8, 1>       0.150  0.174  0.154        0.141  0.182  0.202
  <8, 1, u8>   0.173  0.191  0.148        0.186  0.173  0.166
  69 tests in 8.0 s (9.8 s with start-up); tests/test_gpu_wgrad_edges.py in the same run: 67 tests in 5.4 s (7.0 s).
"""
import ctypes as C

import numpy as np
import pytest

import wgrad_reference as W
from helpers import Bufs

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

N, GUARD = W.N, 64
EINVAL, EWORKSPACE = -1, -2
SINGLE, PAIRS = W.single_cases(), W.pair_cases()
RATIOS = {}                      # (instance, 'single' | 'pair', tensor) -> worst |err| / bound


def case_id(c):
    return "K%d-nx%d-nh%d-nz%d-%s-T%d-s%d-b%g-x%d-%s" % (c.K, c.nx, c.nh, c.nz, c.frames, c.period, c.h_shift, c.beta, c.scale, c.family)


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def guarded(a, n, dev):
    """The device copy of a [K, ld] as rows [GUARD, GUARD + K) of an allocation that is NaN (255 for bytes) everywhere else,
    the padding columns n.. of its own rows included."""
    u8 = a.dtype == np.uint8
    big = np.full((a.shape[0] + 2 * GUARD, a.shape[1]), 255 if u8 else np.nan, a.dtype)
    big[GUARD:GUARD + a.shape[0], :n] = a[:, :n]
    return torch.as_tensor(big, device=dev)[GUARD:GUARD + a.shape[0]]


class Problem:
    """one product: the case's operands on the device, fresh outputs per run, the reference and the bounds"""

    def __init__(self, dev, c):
        self.c, self.dev, self.D = c, dev, W.build(c)
        D = self.D
        self.X, self.H, self.dz = guarded(D.X, c.nx, dev), guarded(D.H, c.nh, dev), guarded(D.dz, N, dev)
        self.Z = guarded(D.Z, c.nz, dev) if c.nz else None
        self.ld = W.strides(c)
        self.rows = [(t, n, self.ld[l]) for t, n, l in (('dKx', c.nx, 'ld_kx'), ('dU', c.nh, 'ld_u'), ('dKz', c.nz, 'ld_kz')) if n]

    def outputs(self):
        bufs, out = Bufs(self.dev), {}
        for t, n, ld in self.rows:
            out[t] = bufs.out(n, ld, pad_cols=ld - N)
            if self.c.beta != 0:
                out[t][:, :N] = torch.as_tensor(self.D.C0[t][:, :N], device=self.dev)
        return bufs, out

    def struct(self, out, ws):
        from clvae_amd import _lib
        c, p_ = self.c, lambda t: None if t is None else C.c_void_p(t.data_ptr())
        w = _lib.WgradProblem()
        w.K, w.N = c.K, N
        w.X, w.ldx, w.nx, w.x_exact_bf16 = p_(self.X), self.ld['ldx'], c.nx, W.FRAMES_MODE[c.frames]
        w.H, w.ldh, w.nh, w.h_shift, w.h_zero_period = p_(self.H), self.ld['ldh'], c.nh, c.h_shift, c.period
        w.Z, w.ldz, w.nz = p_(self.Z), self.ld['ldz'] if c.nz else 0, c.nz
        w.dz, w.lddz = p_(self.dz), self.ld['lddz']
        w.dKx, w.ld_kx, w.dU, w.ld_u = p_(out['dKx']), self.ld['ld_kx'], p_(out['dU']), self.ld['ld_u']
        w.dKz, w.ld_kz = p_(out.get('dKz')), self.ld['ld_kz'] if c.nz else 0
        w.beta = float(c.beta)
        w.ws, w.ws_bytes = p_(ws), 0 if ws is None else ws.numel()
        return w

    def check(self, runs, what, kind):
        """runs: [{tensor: device tensor}] of the four launches"""
        host = [{t: o[t][:, :N].cpu().numpy() for t in o} for o in runs]
        for h in host[1:]:
            for t in h:
                assert np.array_equal(h[t], host[0][t], equal_nan=True), (what, t, "the launches differ")
        ref, bnd = W.reference(self.c, self.D), W.bound(self.c, self.D)
        for t, got in host[0].items():
            bad = W.first_offender(got, ref[t], bnd[t][0])
            assert bad is None, "%s: %s[%d, %d] is off by %.3e, bound %.3e" % ((what, t) + bad)
            key = (W.instance(self.c), kind, t)
            RATIOS[key] = max(RATIOS.get(key, 0.0), W.worst_ratio(got, ref[t], bnd[t][0]))


def workspace(dev, nbytes):
    return torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=dev)


def single_args(w, scale, ws, job):
    return (w.K, w.N, w.X, w.ldx, w.nx, w.x_exact_bf16, w.H, w.ldh, w.nh, w.h_shift, w.h_zero_period, w.Z, w.ldz, w.nz, w.dz, w.lddz,
            w.dKx, w.ld_kx, w.dU, w.ld_u, w.dKz, w.ld_kz, w.beta, scale, w.ws, w.ws_bytes, job)


def reduce_now(jobs, n):
    from clvae_amd import _lib, ops
    assert _lib.lib().clv_splitk_reduce_multi(jobs, n, None, None, None, 0, None, None, 0, ops._stream()) == 0


@pytest.mark.parametrize("c", SINGLE, ids=case_id)
def test_single_launch_against_the_bound(dev, c):
    from clvae_amd import _lib, ops
    L = _lib.lib()
    assert L.clv_lstm_wgrad_supported(N, c.nx, c.nh, c.nz, W.FRAMES_MODE[c.frames])
    p = Problem(dev, c)
    ws = workspace(dev, L.clv_lstm_wgrad_workspace_bytes(c.K, N, c.nx, c.nh, c.nz, c.scale))
    runs, keep = [], []
    for defer in (False, True, False, True):
        bufs, out = p.outputs()
        jobs = (_lib.ReduceJob * 1)()
        w = p.struct(out, ws)
        st = L.clv_lstm_wgrad(*single_args(w, c.scale, ws, C.byref(jobs[0]) if defer else None), ops._stream())
        assert st == 0, st
        if defer:
            reduce_now(jobs, 1)
        torch.cuda.synchronize()
        bufs.check_canaries()
        runs.append(out)
        keep.append(bufs)
    p.check(runs, case_id(c), 'single')


@pytest.mark.parametrize("pq", PAIRS, ids=lambda pq: case_id(pq[0]) + "+" + case_id(pq[1]))
def test_pair_launch_against_the_bound(dev, pq):
    from clvae_amd import _lib, ops
    L = _lib.lib()
    ps = [Problem(dev, c) for c in pq]
    scale = pq[0].scale
    wss = [workspace(dev, L.clv_lstm_wgrad_pair_workspace_bytes(c.K, N, c.nx, c.nh, c.nz, scale)) for c in pq]
    runs, keep = ([], []), []
    for defer in (False, True, False, True):
        outs = [p.outputs() for p in ps]
        w = [p.struct(o[1], ws) for p, o, ws in zip(ps, outs, wss)]
        assert L.clv_lstm_wgrad_pair_supported(C.byref(w[0]), C.byref(w[1]))
        jobs = (_lib.ReduceJob * 2)()
        st = L.clv_lstm_wgrad_pair(C.byref(w[0]), C.byref(w[1]), scale, C.byref(jobs[0]) if defer else None,
                                   C.byref(jobs[1]) if defer else None, ops._stream())
        assert st == 0, st
        if defer:
            reduce_now(jobs, 2)
        torch.cuda.synchronize()
        for (bufs, out), r in zip(outs, runs):
            bufs.check_canaries()
            r.append(out)
        keep.append(outs)
    for p, r in zip(ps, runs):
        p.check(r, "pair " + case_id(p.c), 'pair')


def test_the_tables_reach_every_instance_and_every_contract_value():
    """computed from the tables with the launcher's dispatch rule restated from the header: wide = nh + nz > 96 or nz > 8"""
    wide = lambda c: c.nh + c.nz > 96 or c.nz > 8
    for cs in (SINGLE, [c for pq in PAIRS for c in pq]):
        assert {(wide(c), c.frames) for c in cs} == {(False, 'u8'), (False, 'exact'), (False, 'general'), (True, 'u8'), (True, 'exact')}
    cs = SINGLE + [c for pq in PAIRS for c in pq]
    assert {c.beta for c in cs} == {0.0, 1.0, -0.5}
    assert {c.h_shift for c in cs} == {0, 1, 2}
    assert any(c.period == 0 for c in cs)
    for name in W.PAD_NAMES:                                   # every stride padded somewhere, and plain somewhere
        n = {'ldx': 'nx', 'ldh': 'nh', 'ldz': 'nz'}.get(name)
        live = [c for c in cs if name not in ('ldz', 'ld_kz') or c.nz]
        pad = {W.strides(c)[name] - (getattr(c, n) if n else N) for c in live}
        assert 0 in pad and max(pad) > 0, name
    for p, q in PAIRS:
        assert wide(p) == wide(q) and (p.nz, p.nh, p.pads, p.beta) != (q.nz, q.nh, q.pads, q.beta)
        assert W.instance(p) == W.instance(q)


def test_refusals_return_the_documented_status_and_launch_nothing(dev):
    """EINVAL (a short workspace: EWORKSPACE) from the argument checks on; the outputs keep their NaN and their canaries."""
    from clvae_amd import _lib, ops
    L = _lib.lib()
    base = W.Case(K=64, nx=88, nh=88, nz=2, frames='exact', period=16, h_shift=1, beta=0.0, scale=1, base=128,
                  pads=(4, 4, 3, 4, 4, 4, 4), family='wide', seed=0)
    ws = workspace(dev, 1 << 22)
    checked = []

    def refused(c, expect=EINVAL, scale=1, edit=None, ws_bytes=None, pair_with=None):
        p = Problem(dev, c)
        bufs, out = p.outputs()
        w = p.struct(out, ws)
        if ws_bytes is not None:
            w.ws_bytes = ws_bytes
        if edit:
            edit(w)
        jobs = (_lib.ReduceJob * 2)()
        C.memset(jobs, 0x55, C.sizeof(jobs))
        if pair_with is None:
            assert L.clv_lstm_wgrad(*single_args(w, scale, ws, C.byref(jobs[0])), ops._stream()) == expect
            other = w
        else:
            q = Problem(dev, pair_with)
            bq, oq = q.outputs()
            other = q.struct(oq, workspace(dev, 1 << 22))
            assert not L.clv_lstm_wgrad_pair_supported(C.byref(w), C.byref(other))
            checked.append((bq, oq))
        for a, b in ((w, other), (other, w)):
            if pair_with is not None or expect == EINVAL:      # (the pair's workspace is half the single launch's: EINVAL cases only)
                assert L.clv_lstm_wgrad_pair(C.byref(a), C.byref(b), scale, C.byref(jobs[0]), C.byref(jobs[1]), ops._stream()) == EINVAL
        called_pair = pair_with is not None or expect == EINVAL
        assert bytes(jobs if called_pair else jobs[0]) == bytes(C.sizeof(jobs if called_pair else jobs[0])), "a refused call leaves its jobs all zero"
        checked.append((bufs, out))

    off = lambda name, by: lambda w: setattr(w, name, C.c_void_p(getattr(w, name) + by))
    refused(base._replace(nx=6, pads=(2, 4, 3, 4, 4, 4, 4)))                 # nx % 4
    refused(base._replace(nh=86, pads=(4, 6, 3, 4, 4, 4, 4)))                # nh % 4
    refused(base._replace(pads=(2, 4, 3, 4, 4, 4, 4)))                       # ldx % 4
    refused(base._replace(pads=(4, 2, 3, 4, 4, 4, 4)))                       # ldh % 4
    refused(base._replace(pads=(4, 4, 3, 2, 4, 4, 4)))                       # lddz % 4
    refused(base._replace(frames='u8', pads=(2, 4, 3, 4, 4, 4, 4)))          # byte rows: ldx % 4 as well
    for name in ('X', 'H', 'dz'):
        refused(base, edit=off(name, 4))                                     # bases off a 16-byte boundary
    refused(base._replace(frames='u8'), edit=off('X', 1))                    # byte frames: 4-byte aligned
    refused(base._replace(frames='general', nh=88, nz=9))                    # the wide form with float frames: by nz alone,
    refused(base._replace(frames='general', nh=96, nz=1))                    # ... by nh + nz alone
    refused(base._replace(nh=100, nz=32))                                    # nh + nz > 128
    refused(base._replace(nz=33))
    refused(base, scale=0)
    refused(base, scale=9)
    need = L.clv_lstm_wgrad_workspace_bytes(base.K, N, base.nx, base.nh, base.nz, 1)
    refused(base, expect=EWORKSPACE, ws_bytes=need - 1)
    refused(base, expect=EWORKSPACE, edit=lambda w: setattr(w, 'ws', None))
    # rows shorter than what is read or written of them, a negative shift or period
    refused(base, edit=lambda w: setattr(w, 'ldz', 1))
    refused(base, edit=lambda w: setattr(w, 'ld_kx', N - 4))
    refused(base, edit=lambda w: setattr(w, 'ld_u', N - 4))
    refused(base, edit=lambda w: setattr(w, 'ld_kz', N - 4))
    refused(base, edit=lambda w: setattr(w, 'lddz', N - 4))
    refused(base, edit=lambda w: setattr(w, 'h_shift', -1))
    refused(base, edit=lambda w: setattr(w, 'h_zero_period', -16))
    # a pair: unequal K, unequal frame modes, unequal forms of the kernel
    refused(base, pair_with=base._replace(K=96))
    refused(base, pair_with=base._replace(frames='u8'))
    refused(base, pair_with=base._replace(nz=9))
    torch.cuda.synchronize()
    for bufs, out in checked:
        bufs.check_canaries()
        for o in out.values():
            assert bool(torch.isnan(o[:, :N]).all()), "a refused call wrote an output"


def test_measured_ratios_are_reported():
    """(runs last: prints what the module docstring and DESIGN.md record)"""
    for (inst, kind, t), r in sorted(RATIOS.items(), key=str):
        print("wgrad ratio <%d, %d%s> %s %s: %.3f" % (inst[0], inst[1], ', u8' if inst[2] else '', kind, t, r))
        assert r <= 1.0
