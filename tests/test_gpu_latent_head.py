"""-m gpu: clv_latent_head_fwd / clv_latent_head_bwd (csrc/latent_head.hip) called directly through ctypes, both templates
(latent_dim <= 16 / <= 32), every output against the fp64 reference of tests/latent_head_reference.py: each element of
zargs, Z, rowkl, dzargs, dhs, dWz, dbz within its own bound, every tensor of at least 1000 elements with rms(err / sigma) <= 1.
The backward pass is fed the reference's zargs rounded to fp32 (its contract takes zargs as an exact input); one chained
run per template feeds it the device's own, as a training step does.

Buffers: every output NaN-filled (helpers.Bufs) with a canary tail; Z lives in an [R,ldz] buffer whose padding columns hold
the canary and must keep it, dZ's padding columns hold NaN; hs, zargs (as an input), eps and dZ are views with 64 NaN guard
rows before and behind, so that a read outside [0, R) shows as a NaN; dWz and dbz are views into one flat buffer with
canaries in front, between and behind; the workspace is exactly clv_latent_head_bwd_workspace_bytes(R, L), NaN-filled, plus a
canary tail; a forward pass that does not draw leaves eps bitwise unchanged.  Only hs must be 16-byte aligned: a third of
the cases run with Wz, bz, eps, zargs, Z, dZ, dzargs and dhs one float past a 16-byte boundary (each alone too), the float in
front of each NaN before and after.
Cases: latent_head_reference.GPU_CASES (R 1 .. 128 * 513 + 7 on the wave tile, the block and the 256-workgroup grid cap, every
L kind, pitches L, L + 3, L + 8, immediate and deferred reduction, dzargs stored or NULL, rowkl present or NULL), the edge case
(log_var +-40, mean = 0, eps = 0, dZ = 0, kl_scale = 0), bitwise properties, noise drawn in the kernel, the host's refusals.
Every GPU call is an ordinary in-bounds launch.
NOT exercised: R beyond the 32-bit range of blk * 128 and of the byte offsets in the buffer descriptors (R * 2L * 4 bytes per
block is far below it; a row count of 2^24 and more would need arrays of several GB and minutes of fp64 on the host);
denormal values; a stream other than the current one; launches captured into a graph.
The worst error / bound and rms per output and template are printed at the end of the module (-s)."""
import ctypes as Ct

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import latent_head_reference as LR
from oracle import philox as OP
from helpers import Bufs, CANARY, TAIL

pytestmark = pytest.mark.gpu

H = 88
GUARD = 64
EINVAL, EWORKSPACE = -1, -2
FWD_SCOPE, BWD_SCOPE = 'latent_head_fwd', 'latent_head_bwd'
DW_OFF = 8
MISALIGNABLE = ('Wz', 'bz', 'eps', 'zargs', 'Z', 'dZ', 'dzargs', 'dhs')
_REPORT = dict(ratios={}, rms={}, calls={})


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    yield torch.device("cuda:0")
    r = _REPORT
    for t in sorted(r['ratios']):
        print("\nlatent head <%d> (%d comparisons): worst error / bound: %s" % (t, r['calls'][t], ", ".join("%s %.3g" % kv for kv in r['ratios'][t].items())))
        print("latent head <%d>: worst rms(err / sigma): %s" % (t, ", ".join("%s %.3g" % kv for kv in r['rms'][t].items())))


def N(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


class Inp:
    """an input on the device: `a` inside an allocation that is NaN everywhere else -- GUARD rows (or, for a vector, GUARD
    elements) before and behind; mis: the view starts one float past a 16-byte boundary"""

    def __init__(self, a, dev, mis=0, fill_nan=False):
        a = np.ascontiguousarray(a, dtype=np.float32)
        g = -(-GUARD * (a.shape[1] if a.ndim == 2 else 1) // 4) * 4
        flat = np.full(g + 4 + a.size + g, np.nan, np.float32)
        self.lo, self.n = g + mis, a.size
        if not fill_nan:
            flat[self.lo:self.lo + a.size] = a.ravel()
        self.raw = torch.as_tensor(flat, device=dev)
        self.v = self.raw[self.lo:self.lo + a.size].view(*a.shape)
        assert self.v.data_ptr() % 16 == 4 * mis
        self.before = bits(self.raw)

    def unchanged(self):
        return np.array_equal(bits(self.raw), self.before)

    def outside_unchanged(self):
        b = bits(self.raw)
        return np.array_equal(b[:self.lo], self.before[:self.lo]) and np.array_equal(b[self.lo + self.n:], self.before[self.lo + self.n:])


class Outs:
    """NaN-filled outputs (helpers.Bufs: canary tails); a misaligned one starts one float into its buffer"""

    def __init__(self, dev, mis=()):
        self.bufs, self.mis, self.fronts = Bufs(dev), mis, []

    def out(self, name, *shape, keep=None):
        n = int(np.prod(shape))
        flat = self.bufs.out(n + 4)
        m = 1 if name in self.mis else 0
        v = flat[m:m + n].view(*shape)
        assert v.data_ptr() % 16 == 4 * m
        if keep is not None:                     # the padding columns of a strided output: the canary
            v[:, keep:] = CANARY
        self.fronts.append((name, flat, m, n, shape, keep))
        return v

    def check(self):
        self.bufs.check_canaries()
        for name, flat, m, n, shape, keep in self.fronts:
            f = flat.cpu().numpy()
            assert np.isnan(f[:m]).all() and np.isnan(f[m + n:]).all(), "write beside " + name
            if keep is not None:
                assert (f[m:m + n].reshape(shape)[:, keep:] == CANARY).all(), "padding column of %s written" % name


def _profiled(fn):
    """fn() with the profiler on: (status, the scope names seen)"""
    from clvae_amd import ops
    ops.prof_enable(True)
    try:
        st = fn()
        torch.cuda.synchronize()
        names = [n for n, _, _ in ops.prof_collect()]
    finally:
        ops.prof_enable(False)          # process-wide: no other module sees it on
    return st, names


def inputs(dev, case, mis=()):
    m = lambda k: 1 if k in mis else 0
    return dict(hs=Inp(case['hs'], dev), Wz=Inp(case['Wz'], dev, m('Wz')), bz=Inp(case['bz'], dev, m('bz')),
                eps=Inp(case['eps'], dev, m('eps')), dZ=Inp(case['dZpad'], dev, m('dZ')))


def run_fwd(dev, case, inp=None, mis=(), rowkl=True, noise=None, **override):
    """one clv_latent_head_fwd; returns (status, outputs or None).  noise: (seed, stream, step, first, step_dev tensor or
    None): eps is an output then (got['eps'])."""
    from clvae_amd import _lib, ops
    p_ = ops._ptr
    R, L, ldz = case['R'], case['L'], case['ldz']
    inp = inp or inputs(dev, case, mis)
    eps = Inp(case['eps'], dev, 1 if 'eps' in mis else 0, fill_nan=True) if noise else inp['eps']
    o = Outs(dev, mis)
    zargs, Z = o.out('zargs', R, 2 * L), o.out('Z', R, ldz, keep=L)
    kl = o.out('rowkl', R) if rowkl else None
    nz = None
    if noise:
        seed, stream, step, first, step_dev = noise
        nz = _lib.NoiseDraw(int(seed), int(first), int(stream), int(step), p_(step_dev))
    a = dict(R=R, H=H, L=L, hs=p_(inp['hs'].v), Wz=p_(inp['Wz'].v), bz=p_(inp['bz'].v), eps=p_(eps.v), zargs=p_(zargs), Z=p_(Z), ldz=ldz)
    a.update(override)
    st, names = _profiled(lambda: _lib.lib().clv_latent_head_fwd(a['R'], a['H'], a['L'], a['hs'], a['Wz'], a['bz'], a['eps'], a['zargs'],
                                                                 a['Z'], a['ldz'], p_(kl), Ct.byref(nz) if nz else None, ops._stream()))
    o.check()
    for k in ('hs', 'Wz', 'bz'):
        assert inp[k].unchanged(), k + " written"
    if st != 0:
        assert FWD_SCOPE not in names, "a kernel was launched although the call failed"
        assert torch.isnan(zargs).all() and torch.isnan(Z[:, :L]).all() and (kl is None or torch.isnan(kl).all()) and eps.unchanged()
        return st, None
    assert FWD_SCOPE in names
    if noise:
        assert eps.outside_unchanged(), "eps written outside its R rows"
    else:
        assert eps.unchanged(), "eps written by a forward pass that does not draw"
    got = dict(zargs=N(zargs), Z=N(Z)[:, :L], rowkl=N(kl), eps=N(eps.v))
    got['_t'] = dict(zargs=zargs, Z=Z, rowkl=kl, eps=eps)
    return st, got


def run_bwd(dev, case, zin, inp=None, mis=(), red='i', stored=True, **override):
    """one clv_latent_head_bwd from the zargs `zin` (fp32 values); returns (status, outputs or None)"""
    from clvae_amd import _lib, ops
    p_ = ops._ptr
    lib = _lib.lib()
    R, L, lddz = case['R'], case['L'], case['lddz']
    inp = inp or inputs(dev, case, mis)
    za = Inp(zin, dev, 1 if 'zargs' in mis else 0)
    ep = inp['eps']
    o = Outs(dev, mis)
    dhs = o.out('dhs', R, H)
    dz = o.out('dzargs', R, 2 * L) if stored else None
    db_off = DW_OFF + H * 2 * L + 12
    g_len = db_off + 2 * L
    G = torch.full((g_len + TAIL,), CANARY, dtype=torch.float32, device=dev)
    dWz, dbz = G[DW_OFF:DW_OFF + H * 2 * L].view(H, 2 * L), G[db_off:db_off + 2 * L]
    dWz.fill_(float('nan'))
    dbz.fill_(float('nan'))
    need = lib.clv_latent_head_bwd_workspace_bytes(R, L)
    blocks = -(-R // LR.BLOCK)
    assert need == min(blocks, LR.GRID) * (H + 1) * 2 * L * 4
    ws = torch.full((need // 4 + TAIL,), CANARY, dtype=torch.float32, device=dev)
    ws[:need // 4] = float('nan')
    rq = ops.ReduceQueue(dev) if red == 'd' else None
    job = rq.next_job() if rq is not None else None
    if rq is not None and override:              # a refusal must clear the job it was handed
        Ct.memset(Ct.addressof(rq.jobs), 0xFF, Ct.sizeof(_lib.ReduceJob))
    a = dict(R=R, H=H, L=L, hs=p_(inp['hs'].v), Wz=p_(inp['Wz'].v), zargs=p_(za.v), eps=p_(ep.v), dZ=p_(inp['dZ'].v), lddz=lddz,
             dhs=p_(dhs), dWz=p_(dWz), dbz=p_(dbz), ws=p_(ws), ws_bytes=need)
    a.update(override)
    st, names = _profiled(lambda: lib.clv_latent_head_bwd(a['R'], a['H'], a['L'], a['hs'], a['Wz'], a['zargs'], a['eps'], a['dZ'], a['lddz'],
                                                          float(case['kl']), p_(dz), a['dhs'], a['dWz'], a['dbz'], a['ws'], a['ws_bytes'],
                                                          job, ops._stream()))
    o.check()
    for k, b in list(inp.items()) + [('zargs', za), ('eps', ep)]:
        assert b.unchanged(), k + " written"
    g = G.cpu().numpy()
    gap = np.ones(g_len + TAIL, bool)
    gap[DW_OFF:DW_OFF + H * 2 * L] = gap[db_off:db_off + 2 * L] = False
    assert (g[gap] == CANARY).all(), "write beside dWz / dbz in the flat gradient buffer"
    assert (ws[need // 4:] == CANARY).all(), "write behind the workspace"
    if st != 0:
        assert BWD_SCOPE not in names, "a kernel was launched although the call failed"
        assert torch.isnan(dhs).all() and torch.isnan(dWz).all() and torch.isnan(dbz).all() and (dz is None or torch.isnan(dz).all())
        assert torch.isnan(ws[:need // 4]).all()
        assert rq is None or not any(bytes(rq.jobs[0].opaque)), "the job of a refused call is not all zero"
        return st, None
    assert BWD_SCOPE in names
    if rq is not None:
        empty = not any(bytes(rq.jobs[0].opaque))
        if blocks == 1:      # a single slab is reduced at once: the job comes back all zero, the gradients are complete
            assert empty and not torch.isnan(dWz).any() and not torch.isnan(dbz).any()
        else:
            assert not empty and torch.isnan(dWz).all() and torch.isnan(dbz).all()
        rq.flush()
        torch.cuda.synchronize()
        assert (ws[need // 4:] == CANARY).all(), "the reduction wrote behind the workspace"
        assert (G.cpu().numpy()[gap] == CANARY).all(), "the reduction wrote beside dWz / dbz"
    return st, dict(dzargs=N(dz), dhs=N(dhs), dWz=N(dWz), dbz=N(dbz))


def check(case, got, ref, what):
    """every element against its bound, every tensor against the rms criterion; records the figures per template"""
    rt, rm = LR.ratios(got, ref), LR.rms(got, ref)
    print("%s R=%d L=%d: error / bound %s | rms %s" % (what, case['R'], case['L'], " ".join("%s %.3g" % kv for kv in rt.items()),
                                                        " ".join("%s %.3g" % kv for kv in rm.items())))
    t = LR.lp16(case['L'])
    _REPORT['calls'][t] = _REPORT['calls'].get(t, 0) + 1
    for name, d in (('ratios', rt), ('rms', rm)):
        agg = _REPORT[name].setdefault(t, {})
        for k, v in d.items():
            agg[k] = max(agg.get(k, 0.0), v)
    bad = LR.violations(got, ref) + LR.rms_violations(got, ref)
    assert not bad, "%s: %s" % (what, bad)
    return rt


def both(dev, case, ref, mis=(), red='i', stored=True, rowkl=True, what=""):
    """forward, then backward from the reference's fp32 zargs, each against the reference"""
    inp = inputs(dev, case, mis)
    st, f = run_fwd(dev, case, inp, mis, rowkl)
    assert st == 0 and (f['rowkl'] is not None) == rowkl
    st, b = run_bwd(dev, case, ref['zargs32'], inp, mis, red, stored)
    assert st == 0 and (b['dzargs'] is not None) == stored
    got = dict(f, **b)
    rt = check(case, got, ref, what)
    assert set(rt) == set(LR.OUTPUTS) - ({'rowkl'} if not rowkl else set()) - ({'dzargs'} if not stored else set())
    return got


_IDS = ["%d-%d-%d-%d-%s-%s-%s-%s-%s" % (c[0], c[1], c[2], c[3], 'wide' if c[4] else 'plain', c[5], 'dz' if c[6] else 'nodz',
                                       'kl' if c[7] else 'nokl', 'mis' if c[8] else 'al') for c in LR.GPU_CASES]


@pytest.mark.parametrize("R,L,ldz,lddz,wide,red,stored,rowkl,mis", LR.GPU_CASES, ids=_IDS)
def test_latent_head_matches_the_reference(dev, R, L, ldz, lddz, wide, red, stored, rowkl, mis):
    case = LR.gpu_case(R, L, ldz, lddz, wide)
    ref = LR.ref_case(case)
    both(dev, case, ref, MISALIGNABLE if mis else (), red, stored, rowkl, "case")


@pytest.mark.parametrize("L,kl_zero,mis", [(9, False, False), (9, True, True), (17, False, True), (17, True, False), (1, False, False)])
def test_latent_head_edges(dev, L, kl_zero, mis):
    """log_var = 40 hs[r, 0] over -40 .. 40 (sd^2 from 4e-18 to 2e17), a head column with mean = 0 exactly and log_var = -40,
    rows with eps = 0, rows with dZ = 0, kl_scale = 0"""
    case = LR.edge_case(L, kl_zero, ldz=L + 3, lddz=L + 8)
    ref = LR.ref_case(case)
    got = both(dev, case, ref, MISALIGNABLE if mis else (), 'd', True, True, "edges kl_zero=%s" % kl_zero)
    assert np.array_equal(got['zargs'][:, L], ref['zargs32'][:, L])                # ONE product 40 hs[r, 0], exact in fp32 or rounded once
    assert np.array_equal(got['Z'][:20], got['zargs'][:20, :L])                    # eps = 0: the sample is the mean, bit for bit
    if L >= 2:
        assert (got['zargs'][:, 1] == 0).all() and (got['zargs'][:, L + 1] == -LR.EDGE_LV).all()
        assert (got['dzargs'][10:40, 1] == 0).all()                                # mean = 0 and dZ = 0
    if kl_zero:
        assert (got['dzargs'][10:40] == 0).all()


@pytest.mark.parametrize("R,L", [(128 * 2 + 5, 12), (128 * 2 + 5, 20)])
def test_latent_head_chained(dev, R, L):
    """a training step: the backward pass takes the DEVICE's zargs; the reference then takes those as its exact input"""
    case = LR.make_case(R + L, R, L, wide=True, ldz=L + 8, lddz=L)
    inp = inputs(dev, case)
    st, f = run_fwd(dev, case, inp)
    assert st == 0
    ref = LR.ref_case(case, zargs=f['zargs'])
    st, b = run_bwd(dev, case, f['zargs'], inp, red='d')
    assert st == 0
    check(case, dict(f, **b), ref, "chained")


@pytest.mark.parametrize("name", MISALIGNABLE)
@pytest.mark.parametrize("L", [9, 17])
def test_latent_head_each_pointer_misaligned_alone(dev, L, name):
    case = LR.make_case(500 + L, 129, L, ldz=L + 3, lddz=L + 3)
    both(dev, case, _ref129(case, L), (name,), 'i', True, True, name + " misaligned")


_REF129 = {}


def _ref129(case, L):
    if L not in _REF129:
        _REF129[L] = LR.ref_case(case)
    return _REF129[L]


@pytest.mark.parametrize("R,L", [(300, 9), (300, 24), (128 * 256 + 1, 17), (77, 16)])
def test_latent_head_bitwise_properties(dev, R, L):
    """two launches; immediate against deferred reduction (include/clvae.h: a fixed summation order); dzargs NULL against
    stored; rowkl NULL against present; R <= 128, deferred: run_bwd asserts that the job comes back all zero and the
    gradients are complete after the call"""
    case = LR.make_case(R * 3 + L, R, L, wide=True, ldz=L + 3, lddz=L + 8)
    inp = inputs(dev, case)
    _, f1 = run_fwd(dev, case, inp)
    _, f2 = run_fwd(dev, case, inp)
    _, f3 = run_fwd(dev, case, inp, rowkl=False)
    for k in LR.FWD:
        assert np.array_equal(f1[k], f2[k]), k
    assert f3['rowkl'] is None and np.array_equal(f1['zargs'], f3['zargs']) and np.array_equal(f1['Z'], f3['Z'])
    assert not np.isnan(f1['zargs']).any()
    b = [run_bwd(dev, case, f1['zargs'], inp, red=red, stored=stored)[1]
         for red, stored in (('i', True), ('i', True), ('d', True), ('i', False), ('d', False))]
    for k in LR.BWD:
        assert not np.isnan(b[0][k]).any(), k
        for i, other in enumerate(b[1:]):
            if other[k] is not None:
                assert np.array_equal(b[0][k], other[k]), (k, i + 1)
    assert b[3]['dzargs'] is None and b[4]['dzargs'] is None


# ---- noise drawn in the kernel ----
SEED, STREAM, STEP = 0x1234567890AB, 7, 3
FIRSTS = (0, 4, 6, 4096 * 32, (1 << 33) + 8)


def _drawn(dev, case, first, use_dev, rowkl):
    """a drawing launch; eps against clv_philox_normal (bit for bit), oracle/philox.py (2e-5) and the same launch fed that eps"""
    from clvae_amd import ops
    R, L = case['R'], case['L']
    it = torch.tensor([2], dtype=torch.int32, device=dev) if use_dev else None       # the device step counter is added to `step`
    st, d = run_fwd(dev, case, rowkl=rowkl, noise=(SEED, STREAM, STEP - (2 if use_dev else 0), first, it))
    assert st == 0
    want = torch.empty(R * L, dtype=torch.float32, device=dev)
    ops.philox_normal(want, R * L, SEED, STEP, STREAM, first)
    torch.cuda.synchronize()
    assert torch.equal(want.view(R, L), d['_t']['eps'].v), "eps differs from clv_philox_normal"
    return d


@pytest.mark.parametrize("L", list(range(1, 33)))
def test_latent_head_draws_its_noise(dev, L):
    """R = 77 (ragged), every L, first in FIRSTS: multiples of 4 take the quad-shared path when L is one too, the others one
    call per element; an index beyond 2^32; step + a device step counter or step alone; rowkl present or NULL"""
    R = 77
    base = LR.make_case(900 + L, R, L, ldz=L + 3)
    for i, first in enumerate(FIRSTS):
        rowkl, use_dev = (i + L) % 2 == 0, (i + L // 2) % 2 == 0
        d = _drawn(dev, base, first, use_dev, rowkl)
        ora = OP.normal(R * L, SEED, step=STEP, stream_id=STREAM, first_index=first).reshape(R, L)
        np.testing.assert_allclose(d['eps'], ora, atol=2e-5, rtol=0)           # (the oracle's libm differs from the device's in the last bits)
        case = dict(base, eps=d['eps'])
        st, f = run_fwd(dev, case, rowkl=rowkl)                                 # the same launch fed that eps
        assert st == 0
        for k in LR.FWD:
            assert (d[k] is None and f[k] is None) or np.array_equal(d[k], f[k]), (k, first)
        ref = LR.ref_case(case, backward=False)
        check(case, {k: d[k] for k in LR.FWD}, ref, "drawn first=%d" % first)


@pytest.mark.parametrize("L,first", [(32, 4096 * 32), (17, 6)])
def test_latent_head_draws_its_noise_over_the_grid(dev, L, first):
    """R = 128 * 256 + 1: workgroup 0 draws for a second block of one row"""
    R = LR.BLOCK * LR.GRID + 1
    base = LR.make_case(1900 + L, R, L, ldz=L)
    d = _drawn(dev, base, first, True, True)
    case = dict(base, eps=d['eps'])
    st, f = run_fwd(dev, case)
    assert st == 0
    for k in LR.FWD:
        assert np.array_equal(d[k], f[k]), k
    check(case, {k: d[k] for k in LR.FWD}, LR.ref_case(case, backward=False), "drawn over the grid")
    tail = OP.normal(2 * L, SEED, step=STEP, stream_id=STREAM, first_index=first + (R - 2) * L).reshape(2, L)
    np.testing.assert_allclose(d['eps'][-2:], tail, atol=2e-5, rtol=0)


# ---- refusals ----
def test_latent_head_refusals(dev):
    """CLV_EINVAL / CLV_EWORKSPACE with nothing launched: run_fwd / run_bwd assert that the profiler saw no scope of the
    kernel, that every output still holds NaN and that the deferred job is all zero"""
    from clvae_amd import _lib
    case = LR.make_case(1, 129, 9, ldz=12, lddz=12)
    za = LR.f32(LR.forward_values(LR.A64, case['hs'], case['Wz'], case['bz'], case['eps'])['zargs'])
    need = _lib.lib().clv_latent_head_bwd_workspace_bytes(129, 9)
    keep = []

    def hs_off(dev):
        keep.append(inputs(dev, case)['hs'])
        return Ct.c_void_p(keep[-1].v.data_ptr() + 4)
    for kw in (dict(H=87), dict(H=96), dict(L=0), dict(L=33), dict(R=0), dict(R=-1), dict(ldz=8), dict(hs=None), dict(Wz=None),
               dict(bz=None), dict(eps=None), dict(zargs=None), dict(Z=None), dict(hs=hs_off(dev))):
        assert run_fwd(dev, case, **kw)[0] == EINVAL, kw
    for kw in (dict(H=87), dict(L=0), dict(L=33), dict(R=0), dict(R=-5), dict(lddz=8), dict(hs=None), dict(Wz=None), dict(zargs=None),
               dict(eps=None), dict(dZ=None), dict(dhs=None), dict(dWz=None), dict(dbz=None), dict(hs=hs_off(dev))):
        for red in 'id':
            assert run_bwd(dev, case, za, red=red, **kw)[0] == EINVAL, kw
    for red in 'id':
        assert run_bwd(dev, case, za, red=red, ws=None)[0] == EWORKSPACE
        assert run_bwd(dev, case, za, red=red, ws_bytes=need - 4)[0] == EWORKSPACE
    assert _lib.lib().clv_latent_head_supported(88, 32) == 1 and _lib.lib().clv_latent_head_supported(88, 33) == 0
    assert _lib.lib().clv_latent_head_bwd_workspace_bytes(0, 9) == 0
    st, _ = run_fwd(dev, case)                                  # the same buffers' shapes do run
    assert st == 0
    assert run_bwd(dev, case, za, red='d')[0] == 0
