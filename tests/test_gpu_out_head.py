"""-m gpu: clv_out_head_train (csrc/out_head.hip, csrc/out_head_bf16.hip) called directly, BOTH kernels, every output against
the fp64 reference of tests/out_head_reference.py: each element of logits, rownll, dlogits, dhs, dWo, dbo within its own
bound, every tensor of at least 1000 elements with rms(err / sigma) <= 1, and on the single-product cases every product
within the worst-case bound that tells 6 of 9 bf16 piece pairs from 5.

Which kernel ran is asserted from the profiler's scope name ('out_head_bf16' / 'out_head_train'), never assumed.  The f32-MFMA
kernel is selected by what makes the launcher's out_head_bf16_ok() false -- not by CLV_OUT_HEAD_F32, which is read once
per process: a float target array of pitch 89 or 91 (`how` = 'ldy'), or the Y / dhs / logits / dlogits pointer one float past
a 16-byte boundary (`how` names the pointer).  Whether the engine ever reaches that kernel in practice has not been
measured; this module covers the launcher's rule.

Buffers: every output NaN-filled (helpers.Bufs) with a canary tail and, in front of a misaligned view, NaN that must stay;
dWo and dbo are views into one flat buffer at offsets 8 and 7764 floats with canaries in front, between and behind; the
workspace is exactly clv_out_head_train_workspace_bytes(R) plus a canary tail; the padding columns of a target array of
pitch > 88 hold NaN (bytes: 0xA5).  Cases: out_head_reference.GPU_CASES (R 1 .. 128 * 513 + 7 around the tile, block and grid
boundaries, target pitches, stored outputs, scales, immediate and deferred reduction), byte targets, the clip-point edge
case, the single-product cases, determinism, the host's argument checks.  Every GPU call is an ordinary in-bounds launch.
NOT exercised: the 2 GiB limit of the bf16 kernel's buffer descriptors (widest < 0x80000000, about 6.1 M rows): it would need
several arrays of over 2 GB and minutes of fp64 on the host.
The worst error / bound and rms per output and kernel and the flag counts are printed at the end of the module (-s)."""
import ctypes as Ct

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import out_head_reference as OR
from helpers import Bufs, CANARY, TAIL

pytestmark = pytest.mark.gpu

SCOPE = {'bf16': 'out_head_bf16', 'f32': 'out_head_train'}
EINVAL, EWORKSPACE = -1, -2
_REPORT = dict(ratios={}, rms={}, single={}, flags={}, calls={})
DWO_OFF, DBO_OFF, G_LEN = 8, 8 + 88 * 88 + 12, 8 + 88 * 88 + 12 + 88          # both multiples of four floats


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    yield torch.device("cuda:0")
    r = _REPORT
    for scope in sorted(r['ratios']):
        print("\n%s (%d calls): worst error / bound: %s" % (scope, r['calls'][scope], ", ".join("%s %.3g" % kv for kv in r['ratios'][scope].items())))
        print("%s: worst rms(err / sigma): %s" % (scope, ", ".join("%s %.3g" % kv for kv in r['rms'][scope].items())))
        if scope in r['single']:
            print("%s: single products, worst error / bound: %s" % (scope, ", ".join("%s %.3g" % kv for kv in r['single'][scope].items())))
    print("out head: flagged elements: %s" % ", ".join("%s %d" % kv for kv in sorted(r['flags'].items())))


def T(a, dev, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def N(t):
    return None if t is None else t.detach().cpu().numpy().astype(np.float64)


def run(dev, case, how=None, stored='both', red='i', u8=False, y_off=0, ws_short=0, expect=None, **override):
    """one clv_out_head_train with every pointer, pitch and size under the test's control.  Returns (status, outputs);
    asserts the canaries, the deferred job's state and, with `expect`, the kernel that ran."""
    from clvae_amd import _lib, ops
    p_ = ops._ptr
    L = _lib.lib()
    R, ldy = case['hs'].shape[0], case['ldy']
    bufs = Bufs(dev)
    hs, Wo, bo = T(case['hs'], dev), T(case['Wo'], dev), T(case['bo'], dev)
    if u8:
        Yb = np.full((R, ldy), 0xA5, np.uint8)
        Yb[:, :88] = case['Y']
        yraw = torch.full((R * ldy + 16,), 0xA5, dtype=torch.uint8, device=dev)
        yraw[y_off:y_off + R * ldy] = torch.as_tensor(Yb.reshape(-1), device=dev)
        Y = yraw[y_off:]
    else:
        off = 1 if how == 'Y' else 0
        yraw = torch.full((R * ldy + 4,), float('nan'), dtype=torch.float32, device=dev)
        yraw[off:off + R * ldy] = T(case['Ypad'].reshape(-1), dev)
        Y = yraw[off:]
    fronts = []

    def out(name, *shape):
        """a NaN-filled output; `how` == name: one float past a 16-byte boundary, the float in front must stay NaN"""
        n = int(np.prod(shape))
        flat = bufs.out(n + 4)
        mis = 1 if how == name else 0
        fronts.append((name, flat, mis, n))
        v = flat[mis:mis + n].view(*shape)
        assert v.data_ptr() % 16 == 4 * mis
        return v
    o = dict(rownll=out('rownll', R), dhs=out('dhs', R, 88))
    o['logits'] = out('logits', R, 88) if stored in ('both', 'logits') else None
    o['dl'] = out('dlogits', R, 88) if stored in ('both', 'dlogits') else None
    G = torch.full((G_LEN + TAIL,), CANARY, dtype=torch.float32, device=dev)
    dWo, dbo = G[DWO_OFF:DWO_OFF + 88 * 88].view(88, 88), G[DBO_OFF:DBO_OFF + 88]
    dWo.fill_(float('nan'))
    dbo.fill_(float('nan'))
    need = L.clv_out_head_train_workspace_bytes(R)
    assert need % 4 == 0 and need > 0
    ws = torch.full((need // 4 + TAIL,), CANARY, dtype=torch.float32, device=dev)
    rq = ops.ReduceQueue(dev) if red == 'd' else None
    job = rq.next_job() if rq is not None else None
    a = dict(R=R, H=88, D=88, hs=p_(hs), Wo=p_(Wo), bo=p_(bo), Y=p_(Y), ldy=ldy, rownll=p_(o['rownll']), ws_bytes=need - ws_short)
    a.update(override)
    ops.prof_enable(True)
    try:
        st = L.clv_out_head_train(a['R'], a['H'], a['D'], a['hs'], a['Wo'], a['bo'], a['Y'], int(u8), a['ldy'], float(case['scale']),
                                  p_(o['logits']), a['rownll'], p_(o['dl']), p_(o['dhs']), p_(dWo), p_(dbo), p_(ws), a['ws_bytes'],
                                  job, ops._stream())
        torch.cuda.synchronize()
        names = [n for n, _, _ in ops.prof_collect()]
    finally:
        ops.prof_enable(False)          # process-wide: no other module sees it on
    ran = [k for k, s in SCOPE.items() if s in names]
    if st != 0:
        assert not ran, "a kernel was launched although the call failed"
        return st, None
    if expect is not None:
        assert ran == [expect], "expected the %s kernel, the profiler saw %s" % (expect, names)
    if rq is not None:
        empty = not any(bytes(rq.jobs[0].opaque))
        if R <= 128:         # a single slab is reduced at once: the job comes back empty, the gradients are complete
            assert empty and not torch.isnan(dWo).any() and not torch.isnan(dbo).any()
        else:
            assert not empty and torch.isnan(dWo).all() and torch.isnan(dbo).all()
        rq.flush()
        torch.cuda.synchronize()
    got = {k: N(v) for k, v in o.items()}
    got['dWo'], got['dbo'] = N(dWo), N(dbo)
    bufs.check_canaries()
    for name, flat, mis, n in fronts:
        f = flat.cpu().numpy()
        assert np.isnan(f[:mis]).all() and np.isnan(f[mis + n:]).all(), "write beside " + name
    g = G.cpu().numpy()
    gap = np.ones(G_LEN + TAIL, bool)
    gap[DWO_OFF:DWO_OFF + 88 * 88] = gap[DBO_OFF:DBO_OFF + 88] = False
    assert (g[gap] == CANARY).all(), "write beside dWo / dbo in the flat gradient buffer"
    assert (ws[need // 4:] == CANARY).all(), "write behind the workspace"
    _REPORT['calls'][SCOPE[ran[0]]] = _REPORT['calls'].get(SCOPE[ran[0]], 0) + 1
    return st, got


_REF = {}


def reference(case, key, kernel):
    """the reference of a case, the last one kept (the same case runs on both kernels and with both reductions)"""
    if key not in _REF:
        _REF.clear()
        _REF[key] = {}
    if kernel not in _REF[key]:
        values = next(iter(_REF[key].values()))['values'] if _REF[key] else None
        _REF[key][kernel] = OR.ref_case(case, dropped=(kernel == 'bf16'), values=values)
    return _REF[key][kernel]


def check(case, kernel, got, ref, exempt_flags=False):
    """every element against its bound, every tensor against the rms criterion; records the figures"""
    rt, rm = OR.ratios(got, ref), OR.rms(got, ref)
    print("%s R=%d ldy=%d: error / bound %s | rms %s" % (SCOPE[kernel], case['hs'].shape[0], case['ldy'],
          " ".join("%s %.3g" % kv for kv in rt.items()), " ".join("%s %.3g" % kv for kv in rm.items())))
    for name, d in (('ratios', rt), ('rms', rm)):
        agg = _REPORT[name].setdefault(SCOPE[kernel], {})
        for k, v in d.items():
            agg[k] = max(agg.get(k, 0.0), v)
    for k, v in OR.flag_counts(ref).items():
        _REPORT['flags'][k] = _REPORT['flags'].get(k, 0) + v
    bad = [(k, v) for k, v in rt.items() if not v <= 1.0] + \
        [('rms ' + k, v) for k, v in rm.items() if np.size(ref[k]) >= OR.RMS_MIN and not v <= 1.0]       # violations + rms_violations
    assert not bad, "%s: %s" % (SCOPE[kernel], bad)
    if not exempt_flags:
        assert OR.flag_counts(ref)['clip_l'] <= 1e-4 * ref['logits'].size


@pytest.mark.parametrize("R,kernel,how,ldy,stored,scale,reds", OR.GPU_CASES,
                         ids=["%d-%s-%s-%d-%s-%s-%s" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6]) for c in OR.GPU_CASES])
def test_out_head_matches_the_reference(dev, R, kernel, how, ldy, stored, scale, reds):
    case = OR.gpu_case(R, ldy, scale)
    ref = reference(case, (R, scale), kernel)
    for red in reds:
        st, got = run(dev, case, how=how, stored=stored, red=red, expect=kernel)
        assert st == 0
        assert (got['logits'] is not None) == (stored in ('both', 'logits')) and (got['dl'] is not None) == (stored in ('both', 'dlogits'))
        check(case, kernel, got, ref)


@pytest.mark.parametrize("R,ldy,y_off,red", [(200, 88, 0, 'i'), (129, 92, 4, 'd'), (1000, 96, 0, 'd'), (17, 96, 4, 'i')])
def test_out_head_byte_targets(dev, R, ldy, y_off, red):
    """uint8 frames (the bf16 kernel only), padding 0xA5, Y 16-byte aligned or four bytes past: against the reference, and bit
    for bit the float-target run of the same pitch"""
    case = OR.gpu_case(R, ldy, None)
    ref = reference(case, (R, None), 'bf16')
    st, gf = run(dev, case, red=red, expect='bf16')
    assert st == 0
    st, gb = run(dev, case, red=red, u8=True, y_off=y_off, expect='bf16')
    assert st == 0
    check(case, 'bf16', gb, ref)
    for k in OR.OUTPUTS:
        assert np.array_equal(gf[k], gb[k]), k


@pytest.mark.parametrize("kernel,how,ldy", [('bf16', None, 92), ('f32', 'ldy', 89), ('f32', 'dlogits', 88)])
def test_out_head_edges(dev, kernel, how, ldy):
    """logits exactly on both clip points (inside), one fp32 step outside each, between the float32 clip and the symmetric one,
    far outside; hs rows of zeros and of 1e-30; a Wo column of zeros and one scaled by 30"""
    case = OR.edge_case(ldy)
    ref = OR.ref_case(case, dropped=(kernel == 'bf16'))
    st, got = run(dev, case, how=how, expect=kernel)
    assert st == 0
    check(case, kernel, got, ref, exempt_flags=True)
    c0, n = OR.EDGE_COL0, OR.EDGE_PTS.size
    assert OR.flag_counts(ref)['clip_l'] == 2 * OR.EDGE_NEAR and ref['flags']['clip_l'][:2, c0:c0 + OR.EDGE_NEAR].all()
    for row in (0, 1):       # one product 1.0 * point: exact in both kernels, so the branch taken is known
        assert np.array_equal(got['logits'][row, c0:c0 + n], OR.EDGE_PTS.astype(np.float64))
        assert np.array_equal(got['dl'][row, c0:c0 + n] == 0, ref['dl'][row, c0:c0 + n] == 0)
    assert (got['dl'][0, c0] != 0) and (got['dl'][0, c0 + 1] == 0) and (got['dl'][1, c0 + 2] != 0) and (got['dl'][1, c0 + 3] == 0)
    assert (got['logits'][2:4] == 0).all() and (got['logits'][:, OR.EDGE_ZERO_COL] == 0).all()
    assert (got['dhs'][:, 0][np.abs(ref['dhs'][:, 0]) > 0] != 0).all()


@pytest.mark.parametrize("kernel,how,ldy,R", [('bf16', None, 88, 1), ('bf16', None, 96, 200), ('f32', 'ldy', 91, 1), ('f32', 'dhs', 88, 200)])
def test_out_head_single_products(dev, kernel, how, ldy, R):
    """Wo = permutation times values, bo = 0: every logit, every dhs entry (from the stored dl) and at R = 1 every dWo entry is
    ONE product, held to out_head_reference.SINGLE; dbo == dl[0] bit for bit"""
    case = OR.single_case(R, R, ldy)
    st, got = run(dev, case, how=how, expect=kernel)
    assert st == 0
    check(case, kernel, got, OR.ref_case(case, dropped=(kernel == 'bf16')))
    sr = OR.single_ratios(case, got, kernel)
    print("%s single products R=%d: %s" % (SCOPE[kernel], R, sr))
    agg = _REPORT['single'].setdefault(SCOPE[kernel], {})
    for k, v in sr.items():
        agg[k] = max(agg.get(k, 0.0), v)
    assert not OR.single_violations(case, got, kernel), sr
    assert {'logits', 'dhs'} <= set(sr) and (R > 1 or {'dWo', 'dbo'} <= set(sr))


@pytest.mark.parametrize("kernel,how,ldy", [('bf16', None, 88), ('f32', 'ldy', 89)])
def test_out_head_is_deterministic(dev, kernel, how, ldy):
    """two identical calls: bit-identical outputs (8 slabs, summed in a fixed order)"""
    case = OR.gpu_case(1000, ldy, None)
    for red in 'id':
        _, a = run(dev, case, how=how, red=red, expect=kernel)
        _, b = run(dev, case, how=how, red=red, expect=kernel)
        for k in OR.OUTPUTS:
            assert np.array_equal(a[k], b[k]), (k, red)


def test_out_head_argument_errors(dev):
    """status only: every one of these returns before a launch (run() asserts that no kernel scope was recorded)"""
    case = OR.gpu_case(129, 88, None)
    st, _ = run(dev, case, ws_short=1)
    assert st == EWORKSPACE
    assert run(dev, case, R=0)[0] == EINVAL
    assert run(dev, case, ldy=87)[0] == EINVAL
    assert run(dev, case, H=87)[0] == EINVAL
    assert run(dev, case, rownll=None)[0] == EINVAL
    big = T(np.zeros(88 * 130 + 4), dev)
    assert run(dev, case, hs=Ct.c_void_p(big.data_ptr() + 4))[0] == EINVAL
    assert run(dev, case, Wo=Ct.c_void_p(big.data_ptr() + 4))[0] == EINVAL
    assert run(dev, OR.gpu_case(129, 90, None), u8=True)[0] == EINVAL           # byte targets: the bf16 kernel only, pitch % 4 == 0
    assert run(dev, OR.gpu_case(129, 92, None), u8=True, y_off=2)[0] == EINVAL      # ... and Y 4-byte aligned
    st, got = run(dev, case, expect='bf16')                                        # the same buffers' shapes do run
    assert st == 0
