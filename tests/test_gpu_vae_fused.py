"""-m gpu: clv_vae_fused_step (csrc/vae_fused.hip) called directly, every output against the fp64 reference of
tests/vae_reference.py: each element of logits, w_out, wargs_out, zargs_out, rownll, rowkl, rowloss (kl_w, w_rec) and of the
12 gradient tensors within its own bound; hit exactly outside near-tie rows; loss_means against the fp64 mean of the kernel's
own rows.  Every output is NaN-filled with a canary tail; the flat parameter buffer holds the tensors in an order of the
test's own with NaN gaps between them (a read outside a tensor shows up), the flat gradient buffer the same layout with
canaries in the gaps.

Cases (B, D, H, Hc, C, L, use_x_prev): all four kernel instances (KS 24 / 32 x fp32 / bf16) -- the launcher takes KS = 24 iff
C + (use_x_prev ? D : 0) + L <= 96 and D + C <= 96, both sides of each condition --, widths 1 .. 96 off multiples of 4 and 16,
C 2 .. 16, L 1 .. 16, B 1 / 15 / 16 / 17 / 33 / 512 / 3001, a separate target, need_grads = 0 without labels, logits = NULL,
the in-kernel draw, bump_iterations, logits past both clip points, a w_rec row in its clip, exact ties in w and onehot.
The worst error / bound per output and mode and the flagged elements are printed at the end of the module (run with -s)."""
import ctypes as Ct

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import vae_reference as VR
from helpers import Bufs, CANARY

pytestmark = pytest.mark.gpu

_REPORT = dict(ratios={}, flags={}, bf16_bar={}, calls=0)


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    yield torch.device("cuda:0")
    r = _REPORT
    for mode in sorted(r['ratios']):
        print("\nvae fused %s: worst error / bound: %s" % (mode, ", ".join("%s %.3g" % kv for kv in sorted(r['ratios'][mode].items()))))
    print("vae fused: %d calls; flagged elements: %s" % (r['calls'], ", ".join("%s %d" % kv for kv in sorted(r['flags'].items()))))
    print("vae fused bf16: per-element bound / (10 %% of the tensor's largest entry), median and max: %s" %
          ", ".join("%s %.3g / %.3g" % (k, np.median(v), np.max(v)) for k, v in sorted(r['bf16_bar'].items())))


def T(a, dev, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device=dev)


def N(t):
    return t.detach().cpu().numpy().astype(np.float64)


P_ORDER = [7, 2, 11, 0, 9, 4, 1, 10, 5, 8, 3, 6]      # the tensors' placement in the flat buffers, with gaps in front
P_GAPS = [5, 1, 3, 2, 7, 1, 6, 3, 1, 2, 9, 4]


def step(dev, case, bf16=False, need_grads=True, logits=True, draw=None, means=True, bump=True, ws_bytes=None):
    """one clv_vae_fused_step with every argument under the test's control.  Returns (status, outputs, buffers)."""
    from clvae_amd import _lib, ops
    p_ = ops._ptr
    B, D = case['x'].shape
    C1, L = case['P'][2].shape[1] // 2, case['P'][6].shape[1] // 2
    C, H, Hc = C1 + 1, case['P'][4].shape[1], case['P'][0].shape[1]
    uxp = case['use_x_prev']
    shp = VR.shapes(D, H, Hc, C, L, uxp)
    offs, n = VR.layout(shp, P_ORDER, P_GAPS)
    bufs = Bufs(dev)
    params = T(VR.scatter(case['P'], offs, n, fill=np.nan), dev)
    gm = torch.as_tensor(VR.gap_mask(offs, shp, n), device=dev)
    graw = torch.full((n + 64,), CANARY, dtype=torch.float32, device=dev)
    grads = graw[:n]
    grads[~gm] = float('nan')
    o = dict(w=bufs.out(B, C), wargs=bufs.out(B, 2 * C1), zargs=bufs.out(B, 2 * L), rownll=bufs.out(B), rowkl=bufs.out(B),
             rowloss=bufs.out(B, 3))
    o['logits'] = bufs.out(B, D) if logits else None
    eps_w, eps_z = bufs.inp(case['eps_w']), bufs.inp(case['eps_z'])
    need = _lib.lib().clv_vae_fused_workspace_bytes(B, D, H, Hc, C, L, int(uxp))
    ws = torch.full(((need if ws_bytes is None else max(ws_bytes, 4)) // 4 + 64,), 7.0, dtype=torch.float32, device=dev)
    opts = _lib.VaeStepOpts()
    opts.bf16 = int(bf16)
    lm = bufs.out(5) if means else None
    opts.loss_means = p_(lm)
    it = torch.full((2,), 41, dtype=torch.int32, device=dev)
    if bump:
        opts.bump_iterations = p_(it)
    if draw is not None:
        opts.draw, opts.noise_seed, opts.stream_w, opts.stream_z, opts.first_w, opts.first_z, opts.step = 1, *draw
        opts.step_dev = p_(it)
    x, xp = T(case['x'], dev), T(case['xp'], dev)
    tgt = T(case['target'], dev) if case['target'] is not None else None
    oh = T(case['onehot'], dev) if case['onehot'] is not None else None
    offs_c = np.ascontiguousarray(offs, np.int64)
    st = _lib.lib().clv_vae_fused_step(
        B, D, H, Hc, C, L, int(uxp), p_(x), p_(xp), p_(tgt), p_(oh), None, p_(eps_w), p_(eps_z),
        p_(params), offs_c.ctypes.data_as(Ct.c_void_p), n, float(case['prior']), float(case['class_weight']),
        float(case['kl_weight']), float(case['w_kl_weight']), int(need_grads), p_(grads), p_(ws),
        need if ws_bytes is None else ws_bytes, p_(o['logits']), p_(o['w']), p_(o['wargs']), p_(o['zargs']), p_(o['rownll']),
        p_(o['rowkl']), p_(o['rowloss']), Ct.byref(opts), ops._stream())
    torch.cuda.synchronize()
    _REPORT['calls'] += 1
    got = {k: N(v) for k, v in o.items() if v is not None}
    got['grads'] = VR.gather(N(grads), offs, shp)
    got['eps_w'], got['eps_z'] = N(eps_w), N(eps_z)
    got['means'] = N(lm) if means else None
    got['iterations'] = it.cpu().numpy()
    got['ws_untouched'] = bool((ws == 7.0).all())
    bufs.check_canaries()
    g = graw.cpu().numpy()
    assert (g[n:] == CANARY).all(), "write behind the gradient buffer"
    assert (g[:n][gm.cpu().numpy()] == CANARY).all(), "write into a gap between gradient tensors"
    return st, got


def check(dev, case, mode, got, need_grads=True):
    """every output against the reference; records the ratios and flags"""
    c = dict(case, eps_w=got['eps_w'], eps_z=got['eps_z'])       # the draw: the reference consumes what the kernel wrote
    ref = VR.call(VR.reference, c, need_grads=need_grads, bf16_mode=(mode == 'bf16'))
    g = dict(got) if need_grads else {k: v for k, v in got.items() if k != 'grads'}
    bad = VR.violations(g, ref)
    assert not bad, "%s: %s" % (mode, bad)
    rt = VR.ratios(g, ref)
    agg = _REPORT['ratios'].setdefault(mode, {})
    for k, v in rt.items():
        agg[k] = max(agg.get(k, 0.0), v)
    for k, v in VR.flag_counts(ref).items():
        _REPORT['flags'][k] = _REPORT['flags'].get(k, 0) + v
    if mode == 'bf16' and need_grads:
        for nm, b, r in zip(VR.NAMES, ref['b_grads'], ref['grads']):
            if np.abs(r).max() > 0:
                _REPORT['bf16_bar'].setdefault(nm, []).append(float(np.median(b) / (0.1 * np.abs(r).max())))
    # the loss means of the slab-sum launch against the fp64 mean of the kernel's own rows
    if got['means'] is not None:
        rows = [got['rownll'], got['rowkl'], got['rowloss'][:, 0], got['rowloss'][:, 1], got['rowloss'][:, 2]]
        B = len(rows[0])
        for k, (m, r) in enumerate(zip(got['means'], rows)):
            bound = VR.KAPPA * VR.U * (np.abs(r).sum() * np.sqrt((B + 2) / 3.0) + 2 * np.abs(r.mean()) * B) / B
            assert abs(m - r.mean()) <= bound, (VR.LOSS_COLS[k], m, r.mean(), bound)
    return ref


def k24(D, C, L, uxp):
    return C + (D if uxp else 0) + L <= 96 and D + C <= 96


# (B, D, H, Hc, C, L, use_x_prev, target)
CASES = [
    (1, 88, 88, 88, 2, 4, False, False),        # KS 24
    (15, 88, 88, 88, 2, 4, True, False),        # config 1/2 shape: C + D + L = 94
    (16, 78, 40, 33, 2, 16, True, True),        # C + xo + L = 96 -> KS 24
    (17, 79, 40, 33, 2, 16, True, True),        # C + xo + L = 97 -> KS 32
    (33, 90, 52, 61, 6, 3, False, False),       # D + C = 96 -> KS 24
    (33, 91, 52, 61, 6, 3, False, True),        # D + C = 97 -> KS 32
    (17, 1, 3, 5, 2, 1, False, False),          # the narrowest
    (33, 37, 45, 21, 16, 16, True, True),       # C = L = 16
    (40, 94, 90, 70, 16, 16, False, True),      # KS 32, ragged tiles everywhere
    (512, 96, 96, 96, 9, 7, False, False),      # widest, 32 workgroups
    (3001, 88, 88, 88, 2, 4, True, False),      # many slabs, ragged last workgroup (9 rows)
]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("shape", CASES)
def test_vae_fused_step_matches_the_reference(dev, shape, bf16):
    B, D, H, Hc, C, L, uxp, tgt = shape
    case = VR.make_case(1000 * C + B + D, B, D, H, Hc, C, L, uxp, target=tgt)
    st, got = step(dev, case, bf16=bf16)
    assert st == 0
    check(dev, case, 'bf16' if bf16 else 'fp32', got)
    assert got['iterations'][0] == 42 and got['iterations'][1] == 41        # bump_iterations: once


def test_the_cases_cover_all_four_instances():
    ks = {k24(D, C, L, uxp) for (B, D, H, Hc, C, L, uxp, t) in CASES}
    assert ks == {True, False}
    sides = {(C + (D if uxp else 0) + L, D + C) for (B, D, H, Hc, C, L, uxp, t) in CASES}
    assert any(a == 96 for a, _ in sides) and any(a == 97 for a, _ in sides)
    assert any(b == 96 for _, b in sides) and any(b == 97 for _, b in sides)


@pytest.mark.parametrize("bf16", [False, True])
def test_vae_fused_step_edges(dev, bf16):
    """logits past both clip points, a w_rec row in the lower clip, exact ties in w and in onehot (first index)"""
    case = VR.edge_case()
    st, got = step(dev, case, bf16=bf16)
    assert st == 0
    ref = check(dev, case, 'bf16' if bf16 else 'fp32', got)
    assert (got['grads'][11][:2] == 0).all()                     # no gradient through a clipped logit
    assert got['rowloss'][2, 2] == 0 and ref['rowloss'][2, 2] == 0
    np.testing.assert_array_equal(got['w'][2], np.full(5, np.float32(0.2)))


@pytest.mark.parametrize("bf16", [False, True])
def test_vae_fused_step_forward_only_without_labels(dev, bf16):
    """need_grads = 0, onehot = NULL: hit = w_rec = 0; grads, ws and the counter untouched; logits = NULL is allowed"""
    case = dict(VR.make_case(9, 45, 30, 26, 19, 4, 5, True), onehot=None)
    st, got = step(dev, case, bf16=bf16, need_grads=False, logits=False)
    assert st == 0
    check(dev, case, 'bf16' if bf16 else 'fp32', got, need_grads=False)
    assert (got['rowloss'][:, 1:] == 0).all()
    assert all(np.isnan(g).all() for g in got['grads'])
    assert got['ws_untouched'] and got['iterations'][0] == 41


def test_vae_fused_step_logits_null_with_gradients(dev):
    case = VR.make_case(4, 20, 21, 13, 11, 3, 2, False, target=True)
    st, got = step(dev, case, logits=False)
    assert st == 0
    check(dev, case, 'fp32', got)


@pytest.mark.parametrize("bf16", [False, True])
def test_vae_fused_step_draws_its_noise(dev, bf16):
    """opts.draw: the reference consumes the eps the kernel wrote (their bits are pinned by test_gpu_models.py)"""
    case = VR.make_case(6, 37, 50, 40, 30, 7, 5, True)
    case = dict(case, eps_w=np.zeros_like(case['eps_w']), eps_z=np.zeros_like(case['eps_z']))
    st, got = step(dev, case, bf16=bf16, draw=(0x5eed1234abcd, 3, 4, 17, 29, 2))
    assert st == 0
    assert np.isfinite(got['eps_w']).all() and np.abs(got['eps_w']).max() > 0 and np.abs(got['eps_z']).max() > 0
    check(dev, case, 'bf16' if bf16 else 'fp32', got)


@pytest.mark.parametrize("bf16", [False, True])
def test_vae_fused_step_is_deterministic(dev, bf16):
    """two identical calls: bit-identical outputs (the slab sum runs in a fixed order)"""
    case = VR.make_case(8, 300, 88, 88, 88, 2, 4, True)
    _, a = step(dev, case, bf16=bf16)
    _, b = step(dev, case, bf16=bf16)
    for k in ('logits', 'w', 'wargs', 'zargs', 'rownll', 'rowkl', 'rowloss', 'means'):
        assert np.array_equal(a[k], b[k]), k
    for x, y in zip(a['grads'], b['grads']):
        assert np.array_equal(x, y)


def test_vae_fused_step_argument_errors(dev):
    from clvae_amd import _lib
    case = VR.make_case(2, 40, 24, 20, 16, 3, 2, True)
    need = _lib.lib().clv_vae_fused_workspace_bytes(40, 24, 20, 16, 3, 2, 1)
    st, got = step(dev, case, ws_bytes=need - 4)
    assert st == -2                                              # CLV_EWORKSPACE
    st, got = step(dev, dict(case, onehot=None))
    assert st == -1                                              # CLV_EINVAL: need_grads without onehot
