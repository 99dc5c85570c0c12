"""-m gpu: clv_adam_wn_step (csrc/optim.hip) called directly through ctypes with plans from clv_adam_wn_plan_build, every
route, EVERY output -- params, m, v, mg, vg, s, vn2 and the counter -- against the fp64 reference of
tests/optim_reference.py: each element within its own bound, rms(err / sigma) <= 1 per tensor of at least 1000 elements.

Four steps per case and route; the reference is restarted at every step from the state read back from the device, so each
step is a one-step comparison.  The fast routes run step 1 by the chain (whose vn2 is checked against the true column sums
of the stored parameters), steps 2-4 by the two-launch known-sums form with gdot formed on the host in fp64 from the
read-back state and rounded to fp32; vn2 against the true sums after every step.  The same tables also run all-chain.
Which route a table takes follows from the launcher's rule (known.use, the number of tall matrices, cols % 4 of the tall one: the
flat float4 body or the float2 row-lane body); assert_rule holds the tables to it.  The profiler cannot tell the routes apart
(one scope, 'adam_wn_step', for all), so that the two-launch form really ran is shown by what it alone does:
test_known_sums_are_consumed hands it a gdot and a vn2 that are 1 % off, and the outputs must be those of the known-sums
reference on these inputs and beyond the bounds of the plain form, which recomputes both sums from the parameters.

Buffers: a thin layer (optim_reference.layout) mirrors FlatParams' layout, and one test asserts that both give the same
table.  Every array has a canary tail (helpers.CANARY, TAIL); the padding floats between tensors and the padding columns of
mg / vg / s / vn2 hold the same sentinel; the reference returns whole arrays with bound 0 wherever the step owns nothing,
so sentinels, `m` under RMSprop, mg / vg / s under plain Adam and RMSprop and every tensor outside an only= sub-table are
held bitwise by the same comparison.  grads are compared bitwise after every call.  The workspace is exactly
clv_adam_wn_workspace_bytes of the call's table plus a canary tail.  Refusals are argument checks on the host: every GPU
call here is an ordinary in-bounds launch.  No atomics in the file under test: same inputs, bitwise equal outputs.

Measured on an MI355X (the module's report, -s), worst error / bound over params, m, v, mg, vg, s, vn2 and worst
rms(err / sigma) over params, m, v per route:
  small        0.26 (m)   rms 0.22        chain        0.31 (v)   rms 0.42      vn2 against the true sums 0.068 of the bound
  fast, flat   0.36 (m)   rms 0.48        fast, pair   0.35 (v)   rms 0.44      vn2 against the true sums 0.055 / 0.060
  plain Adam   0.26 (v)   rms 0.44        RMSprop      0.28 (params)  rms 0.44
  fast with gdot or vn2 1 % off, against the known-sums reference on those inputs: flat 0.34 (m), pair 0.36 (v), rms 0.44
  kernel trace, once outside the suite (a chain step, then a known-sums step, 193 x 100 and 193 x 126): the five chain kernels and
  wn_fast_update_kernel + wn_fast_rescale_kernel in both, as the rule predicts (PERFLOG.md)
  lr_t by itself: worst error 0.136 of rel_lr(t) + 6 U;  insensitive elements of params': 7 in 71 chain calls, none elsewhere.
"""
import ctypes as Ct

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import optim_reference as R
from helpers import CANARY, TAIL

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -2
_REPORT = dict(ratios={}, rms={}, sums={}, calls={}, insens={}, lr=0.0)
assert CANARY == R.SENTINEL


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    L = _lib.lib()
    assert L.clv_error_string(EINVAL) and L.clv_error_string(EWORKSPACE)
    yield torch.device("cuda:0")
    r = _REPORT
    for route in sorted(r['ratios']):
        print("\n%s (%d calls): worst error / bound: %s" % (route, r['calls'][route], ", ".join("%s %.3g" % kv for kv in r['ratios'][route].items())))
        print("%s: worst rms(err / sigma): %s" % (route, ", ".join("%s %.3g" % kv for kv in r['rms'][route].items())))
        print("%s: insensitive elements of params' %d; worst |vn2 - true sums| / bound %.3g" % (route, r['insens'][route], r['sums'].get(route, 0.0)))
    print("lr_t by itself: worst error / (rel_lr(t) + 6 U) %.3g" % r['lr'])


def ctable(descs):
    from clvae_amd import _lib
    return (_lib.ParamDesc * len(descs))(*[_lib.ParamDesc(d.offset, d.rows, d.cols, d.col_offset, d.is_matrix, 0) for d in descs])


class Dev:
    """the flat arrays of one table on the device, each with a canary tail; plans per sub-table"""

    def __init__(self, dev, table, st, grads):
        self.dev, self.table = dev, table
        self.a = {}
        for k in R.OUTPUTS + ('grads',):
            h = np.asarray(grads if k == 'grads' else st[k], np.float32)
            raw = torch.full((h.size + TAIL,), CANARY, dtype=torch.float32, device=dev)
            raw[:h.size] = torch.as_tensor(h, device=dev)
            self.a[k] = raw
        self.n = {k: v.numel() - TAIL for k, v in self.a.items()}
        self.it = torch.full((1 + TAIL,), 4321, dtype=torch.int32, device=dev)
        self.it[0] = int(st['t'])
        self.gdot = None
        self.plans = {}

    def set_grads(self, g):
        self.a['grads'][:self.n['grads']] = torch.as_tensor(np.asarray(g, np.float32), device=self.dev)

    def read(self):
        torch.cuda.synchronize()
        out = {}
        for k, raw in self.a.items():
            h = raw.cpu().numpy()
            assert (h[self.n[k]:] == CANARY).all(), ("write behind", k)
            out[k] = h[:self.n[k]].copy()
        it = self.it.cpu().numpy()
        assert (it[1:] == 4321).all()
        out['t'] = int(it[0])
        if self.gdot is not None:
            assert (self.gdot.cpu().numpy()[self.gdot_n:] == CANARY).all()
        return out

    def plan(self, descs):
        from clvae_amd import _lib
        key = tuple(d.name for d in descs)
        if key not in self.plans:
            L = _lib.lib()
            tb = ctable(descs)
            blob = (Ct.c_uint8 * L.clv_adam_wn_plan_bytes(tb, len(descs)))()
            assert L.clv_adam_wn_plan_build(tb, len(descs), blob) == 0
            self.plans[key] = (tb, torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).to(self.dev))
        return self.plans[key]

    def step(self, descs, hyp, mode='advance', known=None, ws_short=0, null=(), weightnorm=None, expect=0):
        """one clv_adam_wn_step on the sub-table `descs`; known as in optim_reference.ref_step, plus 'null': names out of
        ('gdot', 'vnorm2') passed as NULL.  Asserts the status, the workspace's canary tail and that a refused call opened no
        profiler scope."""
        from clvae_amd import _lib, ops
        p_ = ops._ptr
        L = _lib.lib()
        tb, plan = self.plan(descs)
        need = L.clv_adam_wn_workspace_bytes(tb, len(descs))
        assert need > 0 and need % 4 == 0
        ws = torch.full((need // 4 + TAIL,), CANARY, dtype=torch.float32, device=self.dev)
        ks = None
        if known is not None:
            if known.get('gdot') is not None:
                gd = np.asarray(known['gdot'], np.float32)
                self.gdot = torch.full((gd.size + TAIL,), CANARY, dtype=torch.float32, device=self.dev)
                self.gdot[:gd.size] = torch.as_tensor(gd, device=self.dev)
                self.gdot_n = gd.size
            ks = _lib.AdamKnownSums(int(known['tensor']), int(bool(known.get('use'))),
                                    p_(self.gdot) if known.get('gdot') is not None and 'gdot' not in null else None,
                                    None if 'vnorm2' in null else p_(self.a['vn2']))
        it, step_t = {'advance': (self.it, 0), 'readonly': (self.it, R.STEP_READONLY), 'advanced': (self.it, R.STEP_ADVANCED)}.get(
            mode if isinstance(mode, str) else None, (None, mode[1] if isinstance(mode, tuple) else 0))
        ptr = lambda k: None if k in null else p_(self.a[k])
        ops.prof_enable(True)
        try:
            status = L.clv_adam_wn_step(tb, len(descs), p_(plan), ptr('params'), ptr('grads'), ptr('m'), ptr('v'), ptr('mg'), ptr('vg'),
                                        ptr('s'), p_(it), int(step_t), hyp['lr'], hyp['b1'], hyp['b2'], hyp['eps'],
                                        hyp['opt'] if weightnorm is None else weightnorm, Ct.byref(ks) if ks is not None else None,
                                        p_(ws), need - ws_short, ops._stream())
            torch.cuda.synchronize()
            names = [n for n, _, _ in ops.prof_collect()]
        finally:
            ops.prof_enable(False)          # process-wide: no other module sees it on
        assert status == expect, (status, expect)
        assert ('adam_wn_step' in names) == (status == 0), names
        assert (ws.cpu().numpy()[need // 4:] == CANARY).all(), "write behind the workspace"
        return status


def known_for(table, before, grads, use):
    """the known-sums argument for the table's first tall matrix; use: gdot = sum_r g W in fp64 from the read-back state,
    rounded to fp32"""
    tall = [i for i, d in enumerate(table) if R.is_tall(d)]
    if not tall:
        return None
    k = dict(tensor=tall[0], use=bool(use), gdot=None)
    if use:
        k['gdot'] = R.true_sums(before['params'], before['s'], grads, table[tall[0]])['gdot'].astype(np.float32)
    return k


def compare(route, after, before, ref, table, grads):
    """all outputs within their bounds (bound 0 where the step owns nothing), the rms criterion, the counter, grads bitwise"""
    ra, rm = R.ratios(after, ref), R.rms(after, ref, table)
    r = _REPORT
    r['calls'][route] = r['calls'].get(route, 0) + 1
    for key, new in (('ratios', ra), ('rms', rm)):
        old = r[key].setdefault(route, {})
        for k, v in new.items():
            old[k] = max(old.get(k, 0.0), v)
    r['insens'][route] = r['insens'].get(route, 0) + int(ref['insens'].sum())
    assert not R.violations(after, ref), (route, ra)
    assert not R.rms_violations(after, ref, table), (route, rm)
    assert after['t'] == (ref['counter'] if ref['counter'] is not None else before['t'])
    assert (after['grads'].view(np.uint32) == np.asarray(grads, np.float32).view(np.uint32)).all(), "grads written"


def check_sums(route, after, table, grads):
    for d in table:
        if R.is_tall(d):
            q = R.sums_ratio(after['vn2'], after['params'], after['s'], grads, d)
            _REPORT['sums'][route] = max(_REPORT['sums'].get(route, 0.0), q)
            assert q <= 1.0, (route, d.name, q)


def route_key(route, table, use):
    if route != 'fast' or not use:
        return 'chain' if route == 'fast' else route
    return 'fast-' + R.fast_body(table[R.tall_index(table)])


def assert_rule(route, table, case):
    """the launcher's rule: which kernels a call of this table takes"""
    n_big = sum(1 for d in table if R.is_tall(d))
    if route == 'small':
        assert n_big == 0
    elif route == 'chain':
        assert n_big >= 1
    elif route == 'fast':
        d = table[R.tall_index(table)]
        assert n_big == 1 and d.cols % 2 == 0 and d.cols <= 128 and d.offset % 4 == 0 and d.col_offset % 4 == 0
        assert case in R.DEGENERATE_CASES or case['name'].startswith(R.fast_body(d)), "flat: cols % 4 == 0, pair: cols % 4 == 2"


CASE_ROUTES = [(c, r) for c in R.GPU_CASES + R.DEGENERATE_CASES for r in c['routes']]
IDS = ["%s-%s" % (c['name'], r) for c, r in CASE_ROUTES]
BY_NAME = {c['name']: c for c in R.GPU_CASES + R.DEGENERATE_CASES}


def test_layout_is_flatparams(dev):
    """the layer these tests lay their buffers out with gives FlatParams' table: the direct tests stand for what the engines use"""
    from clvae_amd.engine import FlatParams
    for case in R.GPU_CASES + R.DEGENERATE_CASES:
        table, n, n_cols = R.layout(case['shapes'])
        P = FlatParams(case['shapes'], dev)
        assert (P.n, P.n_cols, len(P.shapes)) == (n, n_cols, len(table))
        for d, t in zip(table, P.table):
            assert (t.offset, t.rows, t.cols, t.col_offset, t.is_matrix) == (d.offset, d.rows, d.cols, d.col_offset, d.is_matrix)
        tall = P.tall_tensor()
        assert (tall[0] if tall else None) == R.tall_index(table)
        if case['only']:
            sub, k, _ = P._subplan(case['only'])
            assert [sub[i].offset for i in range(k)] == [d.offset for d in table if d.name in case['only']]


@pytest.mark.parametrize("case,route", CASE_ROUTES, ids=IDS)
def test_every_output_of_every_step(dev, case, route):
    """four steps, every output of every call against ref_step restarted from the device's own state"""
    degenerate = case in R.DEGENERATE_CASES
    table, n, n_cols, st = R.make_state(case, route)
    assert_rule(route, table, case)
    hyp = R.hyper(opt=R.ROUTE_OPT[route])
    wn = hyp['opt'] == R.OPT_ADAM_WN
    g, _ = R.make_grads(table, n, 500, zero=case['name'] == 'zero_gradient')
    D = Dev(dev, table, st, g)
    for step in range(4):
        g, _ = R.make_grads(table, n, 500 + step, zero=case['name'] == 'zero_gradient')
        D.set_grads(g)
        before = D.read()
        use = route == 'fast' and step > 0
        if use and case['only']:            # the fast form through a sub-table, the other tensors in a second call that advances
            sub = [d for d in table if d.name in case['only']]
            rest = [d for d in table if d.name not in case['only']]
            assert R.tall_index(sub) != R.tall_index(table)
            calls = [(sub, 'readonly', known_for(sub, before, g, True)), (rest, 'advance', None)]
        else:
            calls = [(table, 'advance', known_for(table, before, g, use) if wn else None)]
        for descs, mode, known in calls:
            ref = R.ref_step(before, g, descs, hyp, mode, known)
            D.step(descs, hyp, mode, known)
            after = D.read()
            key = route_key(route, table, use) + (' (degenerate)' if degenerate else '')
            if degenerate and case['name'] == 'one_row':
                assert all(np.isfinite(after[k]).all() for k in R.OUTPUTS)
                assert not R.violations(after, ref, ('m', 'v', 'mg', 'vg')), R.ratios(after, ref)
                assert after['t'] == ref['counter']
                assert (after['grads'].view(np.uint32) == g.view(np.uint32)).all(), "grads written"
                for k in R.OUTPUTS:             # what the step does not own (bound 0: padding, sentinels) stays bitwise
                    free = ref['b_' + k] == 0
                    assert (after[k][free].view(np.uint32) == before[k][free].view(np.uint32)).all(), k
            else:
                compare(key, after, before, ref, descs, g)
            if case['name'] == 'zero_gradient':
                for k in ('m', 'v', 'mg', 'vg'):
                    assert (after[k] == before[k]).all()
            before = after
        if wn and not degenerate:
            check_sums(route_key(route, table, use), after, table, g)
    assert after['t'] == st['t'] + 4


@pytest.mark.parametrize("opt", [R.OPT_ADAM_WN, R.OPT_ADAM])
@pytest.mark.parametrize("b2", [0.999, 0.9])
def test_lr_t_by_itself(dev, opt, b2):
    """a bias-only table, params = m = v = 0, g = 1: params' = -lr_t (1 - b1) / (sqrt(1 - b2) + eps), so the error is lr_t's own
    plus the roundings of the update itself (m', v', the square root, + eps, the division, the product: 6 U).  t through the
    counter and as explicit step_t; held to rel_lr(t) + 6 U, relative.  Under CLV_OPT_ADAM the table is the bias alone; under
    CLV_OPT_ADAM_WN a 2 x 4 matrix stands behind it, since a table without a matrix is plain Adam there too and the bias
    would never reach the small-tensor blocks."""
    table, n, n_cols = R.layout([('b/bias', (8,))] + ([('a/kernel', (2, 4))] if opt == R.OPT_ADAM_WN else []))
    mat = opt == R.OPT_ADAM_WN
    hyp = R.hyper(b2=b2, opt=opt)
    worst = 0.0
    rng = np.random.default_rng(8)
    for t in (1, 2, 3, 10, 100, 1000, 10 ** 4, 10 ** 5, 10 ** 6):
        for mode in ('advance', ('explicit', t)):
            st = {k: np.full(n, CANARY, np.float32) for k in R.FLAT}
            st.update({k: np.full(n_cols, CANARY, np.float32) for k in R.COLS})
            for k in R.FLAT:
                st[k][:n] = 0
            if mat:
                st['params'][8:16] = 0.1 * rng.standard_normal(8)
                st['mg'][:4] = st['vg'][:4] = 0
                st['s'][:4] = 1
            st['t'] = t - 1 if mode == 'advance' else 77
            g = np.full(n, CANARY, np.float32)
            g[:8] = 1
            if mat:
                g[8:16] = rng.standard_normal(8)
            D = Dev(dev, table, st, g)
            ref = R.ref_step(st, g, table, hyp, mode)
            assert ref['t'] == t
            D.step(table, hyp, mode)
            after = D.read()
            assert not R.violations(after, ref), R.ratios(after, ref)
            assert after['t'] == (t if mode == 'advance' else 77)
            upd = -ref['params'][:8]
            err = np.abs(after['params'][:8].astype(np.float64) + upd)
            bound = (R.rel_lr(hyp, t) + 6 * R.U) * upd
            q = float((err / bound).max())
            worst = max(worst, q)
            print("lr_t: b2 %g t %d %s: error / bound %.3g (relative error %.3g, bound %.3g)" % (b2, t, 'counter' if mode == 'advance' else 'step_t', q,
                                                                                          float((err / upd).max()), R.rel_lr(hyp, t) + 6 * R.U))
            assert q <= 1.0
    _REPORT['lr'] = max(_REPORT['lr'], worst)
    print("lr_t by itself, b2 %g, opt %d: worst error / bound %.3g" % (b2, opt, worst))


CONSUMED = [('flat_193x100', 'gdot'), ('flat_193x100', 'vn2'), ('flat_first_145x4', 'gdot'), ('flat_11264x88', 'vn2'),
            ('pair_193x126', 'gdot'), ('pair_193x126', 'vn2'), ('pair_first_145x2', 'vn2'), ('pair_11264x90', 'gdot')]


@pytest.mark.parametrize("cname,which", CONSUMED, ids=["%s-%s" % c for c in CONSUMED])
def test_known_sums_are_consumed(dev, cname, which):
    """that the two-launch form ran, and not the chain behind its back: gdot, or the stored vn2, is handed over 1 % too large.  The
    known-sums form takes them on trust, so its outputs are those of the known-sums reference ON THESE INPUTS, every element
    within its bound; the chain would recompute both sums from the parameters, so the same outputs lie beyond the bounds of
    the plain-form reference (params, and mg through grad_g).  Both bodies, with the tall matrix first and in the middle."""
    case = BY_NAME[cname]
    table, n, n_cols, st = R.make_state(case, 'fast')
    hyp = R.hyper()
    g, _ = R.make_grads(table, n, 77)
    ti = R.tall_index(table)
    d = table[ti]
    assert_rule('fast', table, case)
    ts = R.true_sums(st['params'], st['s'], g, d)
    off = np.float32(1.01)
    st['vn2'][d.col_offset:d.col_offset + d.cols] = ts['A'].astype(np.float32) * (off if which == 'vn2' else np.float32(1))
    known = dict(tensor=ti, use=True, gdot=ts['gdot'].astype(np.float32) * (off if which == 'gdot' else np.float32(1)))
    D = Dev(dev, table, st, g)
    before = D.read()
    D.step(table, hyp, 'advance', known)
    after = D.read()
    compare('fast-%s off-by-1%% inputs' % R.fast_body(d), after, before, R.ref_step(before, g, table, hyp, 'advance', known), table, g)
    plain = R.ref_step(before, g, table, hyp, 'advance', dict(tensor=ti, use=False, gdot=None))
    bad = dict(R.violations(after, plain))
    print("\n%s, %s 1 %% off: against the plain form, error / bound: %s" % (cname, which, ", ".join("%s %.3g" % kv for kv in R.ratios(after, plain).items())))
    assert 'params' in bad and 'mg' in bad and 'm' in bad, bad
    # and the vn2 it leaves is computed afresh from V': the true sum of what it stored
    check_sums('fast-%s off-by-1%% inputs' % R.fast_body(d), after, table, g)


MODE_CASES = [('small', 'small'), ('chain_tall_last', 'chain'), ('flat_193x100', 'fast'), ('pair_193x126', 'fast'), ('mixed_plain', 'adam')]


@pytest.mark.parametrize("cname,route", MODE_CASES, ids=["%s-%s" % m for m in MODE_CASES])
@pytest.mark.parametrize("mode", ['advance', 'readonly', 'advanced', 'explicit'])
def test_counter_modes(dev, cname, route, mode):
    """advance, read-only (-1), CLV_STEP_ADVANCED and an explicit t with a NULL counter: the counter afterwards, and the outputs
    are those of the right t -- within the bounds of the reference at t, beyond them for the reference at t - 1 and at t + 1"""
    case = BY_NAME[cname]
    table, n, n_cols, st = R.make_state(case, route)
    hyp = R.hyper(opt=R.ROUTE_OPT[route])
    g, _ = R.make_grads(table, n, 321)
    known = None
    if route in ('chain', 'fast'):
        ti = R.tall_index(table)
        d = table[ti]
        if route == 'fast':                # an honest vn2: the true sums of the stored parameters, rounded
            st['vn2'][d.col_offset:d.col_offset + d.cols] = R.true_sums(st['params'], st['s'], g, d)['A'].astype(np.float32)
        known = known_for(table, st, g, route == 'fast')
    st['t'] = 3
    m = ('explicit', 6) if mode == 'explicit' else mode
    t, counter = R.step_of(3, m)
    D = Dev(dev, table, st, g)
    before = D.read()
    D.step(table, hyp, m, known)
    after = D.read()
    ref = R.ref_step(before, g, table, hyp, m, known)
    assert ref['t'] == t
    compare(route_key(route, table, route == 'fast') + ' modes', after, before, ref, table, g)
    assert after['t'] == (3 if counter is None else counter)
    for other in (t - 1, t + 1):
        wrong = R.ref_step(before, g, table, hyp, ('explicit', other), known)
        assert ('params', ) == tuple(k for k, _ in R.violations(after, wrong, ('params',))), (other, R.ratios(after, wrong))


def test_what_a_step_must_not_touch(dev):
    """stated on its own, though every comparison above holds it too: under RMSprop m, mg, vg, s, vn2 stay bitwise, under plain
    Adam mg, vg, s, vn2; with only= every array slice of every tensor outside the sub-table, vn2 included; sentinels, canaries
    and grads always"""
    case = BY_NAME['mixed_plain']
    for route, frozen in (('rmsprop', ('m', 'mg', 'vg', 's', 'vn2')), ('adam', ('mg', 'vg', 's', 'vn2'))):
        table, n, n_cols, st = R.make_state(case, route)
        for k in ('mg', 'vg', 's', 'vn2'):          # something to lose: not only sentinels
            st[k] = np.random.default_rng(3).standard_normal(n_cols).astype(np.float32)
        if route == 'rmsprop':
            st['m'] = np.random.default_rng(4).standard_normal(n).astype(np.float32)
        g, _ = R.make_grads(table, n, 11)
        D = Dev(dev, table, st, g)
        D.step(table, R.hyper(opt=R.ROUTE_OPT[route]), 'advance', known_for(table, st, g, False))
        after = D.read()
        for k in frozen:
            assert (after[k].view(np.uint32) == st[k].view(np.uint32)).all(), (route, k)
        assert (after['grads'].view(np.uint32) == g.view(np.uint32)).all() and (after['params'] != st['params']).any()
    for cname, route, only in (('small', 'small', ('b/kernel', 'c/bias', 'f/kernel')), ('flat_only_193x128', 'chain', ('b/bias', 't/kernel')),
                               ('chain_two_tall_main_loop', 'chain', ('q/kernel', 't/kernel'))):
        table, n, n_cols, st = R.make_state(BY_NAME[cname], route)
        st['vn2'] = np.random.default_rng(5).standard_normal(n_cols).astype(np.float32)
        g, _ = R.make_grads(table, n, 12)
        sub = [d for d in table if d.name in only]
        D = Dev(dev, table, st, g)
        D.step(sub, R.hyper(), 'readonly', known_for(sub, st, g, False))
        after = D.read()
        own_f, own_c = np.zeros(n, bool), np.zeros(n_cols, bool)
        for d in sub:
            own_f[d.offset:d.offset + d.rows * d.cols] = True
            if d.is_matrix:
                own_c[d.col_offset:d.col_offset + d.cols] = True
        for k in R.FLAT:
            assert (after[k][~own_f].view(np.uint32) == st[k][~own_f].view(np.uint32)).all(), (cname, k)
            assert (after[k][own_f] != st[k][own_f]).any()
        for k in R.COLS:
            assert (after[k][~own_c].view(np.uint32) == st[k][~own_c].view(np.uint32)).all(), (cname, k)
        assert after['t'] == st['t']


REFUSALS = [
    # name, shapes, what is wrong, expected status
    ('odd_cols', [('t/kernel', (160, 7)), ('a/bias', (3,))], dict(use=True), EINVAL),
    ('cols_above_128', [('t/kernel', (160, 130)), ('a/bias', (3,))], dict(use=True), EINVAL),
    ('two_tall', [('t/kernel', (160, 8)), ('u/kernel', (150, 4))], dict(use=True), EINVAL),
    ('gdot_null', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(use=True, null=('gdot',)), EINVAL),
    ('vnorm2_null', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(use=True, null=('vnorm2',)), EINVAL),
    ('tensor_small', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(use=True, tensor=0), EINVAL),
    ('tensor_bias', [('a/bias', (8,)), ('t/kernel', (160, 8))], dict(use=True, tensor=0), EINVAL),
    ('tensor_negative', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(use=True, tensor=-1), EINVAL),
    ('tensor_beyond', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(use=True, tensor=2), EINVAL),
    ('weightnorm_minus1', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(weightnorm=-1), EINVAL),
    ('weightnorm_3', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(weightnorm=3), EINVAL),
    ('workspace_short', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(ws_short=1), EWORKSPACE),
    ('workspace_short_fast', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(use=True, ws_short=1), EWORKSPACE),
    ('wn_without_mg', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(null=('mg',)), EINVAL),
    ('wn_without_vg', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(null=('vg',)), EINVAL),
    ('wn_without_s', [('a/kernel', (16, 3)), ('t/kernel', (160, 8))], dict(null=('s',)), EINVAL),
]


@pytest.mark.parametrize("name,shapes,what,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(dev, name, shapes, what, status):
    """every CLV_EINVAL / CLV_EWORKSPACE condition of the launcher returns its code, opens no profiler scope (no launch) and leaves
    every buffer and the counter bitwise as they were.  Host-side argument checks: nothing faulting is launched."""
    case = dict(name=name, shapes=shapes, routes=('chain',), only=None)
    table, n, n_cols, st = R.make_state(case, 'chain')
    g, _ = R.make_grads(table, n, 13)
    tall = [i for i, d in enumerate(table) if R.is_tall(d)]
    d = table[tall[0]]
    st['vn2'][d.col_offset:d.col_offset + d.cols] = R.true_sums(st['params'], st['s'], g, d)['A'].astype(np.float32)
    known = known_for(table, st, g, True)
    known['use'] = bool(what.get('use'))
    known['tensor'] = what.get('tensor', known['tensor'])
    D = Dev(dev, table, st, g)
    before = D.read()
    D.step(table, R.hyper(), 'advance', known, ws_short=what.get('ws_short', 0), null=what.get('null', ()),
           weightnorm=what.get('weightnorm'), expect=status)
    after = D.read()
    for k in R.OUTPUTS + ('grads',):
        assert (after[k].view(np.uint32) == before[k].view(np.uint32)).all(), k
    assert after['t'] == before['t']
    D.step(table, R.hyper(), 'advance', dict(known, use=False, tensor=tall[0]))       # the table itself is acceptable: the chain takes it
    assert D.read()['t'] == before['t'] + 1


DET = [('small', 'small'), ('chain_two_tall_main_loop', 'chain'), ('flat_11264x88', 'fast'), ('pair_11264x90', 'fast'),
       ('mixed_plain', 'adam'), ('mixed_plain', 'rmsprop')]


@pytest.mark.parametrize("cname,route", DET, ids=["%s-%s" % m for m in DET])
def test_determinism(dev, cname, route):
    """no atomics: the same state and gradients twice give bitwise equal outputs"""
    table, n, n_cols, st = R.make_state(BY_NAME[cname], route)
    hyp = R.hyper(opt=R.ROUTE_OPT[route])
    g, _ = R.make_grads(table, n, 14)
    known = None
    if route in ('chain', 'fast'):
        if route == 'fast':
            d = table[R.tall_index(table)]
            st['vn2'][d.col_offset:d.col_offset + d.cols] = R.true_sums(st['params'], st['s'], g, d)['A'].astype(np.float32)
        known = known_for(table, st, g, route == 'fast')
    outs = []
    for _ in range(2):
        D = Dev(dev, table, st, g)
        D.step(table, hyp, 'advance', known)
        outs.append(D.read())
    for k in R.OUTPUTS:
        assert (outs[0][k].view(np.uint32) == outs[1][k].view(np.uint32)).all(), k
    assert (outs[0]['params'] != st['params']).any()
