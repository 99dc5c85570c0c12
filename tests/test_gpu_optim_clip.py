"""-m gpu: clv_grad_norm_scale and clv_adam_wn_step_clipped (csrc/optim.hip) called directly through ctypes on the tables of
optim_reference.GPU_CASES (2 x 1 up to 11264 x 90, padding full of 4321.0), against tests/optim_clip_reference.py:

  1. norm and scale within their derived bounds for clipnorm = 0.25 norm64, 4 norm64 and inf; two runs, equal bits; grads untouched;
  2. every output of a clipped step, every case and route, against optim_reference.ref_step on g_eff (gdot_eff on the fast route)
     formed from the DEVICE's scale, with ref_step's own bounds and the rms criterion, padding included: clipnorm, clipvalue
     (the median |g|), both.  The fast route has no clipvalue variant: the contract refuses the known-sums form with a
     clamp, and what FlatParams passes then (use = 0) is the chain route of the same table, which is there;
  3. identities without a tolerance: (NULL, 0, 0), a grad_scale that holds 1, and the scale left by clipnorm = inf give the outputs
     of clv_adam_wn_step bit for bit;
  4. decay by itself (as test_gpu_optim.test_lr_t_by_itself isolates lr_t) under all four counter rules, then one whole step per route;
  5. refusals: the status, no launch (no profiler scope), every buffer as it was;
  6. through the model: TrainStep / Model / the train CLIs (cl_vrnn B 8, T 6, L 2, C 3 and a cl_vae).

Buffers, canaries and plans are test_gpu_optim.Dev's.  Every GPU call here is an ordinary in-bounds launch."""
import ctypes as Ct
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import optim_clip_reference as RC
import optim_reference as R
from helpers import CANARY, TAIL, make_synthetic_pickle
from test_gpu_optim import Dev
from vae_reference import U

pytestmark = pytest.mark.gpu

EINVAL, EWORKSPACE = -1, -2
F = np.float32
_WORST = dict(norm=0.0, scale=0.0, lr=0.0)


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    yield torch.device("cuda:0")
    print("\nworst error / bound: norm %.3g, scale %.3g; decay by itself: %.3g" % (_WORST['norm'], _WORST['scale'], _WORST['lr']))


class ClipDev(Dev):
    """test_gpu_optim.Dev with the two new entry points; `stats` [2] with a canary tail"""

    def __init__(self, dev, table, st, grads):
        super().__init__(dev, table, st, grads)
        self.stats = torch.full((2 + TAIL,), CANARY, dtype=torch.float32, device=dev)
        self.one = torch.ones(1, dtype=torch.float32, device=dev)

    def read_stats(self):
        torch.cuda.synchronize()
        h = self.stats.cpu().numpy()
        assert (h[2:] == CANARY).all(), "write behind stats"
        return h[:2].copy()

    def _profiled(self, call, scope, expect):
        from clvae_amd import ops
        ops.prof_enable(True)
        try:
            status = call()
            torch.cuda.synchronize()
            names = [n for n, _, _ in ops.prof_collect()]
        finally:
            ops.prof_enable(False)
        assert status == expect, (status, expect)
        assert (scope in names) == (status == 0), names
        return status

    def norm(self, descs, clipnorm, ws_short=0, null=(), expect=0):
        from clvae_amd import _lib, ops
        p_ = ops._ptr
        L = _lib.lib()
        tb, plan = self.plan(descs)
        need = L.clv_grad_norm_workspace_bytes(tb, len(descs))
        assert need > 0 and need % 4 == 0
        ws = torch.full((need // 4 + TAIL,), CANARY, dtype=torch.float32, device=self.dev)
        arg = lambda k, v: None if k in null else v
        status = self._profiled(lambda: L.clv_grad_norm_scale(
            arg('table', tb), len(descs), arg('plan', p_(plan)), arg('grads', p_(self.a['grads'])), float(clipnorm),
            arg('stats', p_(self.stats)), arg('ws', p_(ws)), need - ws_short, ops._stream()), 'grad_norm_scale', expect)
        assert (ws.cpu().numpy()[need // 4:] == CANARY).all(), "write behind the workspace"
        return status

    def step_clipped(self, descs, hyp, mode='advance', known=None, scale=None, clipvalue=0.0, decay=0.0, expect=0):
        """one clv_adam_wn_step_clipped; scale: None (NULL), 'stats' (stats + 1) or 'one' (a device 1.0f)"""
        from clvae_amd import _lib, ops
        p_ = ops._ptr
        L = _lib.lib()
        tb, plan = self.plan(descs)
        need = L.clv_adam_wn_workspace_bytes(tb, len(descs))
        ws = torch.full((need // 4 + TAIL,), CANARY, dtype=torch.float32, device=self.dev)
        ks = None
        if known is not None:
            if known.get('gdot') is not None:
                gd = np.asarray(known['gdot'], np.float32)
                self.gdot = torch.full((gd.size + TAIL,), CANARY, dtype=torch.float32, device=self.dev)
                self.gdot[:gd.size] = torch.as_tensor(gd, device=self.dev)
                self.gdot_n = gd.size
            ks = _lib.AdamKnownSums(int(known['tensor']), int(bool(known.get('use'))),
                                    p_(self.gdot) if known.get('gdot') is not None else None, p_(self.a['vn2']))
        it, step_t = {'advance': (self.it, 0), 'readonly': (self.it, R.STEP_READONLY), 'advanced': (self.it, R.STEP_ADVANCED)}.get(
            mode if isinstance(mode, str) else None, (None, mode[1] if isinstance(mode, tuple) else 0))
        sp = {None: None, 'stats': p_(self.stats[1:]), 'one': p_(self.one)}[scale]
        a = self.a
        status = self._profiled(lambda: L.clv_adam_wn_step_clipped(
            tb, len(descs), p_(plan), p_(a['params']), p_(a['grads']), p_(a['m']), p_(a['v']), p_(a['mg']), p_(a['vg']), p_(a['s']),
            p_(it), int(step_t), hyp['lr'], hyp['b1'], hyp['b2'], hyp['eps'], hyp['opt'], Ct.byref(ks) if ks is not None else None,
            p_(ws), need, ops._stream(), sp, float(clipvalue), float(decay)), 'adam_wn_step', expect)
        assert (ws.cpu().numpy()[need // 4:] == CANARY).all(), "write behind the workspace"
        return status


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def hold(after, before, ref, table, grads):
    """test_gpu_optim.compare without its report: every output within its bound (0 where the step owns nothing), rms, counter, grads"""
    assert not R.violations(after, ref), R.ratios(after, ref)
    assert not R.rms_violations(after, ref, table), R.rms(after, ref, table)
    assert after['t'] == (ref['counter'] if ref['counter'] is not None else before['t'])
    assert (bits(after['grads']) == bits(grads)).all(), "grads written"


# ------------------------------------------------------------------------------------------------ 1. norm and scale --
@pytest.mark.parametrize("case", R.GPU_CASES, ids=[c['name'] for c in R.GPU_CASES])
def test_norm_and_scale(dev, case):
    table, n, n_cols = R.layout(case['shapes'])
    g, _ = R.make_grads(table, n, 900)
    st = {k: np.zeros(n, F) for k in R.FLAT}
    st.update({k: np.zeros(n_cols, F) for k in R.COLS}, t=0)
    D = ClipDev(dev, table, st, g)
    nm = RC.norm64(g, table)
    for clipnorm in (F(0.25 * nm), F(4 * nm), F(np.inf)):
        ref = RC.norm_ref(g, table, clipnorm)
        runs = []
        for _ in range(2):
            D.stats[:2] = CANARY
            D.norm(table, clipnorm)
            runs.append(D.read_stats())
        assert (bits(runs[0]) == bits(runs[1])).all(), "two runs, other bits"
        got = runs[0].astype(np.float64)
        qn = abs(got[0] - ref['norm']) / ref['b_norm']
        print("%s clipnorm %.6g: norm %.9g (fp64 %.9g) error / bound %.3g; scale %.9g (fp64 %.9g, bound %.3g)"
              % (case['name'], clipnorm, got[0], ref['norm'], qn, got[1], ref['scale'], ref['b_scale']))
        assert qn <= 1.0
        _WORST['norm'] = max(_WORST['norm'], qn)
        assert abs(got[1] - ref['scale']) <= ref['b_scale']
        if ref['b_scale'] > 0:
            _WORST['scale'] = max(_WORST['scale'], abs(got[1] - ref['scale']) / ref['b_scale'])
        else:
            assert runs[0][1] == F(1)            # nothing clipped: an exact 1
        after = D.read()
        assert (bits(after['grads']) == bits(g)).all(), "grads written"
    if case['only']:        # a sub-table's norm is the norm of its own tensors
        sub = [d for d in table if d.name in case['only']]
        D.norm(sub, F(np.inf))
        ref = RC.norm_ref(g, sub, np.inf)
        assert abs(float(D.read_stats()[0]) - ref['norm']) <= ref['b_norm']


# ---------------------------------------------------------------------------------- 2. every output of a clipped step --
CLIPPED = [(c, r, v) for c, r in RC.CASE_ROUTES for v in RC.VARIANTS if not (r == 'fast' and v != 'clipnorm')]


@pytest.mark.parametrize("case,route,variant", CLIPPED, ids=["%s-%s-%s" % (c['name'], r, v) for c, r, v in CLIPPED])
def test_every_output_of_a_clipped_step(dev, case, route, variant):
    table, n, n_cols, st, g = RC.prepared(case, route)
    hyp = R.hyper(opt=R.ROUTE_OPT[route])
    wn = hyp['opt'] == R.OPT_ADAM_WN
    clipnorm, clipvalue = RC.clip_args(variant, g, table)
    D = ClipDev(dev, table, st, g)
    before = D.read()
    scale32 = F(1)
    if clipnorm > 0:
        D.norm(table, clipnorm)                     # over the whole table, whatever sub-tables the step is issued in
        ref = RC.norm_ref(g, table, clipnorm)
        stats = D.read_stats()
        assert abs(float(stats[0]) - ref['norm']) <= ref['b_norm'] and abs(float(stats[1]) - ref['scale']) <= ref['b_scale']
        scale32 = stats[1]
        assert abs(float(scale32) - RC.CLIP_FACTOR) < 1e-5
    use = route == 'fast'
    if use and case['only']:            # the fast form through a sub-table, the other tensors in a second call that advances
        sub = [d for d in table if d.name in case['only']]
        rest = [d for d in table if d.name not in case['only']]
        calls = [(sub, 'readonly', RC.known_for(sub, before, g, True)), (rest, 'advance', None)]
    else:
        calls = [(table, 'advance', RC.known_for(table, before, g, use) if wn else None)]
    for descs, mode, known in calls:
        ref, ge = RC.clipped_ref(before, g, descs, hyp, mode, known, scale32, clipvalue, full_table=table)
        D.step_clipped(descs, hyp, mode, known, scale='stats' if clipnorm > 0 else None, clipvalue=clipvalue)
        after = D.read()
        hold(after, before, ref, descs, g)
        before = after
    assert after['t'] == st['t'] + 1
    if clipnorm > 0:
        assert (bits(D.read_stats()) == bits(stats)).all()


# --------------------------------------------------------------------------------- 3. identities without a tolerance --
IDENT = [('small', 'small'), ('chain_two_tall_main_loop', 'chain'), ('flat_193x100', 'fast'), ('pair_193x126', 'fast'),
         ('pair_first_145x2', 'fast'), ('pair_middle_160x6', 'fast'), ('pair_11264x90', 'fast'), ('flat_11264x88', 'fast'), ('flat_only_193x128', 'chain'), ('mixed_plain', 'adam'), ('mixed_plain', 'rmsprop')]


@pytest.mark.parametrize("cname,route", IDENT, ids=["%s-%s" % m for m in IDENT])
def test_identities(dev, cname, route):
    """(NULL, 0, 0), a grad_scale that holds 1.0f and the scale clipnorm = inf leaves: clv_adam_wn_step's outputs bit for bit.

    The float2 body of the two-launch form (the pair_ cases) is where this is least a matter of course: see
    GradClipped::second_moment in csrc/optim.hip."""
    table, n, n_cols, st, g = RC.prepared(RC.BY_NAME[cname], route)
    hyp = R.hyper(opt=R.ROUTE_OPT[route])
    known = RC.known_for(table, st, g, route == 'fast') if hyp['opt'] == R.OPT_ADAM_WN else None
    D = ClipDev(dev, table, st, g)
    D.step(table, hyp, 'advance', known)
    plain = D.read()
    assert (plain['params'] != st['params']).any()
    for scale in (None, 'one', 'stats'):
        D = ClipDev(dev, table, st, g)
        if scale == 'stats':
            D.norm(table, F(np.inf))
            assert D.read_stats()[1] == F(1)
        D.step_clipped(table, hyp, 'advance', known, scale=scale)
        got = D.read()
        for k in R.OUTPUTS + ('grads',):
            assert (bits(got[k]) == bits(plain[k])).all(), (scale, k)
        assert got['t'] == plain['t']


# ------------------------------------------------------------------------------------------------------------ 4. decay --
@pytest.mark.parametrize("opt", [R.OPT_ADAM_WN, R.OPT_ADAM])
@pytest.mark.parametrize("mode", ['advance', 'readonly', 'advanced', 'explicit'])
def test_decay_by_itself(dev, opt, mode):
    """test_gpu_optim.test_lr_t_by_itself with a decayed rate: a bias, params = m = v = 0, g = 1, so params' = -lr_t (1 - b1) /
    (sqrt(1 - b2) + eps) and the error is lr_t's own plus the six roundings of the update, plus one U for the fp64 rate
    rounded to fp32.  The reference rate is lr / (1 + decay (t - 1)) in fp64, unrounded.  All four counter rules: it = t - 1
    under CLV_STEP_ADVANCED too (the counter then holds t)."""
    table, n, n_cols = R.layout([('b/bias', (8,))] + ([('a/kernel', (2, 4))] if opt == R.OPT_ADAM_WN else []))
    mat = opt == R.OPT_ADAM_WN
    hyp = R.hyper(opt=opt)
    rng = np.random.default_rng(8)
    for t in (1, 2, 1000, 10 ** 6):
        for decay in (1e-4, 1.0):
            st = {k: np.full(n, CANARY, np.float32) for k in R.FLAT}
            st.update({k: np.full(n_cols, CANARY, np.float32) for k in R.COLS})
            for k in R.FLAT:
                st[k][:n] = 0
            if mat:
                st['params'][8:16] = 0.1 * rng.standard_normal(8)
                st['mg'][:4] = st['vg'][:4] = 0
                st['s'][:4] = 1
            m = ('explicit', t) if mode == 'explicit' else mode
            st['t'] = {'advance': t - 1, 'readonly': t - 1, 'advanced': t, 'explicit': 77}[mode]
            g = np.full(n, CANARY, np.float32)
            g[:8] = 1
            if mat:
                g[8:16] = rng.standard_normal(8)
            D = ClipDev(dev, table, st, g)
            exact = dict(hyp, lr=hyp['lr'] / (1.0 + float(F(decay)) * (t - 1)))          # fp64, not rounded
            ref = R.ref_step(st, g, table, exact, m)
            assert ref['t'] == t
            D.step_clipped(table, hyp, m, decay=decay)
            after = D.read()
            assert after['t'] == {'advance': t, 'readonly': t - 1, 'advanced': t, 'explicit': 77}[mode]
            upd = -ref['params'][:8]
            err = np.abs(after['params'][:8].astype(np.float64) + upd)
            bound = (R.rel_lr(hyp, t) + 6 * U + U) * upd
            q = float((err / bound).max())
            _WORST['lr'] = max(_WORST['lr'], q)
            print("decay %g t %d %s: error / bound %.3g" % (decay, t, mode, q))
            assert q <= 1.0
            # and it is the decayed rate, not the plain one, wherever the two lie further apart than the bound
            if decay * (t - 1) > 10 * (R.rel_lr(hyp, t) + 7 * U):
                plain = -R.ref_step(st, g, table, hyp, m)['params'][:8]
                assert (np.abs(after['params'][:8].astype(np.float64) + plain) > (R.rel_lr(hyp, t) + 7 * U) * plain).all()


DECAY_STEPS = [('small', 'small'), ('chain_tall_last', 'chain'), ('flat_193x100', 'fast'), ('pair_193x126', 'fast'),
               ('mixed_plain', 'adam'), ('mixed_plain', 'rmsprop')]


@pytest.mark.parametrize("cname,route", DECAY_STEPS, ids=["%s-%s" % m for m in DECAY_STEPS])
def test_a_decayed_step_per_route(dev, cname, route):
    """one whole step per route through ref_step with the reference's decayed rate (t = 3: lr / 1.5 at decay 0.25); the plain
    rate's reference is beyond the bounds"""
    table, n, n_cols, st, g = RC.prepared(RC.BY_NAME[cname], route)
    hyp = R.hyper(opt=R.ROUTE_OPT[route])
    known = RC.known_for(table, st, g, route == 'fast') if hyp['opt'] == R.OPT_ADAM_WN else None
    D = ClipDev(dev, table, st, g)
    before = D.read()
    assert before['t'] == 2
    ref, _ = RC.clipped_ref(before, g, table, hyp, 'advance', known, F(1), decay=0.25)
    D.step_clipped(table, hyp, 'advance', known, decay=0.25)
    after = D.read()
    hold(after, before, ref, table, g)
    assert 'params' in dict(R.violations(after, R.ref_step(before, g, table, hyp, 'advance', known), ('params',)))


# -------------------------------------------------------------------------------------------------------- 5. refusals --
def test_refusals(dev):
    """every refused value: its status, no launch (no profiler scope opened), stats, every buffer and the counter as they were"""
    case = dict(name='refusals', shapes=[('a/kernel', (16, 3)), ('t/kernel', (160, 8))], routes=('fast',), only=None)
    table, n, n_cols, st, g = RC.prepared(case, 'fast')
    hyp = R.hyper()
    D = ClipDev(dev, table, st, g)
    before = D.read()
    known = RC.known_for(table, before, g, True)

    def untouched():
        after = D.read()
        for k in R.OUTPUTS + ('grads',):
            assert (bits(after[k]) == bits(before[k])).all(), k
        assert after['t'] == before['t'] and (D.read_stats() == CANARY).all()
    for bad in (0.0, -1.0, float('nan')):
        D.norm(table, bad, expect=EINVAL)
    for null in ('table', 'plan', 'grads', 'stats', 'ws'):
        D.norm(table, 1.0, null=(null,), expect=EINVAL)
    D.norm(table, 1.0, ws_short=1, expect=EINVAL)
    untouched()
    for bad in (-1.0, float('nan')):
        D.step_clipped(table, hyp, 'advance', None, clipvalue=bad, expect=EINVAL)
    for bad in (-1.0, float('nan'), float('inf')):
        D.step_clipped(table, hyp, 'advance', None, decay=bad, expect=EINVAL)
    D.step_clipped(table, hyp, 'advance', known, scale='one', clipvalue=0.5, expect=EINVAL)       # clipvalue with known.use
    untouched()
    D.step_clipped(table, hyp, 'advance', dict(known, use=False), scale='one', clipvalue=0.5)     # the same table, the chain: accepted
    assert D.read()['t'] == before['t'] + 1


# ----------------------------------------------------------------------------------------------- 6. through the model --
def _t(a, dev):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=dev)


def _vrnn(dev, seed=11):
    from clvae_amd.engine import VrnnEngine
    from oracle import clvae_oracle as O
    B, Tn, L, C = 8, 6, 2, 3
    cfg = O.vrnn_config(latent_dim=L, seq_length=Tn, n_classes=C, use_x_prev=True)
    p = {k: np.asarray(v, np.float32) for k, v in O.vrnn_init_params(cfg, seed=seed).items()}
    rng = np.random.default_rng(0)
    win = (rng.random((B, Tn + 1, 88)) < 0.05).astype(np.float32)
    wt = np.eye(C, dtype=np.float32)[rng.integers(0, C, B)]
    eng = VrnnEngine(cfg, B, dev)
    eng.P.set_weights(p)
    return eng, (_t(win[:, 1:], dev), _t(win[:, :-1], dev), _t(wt, dev))


def _vae(dev, seed=6):
    from clvae_amd.engine import VaeEngine
    from oracle import clvae_oracle as O
    B, C = 8, 3
    cfg = O.vae_config(latent_dim=3, n_classes=C, use_x_prev=True)
    eng = VaeEngine(cfg, B, dev)
    eng.P.set_weights({k: np.asarray(v, np.float32) for k, v in O.vae_init_params(cfg, seed=seed).items()})
    rng = np.random.default_rng(1)
    x = (rng.random((B, 88)) < 0.1).astype(np.float32)
    xp = (rng.random((B, 88)) < 0.1).astype(np.float32)
    wt = np.eye(C, dtype=np.float32)[rng.integers(0, C, B)]
    return eng, (_t(x, dev), _t(xp, dev), _t(wt, dev))


def _flat(P, buf):
    own = np.zeros(P.n, bool)
    for i in range(len(P.shapes)):
        d = P.table[i]
        own[d.offset:d.offset + d.rows * d.cols] = True
    return buf.detach().cpu().numpy().astype(np.float64), own


@pytest.mark.parametrize("family", ['cl_vrnn', 'cl_vae'])
def test_one_adam_step_of_a_model_with_clipnorm(dev, family):
    """optimizer 'adam', equal seeds: after one step P.m = (1 - b1) g for every tensor, so the unclipped twin's P.m gives the
    whole gradient and its norm64.  (Held here first: P.m against (1 - b1) times the gradient buffer the step left, one
    rounding; the gradient, and m_unclipped in what follows, are then taken in their exact values, (1 - b1) g in fp64, not
    through m's own rounding.)  With clipnorm = 0.5 norm64 on a twin, grad_stats reads the norm and 0.5 within test 1's
    bounds and P.m = 0.5 m_unclipped within that bound plus two roundings (the scaled gradient's, and m's own)."""
    from clvae_amd.trainer import TrainStep
    make = _vrnn if family == 'cl_vrnn' else _vae
    eng, batch = make(dev)
    ts = TrainStep(eng, seed=5, optimizer='adam', use_graph=False)
    ts.stage_batch(*batch)
    ts.step()
    torch.cuda.synchronize()
    m0, own = _flat(eng.P, eng.P.m)
    g64, _ = _flat(eng.P, eng.P.grads)
    c1 = 1.0 - float(F(0.9))
    assert (np.abs(m0 - c1 * g64)[own] <= U * np.abs(c1 * g64)[own]).all(), "P.m is not (1 - b1) g"
    assert (eng.P.grad_stats.cpu().numpy() == np.asarray([0, 1], F)).all()
    descs = [R.Desc('t%d' % i, (), eng.P.table[i].offset, eng.P.table[i].rows, eng.P.table[i].cols, eng.P.table[i].col_offset,
                    eng.P.table[i].is_matrix) for i in range(len(eng.P.shapes))]
    nm = RC.norm64(g64, descs)
    assert nm > 0
    clipnorm = float(F(0.5 * nm))
    ref = RC.norm_ref(g64, descs, clipnorm)
    eng2, batch2 = make(dev)
    ts2 = TrainStep(eng2, seed=5, optimizer='adam', use_graph=False, clipnorm=clipnorm)
    ts2.stage_batch(*batch2)
    ts2.step()
    torch.cuda.synchronize()
    assert (bits(eng2.P.grads.cpu().numpy()) == bits(eng.P.grads.cpu().numpy())).all(), "the twins' gradients differ"
    stats = ts2.grad_stats.cpu().numpy().astype(np.float64)
    assert ts2.grad_stats is eng2.P.grad_stats
    print("%s: norm %.9g (fp64 %.9g, bound %.3g), scale %.9g (fp64 %.9g, bound %.3g)" % (family, stats[0], nm, ref['b_norm'], stats[1],
                                                                                      ref['scale'], ref['b_scale']))
    assert abs(stats[0] - nm) <= ref['b_norm'], (stats, nm, ref)
    assert abs(stats[1] - ref['scale']) <= ref['b_scale'] and abs(ref['scale'] - 0.5) < 1e-6
    m1, _ = _flat(eng2.P, eng2.P.m)
    half = ref['scale'] * c1 * g64                       # 0.5 m_unclipped
    bound = ref['b_scale'] / ref['scale'] * np.abs(half) + 2 * U * np.abs(half)
    assert (np.abs(m1 - half)[own] <= bound[own]).all(), float((np.abs(m1 - half)[own] / np.maximum(bound[own], 1e-300)).max())
    assert (m1[~own] == 0).all() and np.abs(m1[own]).max() > 0
    # and the parameters moved differently: the second moment took (0.5 g)^2
    v0, _ = _flat(eng.P, eng.P.v)
    v1, _ = _flat(eng2.P, eng2.P.v)
    big = own & (v0 > 1e-20)
    assert big.any() and np.allclose(v1[big], 0.25 * v0[big], rtol=1e-5)


def test_cl_vrnn_adam_wn_takes_the_known_sums_form_under_clipnorm(dev):
    """'adam-wn' on cl_vrnn with clipnorm: after the first (five-launch) step norms_valid holds and the step is the two-launch
    known-sums form -- 2 norm launches + 2, against 2 + 5 with fast_adam off (counted from the profiler's scopes' kernel
    records is not possible: one scope per call; so the route is shown as test_gpu_optim does, by what the form alone
    consumes: gdot).  Its parameters stay within ref_step's bounds of the five-launch form on the same gradients."""
    from clvae_amd.trainer import TrainStep
    eng, batch = _vrnn(dev)
    ts = TrainStep(eng, seed=5, optimizer='adam-wn', use_graph=False, clipnorm=1e-3)
    ts.stage_batch(*batch)
    ts.step()
    assert eng.P.norms_valid and eng.P.tall_tensor() is not None
    P = eng.P
    snap = lambda: {k: getattr(P, k).detach().clone() for k in ('params', 'm', 'v', 'mg', 'vg', 's', 'vn2', 'iterations')}
    # the second step in pieces: backward, then the optimizer twice from the same state and gradients
    ts._main()
    ts._tail()
    assert eng.gdot_fresh
    gdot = ts._gdot()
    assert gdot is not None
    s0 = snap()
    g = P.grads.detach().cpu().numpy().copy()
    P.adam_step(lr=ts.lr, b2=ts.b2, weightnorm=1, gdot=gdot, **ts.clip)          # what _update() issues
    assert P.norms_valid
    torch.cuda.synchronize()
    fast = snap()
    stats = P.grad_stats.cpu().numpy().copy()
    assert stats[0] > 1e-3 and abs(stats[1] * stats[0] - 1e-3) < 1e-8           # clipped
    # the form consumed gdot: with gdot 1 % off the parameters of the tall matrix come out differently
    for k, v in s0.items():
        getattr(P, k).copy_(v)
    P.norms_valid = True
    P.adam_step(lr=ts.lr, b2=ts.b2, weightnorm=1, gdot=gdot * 1.01, **ts.clip)
    torch.cuda.synchronize()
    assert (snap()['params'] != fast['params']).any(), "gdot was not read: not the known-sums form"
    # the five-launch form on the same state and gradients, through the fp64 reference
    descs = [R.Desc('t%d' % i, (), P.table[i].offset, P.table[i].rows, P.table[i].cols, P.table[i].col_offset, P.table[i].is_matrix)
             for i in range(len(P.shapes))]
    st = {k: s0[k].cpu().numpy() for k in R.OUTPUTS}
    st['t'] = int(s0['iterations'].item())
    ti = P.tall_tensor()[0]
    ref, _ = RC.clipped_ref(st, g, descs, R.hyper(), 'advance', dict(tensor=ti, use=False, gdot=None), stats[1])
    got = {k: fast[k].cpu().numpy() for k in R.OUTPUTS}
    # gdot comes from the backward pass (its own rounding, not ref_step's), so params are held to the chain's bounds with the
    # known-sums form's extra rounding of B inside them; m, v, mg, vg, s follow from the same sums
    assert not R.violations(got, ref, ('params',)), R.ratios(got, ref, ('params',))
    assert int(fast['iterations'].item()) == st['t'] + 1


@pytest.mark.parametrize("family", ['cl_vrnn', 'cl_vae'])
def test_graph_replay_equals_eager_bit_for_bit(dev, family):
    """4 steps with clipnorm, clipvalue and decay: the captured step (norm launches and clipped optimizer inside the graph) and the
    eager step leave the same bits, grad_stats included"""
    from clvae_amd.trainer import TrainStep
    make = _vrnn if family == 'cl_vrnn' else _vae
    out = []
    for use_graph in (False, True):
        eng, batch = make(dev)
        ts = TrainStep(eng, seed=5, use_graph=use_graph, clipnorm=1e-3, clipvalue=1e-4, decay=0.1)
        for _ in range(4):
            ts.stage_batch(*batch)
            ts.step()
        torch.cuda.synchronize()
        assert (ts._graphs is not None) == use_graph
        out.append([t.cpu().numpy().copy() for t in eng.P.state_tensors()] + [ts.grad_stats.cpu().numpy().copy()])
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()
    assert out[0][-1][0] > 0 and 0 < out[0][-1][1] < 1


def test_forced_dp_schedule_with_clipnorm_takes_the_one_piece_update(dev, monkeypatch):
    """CLV_FORCE_DP_GRAPHS=1: with clipnorm the update is one piece after both buckets (the norm is the averaged gradient's, over
    the whole table); clipvalue and decay alone keep the split update.  4 steps give the single-GPU step's weights within
    test_gpu_api's tolerances for the forced schedule against the plain step (rtol 2e-5, atol 2e-7)."""
    from clvae_amd.trainer import TrainStep
    clip = dict(clipnorm=1e-3, clipvalue=1e-4, decay=0.1)

    def run(**kw):
        eng, batch = _vrnn(dev)
        ts = TrainStep(eng, seed=5, **kw)
        for _ in range(4):
            ts.stage_batch(*batch)
            ts.step()
        torch.cuda.synchronize()
        return ts, eng.P.get_weights(), eng.P.grad_stats.cpu().numpy().copy()
    _, plain, stats = run(**clip)
    monkeypatch.setenv('CLV_FORCE_DP_GRAPHS', '1')
    ts, got, stats_dp = run(**clip)
    assert ts.ar is not None and len(ts.tail_names) == 1 and not ts.split_update
    for k in plain:
        np.testing.assert_allclose(got[k], plain[k], rtol=2e-5, atol=2e-7, err_msg=k)
    np.testing.assert_allclose(stats_dp, stats, rtol=2e-5)
    ts2, got2, _ = run(clipvalue=1e-4, decay=0.1)
    assert ts2.ar is not None and ts2.split_update
    monkeypatch.delenv('CLV_FORCE_DP_GRAPHS')
    _, plain2, _ = run(clipvalue=1e-4, decay=0.1)
    for k in plain2:
        np.testing.assert_allclose(got2[k], plain2[k], rtol=2e-5, atol=2e-7, err_msg=k)


@pytest.mark.parametrize("which,extra", [('cl_vae', ['--use_x_prev', '--latent_dim', '4', '--batch_size', '50']),
                                         ('cl_vrnn', ['--use_x_prev', '--seq_length', '8', '--batch_size', '20'])])
def test_fit_through_the_cli_flags(dev, tmp_path, which, extra):
    """both families, two epochs on the synthetic pickle with --clipnorm, --clipvalue and --lr_decay: finite losses, and the
    step really clipped and decayed (grad_stats; the model's optimizer object carries the three values)"""
    import importlib
    from clvae_amd.cli import OPTIMIZER_FLAGS, parser_for
    TR = importlib.import_module('clvae_amd.%s.train' % which)
    data = make_synthetic_pickle(str(tmp_path / "syn.pickle"), n_songs=(10, 4, 4), seed=1)
    mdir = str(tmp_path / "models")
    os.makedirs(mdir)
    args = parser_for(which + '.train', OPTIMIZER_FLAGS).parse_args(
        ['r', '--num_epochs', '2', '--patience', '0', '--train_file', data, '--model_dir', mdir, '--clipnorm', '0.01',
         '--clipvalue', '0.001', '--lr_decay', '0.01'] + extra)
    np.random.seed(0)
    model, best = TR.train(args)
    o = model.optimizer
    assert (o.name, o.clipnorm, o.clipvalue, o.decay) == ('adam-wn', 0.01, 0.001, 0.01)
    h = model.history.history
    assert len(h['loss']) == 2 and np.isfinite(h['loss']).all() and np.isfinite(h['val_loss']).all()
    ts = model._step
    assert ts.clip == dict(clipnorm=0.01, clipvalue=0.001, decay=0.01)
    stats = ts.grad_stats.cpu().numpy()
    assert np.isfinite(stats).all() and stats[0] > 0.01 and abs(stats[0] * stats[1] - 0.01) < 1e-6
