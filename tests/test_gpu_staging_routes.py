"""-m gpu: which form of the mini-batch assembly a TrainStep picks for what it is bound to, and one warm TrainStep taken from
one form to another.

The assembly has two launch forms -- folded into the step's first launch (ops.label_stage: the label forward launch of the
pair path, the fused cl_vae step) or a clv_gather_rows_multi launch of its own -- and leaves the batch as bytes or as floats.
TrainStep._label_stage / _bytes_batch / _segments / _note_outputs choose, per engine and per kind of source.

1. ROUTES, the expected choice as data, per engine path (at the small shapes the suite already uses for each: the pair path, the
   large-batch use_mx path, cl_vae fused) and source kind.  Beside the choice, after each of period + 2 steps the LIVE batch --
   ts._f8 when set, else ts.X / ts.Xp; w_true; Y when bound -- equals the rows label_reference.stage_rows names, bit for bit.
2. SCRIPTS: sequences of stage_batch / bind_batches / unbind_batches / evaluation / set_weights on ONE TrainStep, run twice from
   the same weights, with use_graph=True and use_graph=False: every loss after every step, every live batch and the parameters
   at the end are equal bit for bit (a capture that allocates, syncs or bakes in a stale route would differ or raise), and
   every bound step was fed the rows its cursor names.  The first script on the pair path is also held to the fp64 oracle with
   the bars of tests/test_gpu_timed_step.py.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from label_reference import stage_rows
from oracle import clvae_oracle as O
from oracle import philox as OP
from test_gpu_timed_step import LOSS_TOL, check_params

pytestmark = pytest.mark.gpu

D = 88
PERIOD = 2
SEED = 2024

# engine paths: the shapes of tests/test_gpu_timed_step.py::test_batch_assembly_inside_the_label_launch_equals_the_gather_launch
# (pair), tests/test_gpu_frames_u8.py::test_step_on_byte_batch_equals_step_on_float_batch (use_mx) and
# test_cl_vae_batch_assembly_inside_the_fused_step_equals_the_gather_launch (cl_vae); `path`: what the engine must report
ENGINES = {
    'pair':        dict(model='vrnn', B=16, T=12, L=2, C=10, hist=True, path=dict(fuse_pair=True, use_mx=False, u8_route='label')),
    'pair-nohist': dict(model='vrnn', B=16, T=12, L=2, C=10, hist=False, path=dict(fuse_pair=True, use_mx=False, u8_route='label')),
    'mx':          dict(model='vrnn', B=768, T=5, L=12, C=3, hist=True, path=dict(fuse_pair=False, use_mx=True, u8_route='gather')),
    'mx-nohist':   dict(model='vrnn', B=768, T=5, L=12, C=3, hist=False, path=dict(fuse_pair=False, use_mx=True, u8_route='gather')),
    'vae':         dict(model='vae', B=40, T=1, L=4, C=2, hist=True, path=dict(fused=True, u8_route=None)),
    'vae-nohist':  dict(model='vae', B=40, T=1, L=4, C=2, hist=False, path=dict(fused=True, u8_route=None)),
}

# source kinds: (frames, row list, history bound?, target bound?)
#   frames    'u8-rows' whole uint8 rows; 'u8-windows' DevWindows of a uint8 frame store; 'f32-rows'; 'u8-view' frames 1 .. T / 0 .. T-1
#             of ONE uint8 [n, T + 1, 88] tensor (rows whole, not back to back: not contiguous)
#   row list  'seq' idx None; 'perm' a permutation; 'rank' a permutation, offset = B with stride = 2 B (rank 1 of 2)
KINDS = {
    'u8-rows':        ('u8-rows', 'seq', True, False),
    'u8-rows-perm':   ('u8-rows', 'perm', True, False),
    'u8-rows-rank':   ('u8-rows', 'rank', True, False),
    'u8-windows':     ('u8-windows', 'perm', True, False),
    'f32-rows':       ('f32-rows', 'perm', True, False),
    'u8-view':        ('u8-view', 'perm', True, False),
    'u8-rows-target': ('u8-rows', 'perm', True, True),
    'hist-missing':   ('u8-rows', 'perm', False, False),       # a model with history frames bound without them
    'hist-unwanted':  ('u8-rows', 'perm', True, False),        # a model without history frames bound with them
    'u8-windows-nohist': ('u8-windows', 'perm', False, False),
}

# (engine, kind) -> (where the batch is assembled, what it is left as)
#   'label': inside the step's first launch (TrainStep._label_stage() gives a stage); 'gather': a launch of its own
#   'bytes': ts._f8 is set and the step reads uint8 frames; 'float': ts.X / ts.Xp
ROUTES = {
    ('pair', 'u8-rows'):        ('label', 'bytes'),
    ('pair', 'u8-rows-perm'):   ('label', 'bytes'),
    ('pair', 'u8-rows-rank'):   ('label', 'bytes'),
    ('pair', 'u8-windows'):     ('label', 'bytes'),
    ('pair', 'f32-rows'):       ('gather', 'float'),
    ('pair', 'u8-view'):        ('gather', 'float'),
    ('pair', 'u8-rows-target'): ('gather', 'float'),
    ('pair', 'hist-missing'):   ('gather', 'float'),
    ('pair-nohist', 'hist-unwanted'):     ('gather', 'float'),
    ('pair-nohist', 'u8-windows-nohist'): ('label', 'bytes'),
    ('mx', 'u8-rows'):          ('gather', 'bytes'),
    ('mx', 'u8-rows-perm'):     ('gather', 'bytes'),
    ('mx', 'u8-rows-rank'):     ('gather', 'bytes'),
    ('mx', 'u8-windows'):       ('gather', 'bytes'),
    ('mx', 'f32-rows'):         ('gather', 'float'),
    ('mx', 'u8-view'):          ('gather', 'float'),
    ('mx', 'u8-rows-target'):   ('gather', 'float'),
    ('mx', 'hist-missing'):     ('gather', 'float'),
    ('mx-nohist', 'hist-unwanted'):       ('gather', 'float'),
    ('mx-nohist', 'u8-windows-nohist'):   ('gather', 'bytes'),
    ('vae', 'u8-rows'):         ('label', 'float'),
    ('vae', 'u8-rows-perm'):    ('label', 'float'),
    ('vae', 'u8-rows-rank'):    ('label', 'float'),
    ('vae', 'u8-windows'):      ('label', 'float'),
    ('vae', 'f32-rows'):        ('gather', 'float'),
    ('vae', 'u8-view'):         ('gather', 'float'),
    ('vae', 'u8-rows-target'):  ('gather', 'float'),
    ('vae', 'hist-missing'):    ('gather', 'float'),
    ('vae-nohist', 'hist-unwanted'):      ('gather', 'float'),
    ('vae-nohist', 'u8-windows-nohist'):  ('label', 'float'),
}


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()
    return torch.device("cuda:0")


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def config(e, **extra):
    if e['model'] == 'vrnn':
        cfg = O.vrnn_config(latent_dim=e['L'], seq_length=e['T'], n_classes=e['C'], use_x_prev=e['hist'])
    else:
        cfg = O.vae_config(latent_dim=e['L'], n_classes=e['C'], use_x_prev=e['hist'])
    return dict(cfg, **extra)


def weights(e, seed):
    init = O.vrnn_init_params if e['model'] == 'vrnn' else O.vae_init_params
    return {k: f32(v) for k, v in init(config(e), seed=seed).items()}


def make_engine(e, dev, p, **extra):
    from clvae_amd.engine import VaeEngine, VrnnEngine
    eng = (VrnnEngine if e['model'] == 'vrnn' else VaeEngine)(config(e, **extra), e['B'], dev)
    path = e['path']
    if e['model'] == 'vrnn':
        assert bool(eng.fuse_pair) == path['fuse_pair'] and bool(eng.use_mx) == path['use_mx']
    else:
        assert bool(eng.fused) == path['fused']
    if 'fuse_notes' not in extra:
        assert eng.frames_u8_route() == path['u8_route']
    eng.P.set_weights(p)
    return eng


class Data:
    """one data set of n = 2 * PERIOD * B windows in every form: a uint8 frame store with a start table (with a repeated start),
    the same windows as whole rows (uint8, float32), as views of one [n, T + 1, 88] tensor; labels; a target (the windows two
    frames on); numpy copies for the reference"""

    def __init__(self, e, dev, seed=7):
        from clvae_amd.trainer import DevWindows
        rng = np.random.default_rng(seed)
        B, T, C = e['B'], e['T'], e['C']
        self.B, self.T, self.n = B, T, 2 * PERIOD * B
        n = self.n
        Fr = n + T + 12
        store = (rng.random((Fr, D)) < 0.05).astype(np.uint8)
        starts = rng.permutation(n + 8)[:n].astype(np.int64)
        starts[1] = starts[0]
        take = lambda t0, k: np.stack([store[s + t0:s + t0 + k] for s in starts])
        self.np = dict(cur=take(1, T).reshape(n, T * D), hist=take(0, T).reshape(n, T * D), target=take(2, T).reshape(n, T * D),
                       w=np.eye(C, dtype=np.float32)[rng.integers(0, C, n)])
        self.perm = rng.permutation(n).astype(np.int64)
        u8 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.uint8), device=dev)
        self.store, self.starts = u8(store), torch.as_tensor(starts, device=dev)
        both = u8(take(0, T + 1))                              # [n, T + 1, 88]: frame 0 is history only, frame T current only
        shape = (n, T, D) if e['model'] == 'vrnn' else (n, D)
        self.dev = {
            'u8-rows': dict(cur=u8(self.np['cur']).view(shape), hist=u8(self.np['hist']).view(shape)),
            'u8-windows': dict(cur=DevWindows(self.store, self.starts, 1), hist=DevWindows(self.store, self.starts, 0)),
            'u8-view': dict(cur=both[:, 1:] if e['model'] == 'vrnn' else both[:, 1], hist=both[:, :-1] if e['model'] == 'vrnn' else both[:, 0]),
        }
        self.dev['f32-rows'] = {k: v.float() for k, v in self.dev['u8-rows'].items()}
        assert not self.dev['u8-view']['cur'].is_contiguous() and not self.dev['u8-view']['hist'].is_contiguous()
        self.target = u8(self.np['target']).view(shape)
        self.w = torch.as_tensor(self.np['w'], device=dev)
        self.d_perm = torch.as_tensor(self.perm, device=dev)

    def bind_args(self, frames, rows, hist=True, target=False, period=PERIOD):
        """(positional, keyword) arguments of bind_batches, and the reference's (idx, period, stride, offset)"""
        B = self.B
        idx, stride, offset = dict(seq=(None, B, 0), perm=(self.perm, B, 0), rank=(self.perm, 2 * B, B))[rows]
        src = self.dev[frames]
        kw = dict(idx=None if idx is None else self.d_perm, period=period, stride=stride, offset=offset,
                  d_target=self.target if target else None)
        return (src['cur'], src['hist'] if hist else None, self.w), kw, (idx, period, stride, offset)


def live_batch(ts, hist, target):
    """what the step was fed, as numpy: X, Xp (or None), w_true, Y (or None) -- the byte batch when the step reads bytes"""
    B = ts.eng.B
    f8 = ts._f8
    x = (f8[0] if f8 is not None else ts.X).reshape(B, -1).cpu().numpy()
    xp = None
    if hist:
        xp = (f8[1] if f8 is not None else ts.Xp).reshape(B, -1).cpu().numpy()
    y = ts.Y.reshape(B, -1).cpu().numpy() if target else None
    return x, xp, ts.w_true.cpu().numpy().copy(), y


def assert_fed(ts, data, sr, hist, target, what):
    x, xp, w, y = live_batch(ts, hist, target)
    assert x.dtype == (np.uint8 if ts._f8 is not None else np.float32)
    assert np.array_equal(x.astype(np.float32), data.np['cur'][sr].astype(np.float32)), (what, 'current frames')
    if hist:
        assert np.array_equal(xp.astype(np.float32), data.np['hist'][sr].astype(np.float32)), (what, 'history frames')
    assert np.array_equal(w, data.np['w'][sr]), (what, 'labels')
    if target:
        assert np.array_equal(y, data.np['target'][sr].astype(np.float32)), (what, 'target frames')


_DATA = {}


def data_of(name, dev):
    key = name.split('-')[0]                 # the engines with and without history share their path's data set
    if key not in _DATA:
        _DATA[key] = Data(ENGINES[key], dev)
    return _DATA[key]


# ------------------------------------------------------------------------------------------------------ 1. routes --
@pytest.mark.parametrize("engine,kind", sorted(ROUTES), ids=["%s:%s" % k for k in sorted(ROUTES)])
def test_route_and_live_batch(dev, engine, kind):
    from clvae_amd.trainer import TrainStep
    e = ENGINES[engine]
    frames, rows, hist, target = KINDS[kind]
    where, left_as = ROUTES[(engine, kind)]
    data = data_of(engine, dev)
    eng = make_engine(e, dev, weights(e, 3))
    ts = TrainStep(eng, seed=SEED)
    args, kw, (idx, period, stride, offset) = data.bind_args(frames, rows, hist, target)
    ts.bind_batches(*args, **kw)
    assert ('label' if ts._label_stage() is not None else 'gather') == where
    for it in range(period + 2):             # eager, the capture, replays; past the end of the period
        ts.step()
        torch.cuda.synchronize()
        assert ('bytes' if ts._f8 is not None else 'float') == left_as, it
        sr = stage_rows(e['B'], idx, 0, (it, 0, period, stride, offset))
        assert_fed(ts, data, sr, hist, target, (engine, kind, it))
        assert all(np.isfinite(v) for v in eng.losses().values())
    assert ts._graphs is not None and int(eng.P.iterations.item()) == period + 2
    assert eng.frames_exact_bf16 == (frames != 'f32-rows') or e['model'] == 'vae'


def test_a_source_whose_rows_are_not_whole_is_refused(dev):
    """the launches read memory, not a tensor's strides: a view whose ROWS are broken up cannot be assembled and must not be
    taken for its base pointer's neighbours"""
    from clvae_amd.trainer import TrainStep
    e = ENGINES['pair']
    data = data_of('pair', dev)
    ts = TrainStep(make_engine(e, dev, weights(e, 3)), seed=SEED)
    wide = torch.zeros(data.n, e['T'], 2 * D, dtype=torch.uint8, device=dev)
    ts.bind_batches(wide[:, :, :D], wide[:, :, D:], data.w, period=PERIOD)
    with pytest.raises(ValueError, match='contiguous'):
        ts.step()


# ------------------------------------------------------------------------------------------------- 2. transitions --
# a script: ('stage', batch)   stage_batch of float rows batch * B .. of the data set
#           ('bind', frames, rows, dict(hist=, target=, period=, plan=))   bind_batches
#           ('unbind',)  ('eval',)  what Model.evaluate_device does for one chunk  ('set_weights',)  other weights, from outside
#           ('poke',)    one byte of the bound uint8 rows overwritten IN PLACE with 200
#           ('step', n)  n steps; each must have been fed the rows its cursor (or the staged batch) names.  Three where the
#                        route is new: with use_graph the first runs eagerly (TrainStep._route_changed), the second is the
#                        capture, the third a replay
#           ('expect', attribute of the engine, value)
SCRIPTS = {
    'staged-bound-staged': [('stage', 0), ('step', 1), ('stage', 1), ('step', 1),
                            ('bind', 'u8-rows', 'seq', {}), ('step', PERIOD + 1), ('unbind',),
                            ('stage', 1), ('step', 1), ('stage', 0), ('step', 1), ('stage', 1), ('step', 1)],
    'target-then-none': [('bind', 'u8-rows', 'perm', dict(target=True)), ('step', 3), ('bind', 'u8-rows', 'perm', {}), ('step', 3)],
    'float-windows-rows-float': [('bind', 'f32-rows', 'perm', {}), ('step', 3), ('expect', 'frames_exact_bf16', False),
                                 ('bind', 'u8-windows', 'perm', {}), ('step', 3), ('expect', 'frames_exact_bf16', True),
                                 ('bind', 'u8-rows', 'seq', {}), ('step', 3), ('expect', 'frames_exact_bf16', True),
                                 ('bind', 'f32-rows', 'seq', {}), ('step', 3), ('expect', 'frames_exact_bf16', False)],
    'evaluation-between-steps': [('bind', 'u8-rows', 'perm', dict(period=3)), ('step', 3), ('eval',), ('step', 4)],
    'weights-set-from-outside': [('bind', 'u8-rows', 'perm', {}), ('step', 3), ('set_weights',), ('step', 3)],
    'plan-then-none': [('bind', 'u8-rows', 'seq', dict(plan=True)), ('step', 3), ('bind', 'u8-rows', 'seq', {}), ('step', 3)],
    'binary-store-turns-loud': [('bind', 'u8-rows', 'seq', {}), ('step', 3), ('expect', 'notes_valid', True),
                                ('poke',), ('bind', 'u8-rows', 'seq', {}), ('step', 3), ('expect', 'notes_valid', False)],
}
RUNS = [(s, e) for s in SCRIPTS for e in ('pair', 'mx', 'vae')
        if not (s == 'binary-store-turns-loud' and e != 'pair')         # note lists: the pair path only (VrnnEngine.fuse_notes)
        and not (s == 'float-windows-rows-float' and e == 'vae')]       # frames_exact_bf16 is cl_vrnn's
KEY_MAPS = {10: {'A': 0, 'A-': 1, 'B-': 2, 'C': 3, 'D': 4, 'D-': 5, 'E': 6, 'E-': 7, 'F': 8, 'G': 9}, 3: {'C': 0, 'G': 1, 'D': 2},
            2: {'C': 0, 'G': 1}}      # class of a key name, per number of classes (augment.TransposePlan.build)


# A byte of 200 through freshly initialised weights drives the label head's log-variance to 18 (probed on an MI355X: wargs up to
# 17.9, kl_w 150), and the logistic-normal sample exp(mean + e^9 eps) overflows in any precision: W, and with it every loss
# behind it, is NaN -- on the device and in the fp64 oracle's formula alike.  NaN compares unequal to itself and would make the
# rest of the script vacuous, so that script starts from the same weights scaled down.
WEIGHT_SCALE = {'binary-store-turns-loud': 0.25}


def run_script(dev, engine, script, use_graph, scale=1.0):
    """-> (losses per step, live batch per step, parameters at the end, source rows per step)"""
    from clvae_amd.augment import TransposePlan
    from clvae_amd.trainer import TrainStep
    e = ENGINES[engine]
    B = e['B']
    data = Data(e, dev) if any(op[0] == 'poke' for op in script) else data_of(engine, dev)       # a poke spoils the data set
    extra = dict(fuse_notes=True) if any(op[0] == 'poke' for op in script) else {}
    eng = make_engine(e, dev, {k: v * scale for k, v in weights(e, 3).items()}, **extra)
    if extra:
        assert eng.fuse_notes
    ts = TrainStep(eng, seed=SEED, use_graph=use_graph)
    count, bound, staged = 0, None, None
    losses, lives, fed = [], [], []
    for op in script:
        if op[0] == 'stage':
            staged = np.arange(op[1] * B, (op[1] + 1) * B)
            f = data.dev['f32-rows']
            ts.stage_batch(f['cur'][staged[0]:staged[0] + B], f['hist'][staged[0]:staged[0] + B], data.w[staged[0]:staged[0] + B])
        elif op[0] == 'bind':
            o = dict(dict(hist=True, target=False, period=PERIOD, plan=False), **op[3])
            args, kw, ref = data.bind_args(op[1], op[2], o['hist'], o['target'], o['period'])
            if o['plan']:
                T = e['T']
                lab = data.np['w'].argmax(1)
                fr = [data.np['cur'].reshape(-1, T, D), data.np['hist'].reshape(-1, T, D)]
                kw['augment'] = TransposePlan.build(fr, lab, KEY_MAPS[e['C']], semitones=6, n_classes=e['C']).to(dev)
            ts.bind_batches(*args, **kw)
            bound = dict(ref=ref, step0=count, hist=o['hist'], target=o['target'], plan=o['plan'])
        elif op[0] == 'unbind':
            ts.unbind_batches()
            bound = None
        elif op[0] == 'eval':
            src = data.dev['u8-rows']
            ts.gather_batch(src['cur'], src['hist'], data.w, None, row0=B, d_target=None)
            ts.draw_noise(stream_offset=2, row0=0)
            eng.loss_and_grads(ts.X, ts.Xp, ts.w_true, ts.eps_w, ts.eps_z, need_grads=False, target=ts.Y)
        elif op[0] == 'set_weights':
            eng.P.set_weights(weights(e, 4))
        elif op[0] == 'poke':
            rows = data.dev['u8-rows']['cur']
            rows.view(-1)[3 * rows[0].numel() + 5:3 * rows[0].numel() + 6].fill_(200)      # row 3 of batch 0
            data.np['cur'][3, 5] = 200
        elif op[0] == 'expect':
            assert getattr(eng, op[1]) == op[2], op
        elif op[0] == 'step':
            for _ in range(op[1]):
                ts.step()
                torch.cuda.synchronize()
                if bound is not None:
                    idx, period, stride, offset = bound['ref']
                    sr = stage_rows(B, idx, 0, (count, bound['step0'], period, stride, offset))
                    if not bound['plan']:
                        assert_fed(ts, data, sr, bound['hist'], bound['target'], (engine, count))
                else:
                    sr = staged
                    assert_fed(ts, data, sr, True, False, (engine, count))
                fed.append(np.asarray(sr))
                losses.append(dict(eng.losses()))
                lives.append(live_batch(ts, True, bound is not None and bound['target']))
                count += 1
                assert int(eng.P.iterations.item()) == count
    if use_graph:
        assert ts._graphs is not None
    return losses, lives, {k: np.array(v) for k, v in eng.P.get_weights().items()}, fed


def oracle_follow(e, data, fed, seed):
    """the fp64 oracle's losses per step and parameters at the end for cl_vrnn steps fed the rows `fed` (the loop of
    tests/test_gpu_timed_step.py)"""
    cfg = config(e)
    B, T, C, L = e['B'], e['T'], e['C'], e['L']
    p = weights(e, 3)
    st = O.adam_wn_init(p)
    out = []
    for it, sr in enumerate(fed):
        eW = f32(OP.normal(B * (C - 1), seed, step=it, stream_id=0).reshape(B, C - 1))
        eZ = f32(OP.normal(B * T * L, seed, step=it, stream_id=1).reshape(B, T, L))
        X, Xp = data.np['cur'][sr].reshape(B, T, D).astype(np.float64), data.np['hist'][sr].reshape(B, T, D).astype(np.float64)
        ref = O.vrnn_loss_and_grads(p, cfg, X, Xp, data.np['w'][sr].astype(np.float64), eW, eZ)
        O.adam_wn_step(p, ref['grads'], st)
        out.append(ref)
    return out, p


@pytest.mark.parametrize("script,engine", RUNS, ids=["%s:%s" % r for r in RUNS])
def test_transition_graph_equals_eager(dev, script, engine):
    runs = [run_script(dev, engine, SCRIPTS[script], use_graph, WEIGHT_SCALE.get(script, 1.0)) for use_graph in (True, False)]
    (la, va, pa, fa), (lb, vb, pb, fb) = runs
    assert all(np.isfinite(v) for step in la for v in step.values())
    assert len(la) == len(lb) == sum(op[1] for op in SCRIPTS[script] if op[0] == 'step')
    for it, (a, b) in enumerate(zip(la, lb)):
        assert a == b, (it, a, b)
    for it, (a, b) in enumerate(zip(va, vb)):
        for x, y in zip(a, b):
            assert (x is None and y is None) or np.array_equal(x, y), it
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    if script == 'staged-bound-staged' and engine == 'pair':
        e = ENGINES[engine]
        refs, p = oracle_follow(e, data_of(engine, dev), fa, SEED)
        for it, ref in enumerate(refs):
            for k in ('vae', 'kl_z', 'kl_w', 'w_rec', 'total', 'elbo'):
                print("step %d %s gpu %.6f oracle %.6f" % (it, k, la[it][k], ref[k]))
                assert abs(la[it][k] - ref[k]) <= LOSS_TOL, (it, k, la[it][k], ref[k])
        worst = check_params(pa, p, len(refs), what="staged-bound-staged")
        print("parameters after %d steps: max |dw| %.2e" % (len(refs), worst))
