"""-m gpu: the thirteen entry points of csrc/smc.hip and csrc/voices.hip over the case tables of tests/filter_reference.py,
each output judged by that file against the fp64 references (smc_reference, gibbs_reference, smc_key_reference,
voices_reference, oracle.philox): widths 1 .. 200 on both sides of the group of 16, the 64-bit mask seam and the 64-note
loops, row counts around the workgroups' 4 and 16 rows, one to 1024 particles, weights that are uniform, dominated by one
particle or thousands of nats apart, a first melody of 2^35 + 7, out-of-range picks and ancestors where the kernels clamp,
NaN payloads through the gather, and every argument error the launchers name.

Buffers: every output is a helpers.Bufs buffer (NaN, FILL_U8 or -7 inside, a canary behind), every buffer a kernel updates in
place is built the same way, check_canaries() runs after every call, and every call is made twice and compared bit for bit.
A test goes through all its cases and reports every failure with the first offending element.

Bit for bit: frames, history rows, ancestors, flags, resample counts, picks, one-hot label rows, gathered payloads (as
uint32), retained paths, latents, bridges, renewed flags, pinned rows; the chain twin's x and logb against the filter's; a
not-counted pair against clv_smc_sample and clv_bernoulli_sample_clamped; with one particle logW == 0 and logZ the running
sum of ell; with uniform weights ess == P; every output after a step outside [S, S + nsteps); every other melody beside
one whose ell is NaN; a second call.

Measured on an MI355X (the module's report, -s), worst error / bound per kernel and output:
  smc_sample_kernel           ell 0.00063 (of rtol 1e-12: 6e-16 relative)
  voices_sample_kernel        ell 0.00042, logb 0.00021, the same from both entry points
  smc_resample_kernel<false>  logW 0.41, logZ 0.41, ess 0.15      smc_resample_kernel<true>  the same figures
                              (the kernel's order of sums evaluated in numpy, tests/test_filter_reference.py: 0.41, 0.40, 0.15)
  smc_init_w_kernel           logistic-normal rows 0.096 (of 16 ulp of 1.0 in float32); categorical rows bit for bit
  smc_w_posterior_kernel      0.0029 (of rtol 1e-12)
Everything listed as bit for bit was; all 162 refusals were CLV_EINVAL with every output untouched; no canary moved; no defect
was found in csrc/smc.hip or csrc/voices.hip.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import filter_reference as F
from helpers import CANARY, CANARY_U8, FILL_U8, TAIL, Bufs

pytestmark = pytest.mark.gpu

_REPORT = {}
NAN = float('nan')


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    yield torch.device("cuda:0")
    for k in sorted(_REPORT):
        print("\n%-28s worst error / bound: %s" % (k, ", ".join("%s %.3g" % kv for kv in sorted(_REPORT[k].items()))
                                                      or "every output bit for bit"), end="")
    print()


class Cases:
    """runs the cases of a test, collects the ratios per kernel and every failure (tests/test_gpu_seq.py's collector)"""

    def __init__(self):
        self.fails, self.n = [], 0

    def run(self, kernel, name, fn):
        self.n += 1
        rep = _REPORT.setdefault(kernel, {})
        try:
            for k, v in fn().items():
                rep[k] = max(rep.get(k, 0.0), v)
            return True
        except AssertionError as e:
            rep['FAILED'] = rep.get('FAILED', 0) + 1
            self.fails.append("%s %s: %s" % (kernel, name, e))
            return False

    def done(self):
        assert self.n > 0
        assert not self.fails, "%d failures:\n%s" % (len(self.fails), "\n".join(self.fails[:40]))


class Outs(Bufs):
    """helpers.Bufs plus what these kernels need: int32 outputs (-7 inside) and in-place buffers of any dtype"""

    def i32(self, *shape):
        n = int(np.prod(shape))
        raw = torch.full((n + TAIL,), int(CANARY), dtype=torch.int32, device=self.dev)
        raw[:n] = F.I32_FILL
        self.all.append((raw, n, shape, 0, int(CANARY)))
        return raw[:n].view(*shape)

    def inplace(self, a):
        """Bufs.inp for any dtype, bit for bit: a buffer the kernel reads and overwrites"""
        a = np.array(a)
        canary = CANARY_U8 if a.dtype == np.uint8 else int(CANARY) if a.dtype.kind == 'i' else CANARY
        raw = torch.full((a.size + TAIL,), canary, dtype=torch.from_numpy(a).dtype, device=self.dev)
        raw[:a.size] = torch.as_tensor(a.reshape(-1), device=self.dev)
        self.all.append((raw, a.size, a.shape, 0, canary))
        return raw[:a.size].view(*a.shape)


def T(dev, a):
    return None if a is None else torch.as_tensor(np.array(a), device=dev)


def N(x):
    return None if x is None else x.cpu().numpy()


def counter(dev, c):
    return torch.full((1,), int(c), dtype=torch.int32, device=dev)


def twice(name, fn):
    """two calls of fn() -> {output: array, list of arrays or None}, the same bits"""
    a, b = fn(), fn()
    for k in a:
        for j, (x, y) in enumerate(zip(*[v if isinstance(v, list) else [v] for v in (a[k], b[k])])):
            if x is not None:
                F.check_bits("%s %s[%d], a second call" % (name, k, j), y, x)
    return a


F64, I32, U8 = torch.float64, torch.int32, torch.uint8


# ------------------------------------------------------------------------------------------------------ clv_smc_sample --
def sample_once(dev, c, d, k):
    from clvae_amd import ops
    B = Outs(dev)
    R, D, n = c['R'], c['D'], c['nsteps']
    x, ell, hist = B.out(R, D), B.out(R, dtype=F64), B.out(n, R, D, dtype=U8)
    ops.smc_sample(R, D, c['P'], n, c['S'], d['xhat'], d['u'], d['roll'], counter(dev, c['S'] + k), x, ell, hist)
    torch.cuda.synchronize()
    B.check_canaries()
    return dict(x=N(x), ell=N(ell), hist=N(hist))


def test_smc_sample_table(dev):
    run = Cases()
    for i, c in enumerate(F.SAMPLE):
        inp = F.sample_inputs(i)
        d = {k: T(dev, v) for k, v in inp.items()}
        for k in (0, 1, c['nsteps'] - 1, -1, c['nsteps']):
            name = "%s k=%d" % (c['name'], k)
            run.run('smc_sample_kernel', name, lambda: F.judge_sample(name, c, inp, k, twice(name, lambda: sample_once(dev, c, d, k))))
    run.done()


# ------------------------------------------------------------------------------------------- the two voices entry points --
def voices_once(dev, c, d, k, smc):
    from clvae_amd import ops
    B = Outs(dev)
    R, D, n, S = c['R'], c['D'], c['nsteps'], c['S']
    x, logb = B.out(R, D), B.out(R, dtype=F64)
    if smc:
        ell, hist = B.out(R, dtype=F64), B.out(n, R, D, dtype=U8)
        ops.smc_sample_voices(R, D, c['P'], n, S, d['xhat'], d['u'], d['roll'], d['voices'], counter(dev, S + k), x, ell, hist, logb)
    else:
        ops.bernoulli_sample_voices(R * D, D, n, S, d['xhat'], d['u'], d['roll'], d['voices'], counter(dev, S + k), x, logb)
    torch.cuda.synchronize()
    B.check_canaries()
    return dict(x=N(x), logb=N(logb), **(dict(ell=N(ell), hist=N(hist)) if smc else {}))


def twins_once(dev, c, d, k):
    """clv_smc_sample and clv_bernoulli_sample_clamped on the same rows (an all-free roll where the case has none)"""
    from clvae_amd import ops
    R, D, P, n, S = c['R'], c['D'], c['P'], c['nsteps'], c['S']
    roll = d['roll'] if d['roll'] is not None else torch.full((R // P, n, D), F.FREE, dtype=U8, device=dev)
    got = sample_once(dev, dict(c), dict(d, roll=roll), k)
    B = Outs(dev)
    xc = B.out(R, D)
    ops.bernoulli_sample_clamped(R * D, D, n, S, d['xhat'], d['u'], roll.repeat_interleave(P, 0).contiguous(), counter(dev, S + k), xc)
    torch.cuda.synchronize()
    B.check_canaries()
    return got, N(xc)


def test_voices_table(dev):
    run = Cases()
    for i, c in enumerate(F.VOICES):
        inp = F.voices_inputs(i)
        d = {k: T(dev, v) for k, v in inp.items()}
        for k in (0, c['nsteps'] - 1, -1, c['nsteps']):
            name = "%s k=%d" % (c['name'], k)

            def one():
                got = twice(name, lambda: voices_once(dev, c, d, k, True))
                rep = F.judge_voices(name, c, inp, k, got)
                if c['P'] == 1:                           # the chain's twin: the same frame, the same log B[0][0]
                    chain = twice(name + " chain", lambda: voices_once(dev, c, d, k, False))
                    F.check_bits(name + " x, chain twin", chain['x'], got['x'], ('row', 'note'))
                    F.check_bits(name + " logb, chain twin", chain['logb'], got['logb'], ('row',))
                    rep = {'chain ' + kk: v for kk, v in F.judge_voices(name + " chain", c, inp, k, chain).items()} | rep
                if k == 0:                                # a pair that is not lo <= hi <= 15 is the twins' draw and weight
                    free = F.voices_rows(c, inp, k)[2]
                    plain, xc = twins_once(dev, c, d, k)
                    for key in ('x', 'ell'):
                        F.check_bits("%s %s of the free rows, clv_smc_sample" % (name, key), got[key][free], plain[key][free])
                    F.check_bits(name + " hist of the free rows, clv_smc_sample", got['hist'][k][free], plain['hist'][k][free])
                    F.check_bits(name + " x of the free rows, clv_bernoulli_sample_clamped", got['x'][free], xc[free])
                return rep
            run.run('voices_sample_kernel', name, one)
    run.done()


# ------------------------------------------------------------------------- clv_smc_resample, clv_smc_resample_conditional --
RS_OUT = ('logW', 'logZ', 'ess', 'nres', 'flag', 'anc')


def resample_run(dev, c, conditional, ell):
    """the whole script from poisoned state (NaN logW and logZ, -5 resample counts), then two steps outside the range"""
    from clvae_amd import ops
    fn = ops.smc_resample_conditional if conditional else ops.smc_resample
    G, P, n, S = c['G'], c['P'], c['nsteps'], c['S']
    R = G * P
    B = Outs(dev)
    b = dict(logW=B.inplace(np.full(R, np.nan)), logZ=B.inplace(np.full(G, np.nan)), ess=B.out(G, n, dtype=F64),
             nres=B.inplace(np.full(G, -5, np.int32)), flag=B.i32(G), anc=B.i32(n, R))
    ell_d = T(dev, ell.reshape(n, R))
    steps = []
    for k in list(range(n)) + [-1, n]:
        fn(G, P, n, S, c['seed'], c['m0'], c['tau'], ell_d[max(0, min(k, n - 1))], b['logW'], b['logZ'], b['ess'], b['nres'],
           b['flag'], b['anc'], counter(dev, S + k))
        torch.cuda.synchronize()
        B.check_canaries()
        got = {key: N(b[key]) for key in RS_OUT}
        if 0 <= k < n:
            steps.append(got)
        else:
            for key in RS_OUT:
                F.check_bits("%s %s after step S%+d, outside the range" % (c['name'], key, k), got[key], steps[-1][key])
    return steps


def steps_as_dict(steps):
    return {key: [s[key] for s in steps] for key in RS_OUT}


@pytest.mark.parametrize("conditional", [False, True], ids=['systematic', 'conditional'])
def test_smc_resample_table(dev, conditional):
    run = Cases()
    kernel = 'smc_resample_kernel<%s>' % ('true' if conditional else 'false')
    for i, c in enumerate(F.RESAMPLE):
        ell = F.resample_script(i)

        def one():
            steps = twice(c['name'], lambda: steps_as_dict(resample_run(dev, c, conditional, ell)))
            steps = [{key: steps[key][k] for key in RS_OUT} for k in range(c['nsteps'])]
            rep = F.judge_resample(c['name'], c, conditional, ell, steps)
            if c['G'] >= 2 and i % 3 == 0:                # a NaN in melody 1's ell from step 2 on: no other melody moves
                bad = np.array(ell)
                bad[2:, 1, c['P'] // 2] = np.nan
                other = np.arange(c['G']) != 1
                rows = np.repeat(other, c['P'])
                for k, (s, t) in enumerate(zip(steps, resample_run(dev, c, conditional, bad))):
                    for key in RS_OUT:
                        sel = (lambda a: a[..., rows]) if key in ('logW', 'anc') else (lambda a: a[other])
                        F.check_bits("%s step %d %s beside a NaN melody" % (c['name'], k, key), sel(t[key]), sel(s[key]))
            return rep
        run.run(kernel, c['name'], one)
    run.done()


# ------------------------------------------------------------------------------------------------------ clv_smc_gather --
def gather_once(dev, c, inp, k):
    from clvae_amd import ops
    B = Outs(dev)
    bufs = [B.inp(b.view(np.float32)) for b in inp['bufs']]
    g = ops.SmcGather(c['R'], c['P'], c['nsteps'], c['S'], bufs)
    g.scratch = B.out(sum(c['widths']) * c['R'])
    g(T(dev, inp['anc']), T(dev, inp['flag']), counter(dev, c['S'] + k))
    torch.cuda.synchronize()
    B.check_canaries()
    return dict(bufs=[N(b).view(np.uint32) for b in bufs])


def test_smc_gather_table(dev):
    run = Cases()
    for i, c in enumerate(F.GATHER):
        inp = F.gather_inputs(i)
        for k in (c['k'], 0, -1, c['nsteps']):
            name = "%s k=%d" % (c['name'], k)
            run.run('smc_gather_kernel', name,
                    lambda: F.judge_gather(name, c, inp, k, twice(name, lambda: gather_once(dev, c, inp, k))['bufs']))
    run.done()


# --------------------------------------------------------------------------------------------------- clv_smc_backtrack --
def backtrack_once(dev, c, d):
    from clvae_amd import ops
    B = Outs(dev)
    G, P, n, D, n_out = c['G'], c['P'], c['nsteps'], c['D'], c['n_out']
    Xs = B.out(G, n_out, n, D)
    picks = B.i32(G, n_out) if c['picks'] else None
    ops.smc_backtrack(G, P, n, D, n_out, c['seed'], c['m0'], c['step'], d['logW'], d['anc'], d['hist'], Xs, picks)
    torch.cuda.synchronize()
    B.check_canaries()
    return dict(Xs=N(Xs), picks=N(picks))


def test_smc_backtrack_table(dev):
    run = Cases()
    for i, c in enumerate(F.BACKTRACK):
        inp = F.backtrack_inputs(i)
        d = {k: T(dev, v) for k, v in inp.items()}
        run.run('smc_backtrack_kernel', c['name'],
                lambda: F.judge_backtrack(c['name'], c, inp, twice(c['name'], lambda: backtrack_once(dev, c, d))))
    run.done()


# ---------------------------------------------------------------------- clv_smc_backtrack_path, the pins, clv_smc_take_w --
def path_once(dev, c, d):
    from clvae_amd import ops
    B = Outs(dev)
    G, P, S, L, D, n = c['G'], c['P'], c['S'], c['L'], c['D'], c['nsteps']
    x_ref, z_ref, renewed = B.out(G, n, D, dtype=U8), B.out(G, S + n, L), B.out(G, n, dtype=U8)
    b_ref = B.out(G, D) if S else None
    ops.smc_backtrack_path(G, P, n, S, D, L, d['picks'], d['anc'], d['hist'], d['zhist'], d['brows'] if S else None, x_ref,
                           z_ref, b_ref, renewed)
    torch.cuda.synchronize()
    B.check_canaries()
    return dict(x_ref=N(x_ref), z_ref=N(z_ref), renewed=N(renewed), bridge_ref=N(b_ref))


def test_smc_backtrack_path_table(dev):
    run = Cases()
    for i, c in enumerate(F.PATH):
        inp = F.path_inputs(i)
        d = {k: T(dev, v) for k, v in inp.items()}
        run.run('smc_backtrack_path_kernel', c['name'],
                lambda: F.judge_path(c['name'], c, inp, twice(c['name'], lambda: path_once(dev, c, d))))
    run.done()


def pin_once(dev, c, inp, d, step, with_bridge):
    from clvae_amd import ops
    B = Outs(dev)
    G, P, S, L, D, n = c['G'], c['P'], c['S'], c['L'], c['D'], c['nsteps']
    z, x, hist = B.inp(inp['z0']), B.inp(inp['x0']), B.inplace(inp['h0'])
    ops.smc_pin_z(G, P, L, S + n, d['z_ref'], counter(dev, step), z)
    ops.smc_pin_frame(G, P, D, n, S, d['x_ref'], d['bridge'] if with_bridge else None, counter(dev, step), x, hist)
    torch.cuda.synchronize()
    B.check_canaries()
    return dict(z=N(z), x=N(x), hist=N(hist))


def test_smc_pin_tables(dev):
    run = Cases()
    for i, c in enumerate(F.PIN):
        inp = F.pin_inputs(i)
        d = {k: T(dev, v) for k, v in inp.items()}
        for step in range(-1, c['S'] + c['nsteps'] + 2):
            for with_bridge in ((True, False) if c['S'] and step == c['S'] - 1 else (bool(c['S']),)):
                name = "%s step %d bridge %s" % (c['name'], step, with_bridge)
                run.run('smc_pin_kernels', name, lambda: F.judge_pin(
                    name, c, inp, step, with_bridge, twice(name, lambda: pin_once(dev, c, inp, d, step, with_bridge))))
    run.done()


def test_smc_take_w_table(dev):
    from clvae_amd import ops
    run = Cases()
    for i, c in enumerate(F.TAKE_W):
        inp = F.take_w_inputs(i)
        d = {k: T(dev, v) for k, v in inp.items()}

        def once():
            B = Outs(dev)
            w_out = B.out(c['G'], c['n_out'], c['C'])
            ops.smc_take_w(c['G'], c['P'], c['C'], c['n_out'], d['picks'], d['wr'], w_out)
            torch.cuda.synchronize()
            B.check_canaries()
            return dict(w_out=N(w_out))
        run.run('smc_take_w_kernel', c['name'], lambda: F.judge_take_w(c['name'], c, inp, twice(c['name'], once)))
    run.done()


# -------------------------------------------------------------------------------- clv_smc_init_w, clv_smc_w_posterior --
def test_smc_init_w_table(dev):
    from clvae_amd import ops
    run = Cases()
    for i, c in enumerate(F.INIT_W):
        inp = F.init_w_inputs(i)
        d = {k: T(dev, v) for k, v in inp.items()}

        def once():
            B = Outs(dev)
            wr = B.out(c['G'] * c['P'], c['C'])
            ops.smc_init_w(c['G'], c['P'], c['C'], c['mode'], c['seed'], c['m0'], d.get('probs'), d.get('mean'), d.get('log_var'), wr)
            torch.cuda.synchronize()
            B.check_canaries()
            return dict(wr=N(wr))
        run.run('smc_init_w_kernel', c['name'], lambda: F.judge_init_w(c['name'], c, inp, twice(c['name'], once)))
    run.done()


def test_smc_w_posterior_table(dev):
    from clvae_amd import ops
    run = Cases()
    for i, c in enumerate(F.POSTERIOR):
        inp = F.posterior_inputs(i)
        d = {k: T(dev, v) for k, v in inp.items()}
        G, P, Cn, n, S = c['G'], c['P'], c['C'], c['nsteps'], c['S']
        written = (0, 3, n - 1)

        def once():
            B = Outs(dev)
            out = B.inplace(np.full((G, n, Cn), -7.0))
            for step in (0, S - 1, S + n) + tuple(S + k for k in written):     # a seed step, the bridge, past the end
                ops.smc_w_posterior(G, P, Cn, n, S, d['logW'], d['wr'], counter(dev, step), out)
            torch.cuda.synchronize()
            B.check_canaries()
            return dict(out=N(out))
        run.run('smc_w_posterior_kernel', c['name'], lambda: F.judge_posterior(c['name'], c, inp, written, twice(c['name'], once)))
    run.done()


# ------------------------------------------------------------------------------------------------------------ refusals --
def test_c_abi_refusals(dev):
    """every argument error the thirteen launchers name is CLV_EINVAL, raised as ops.check raises it, and leaves every output
    as it was; the unchanged arguments are accepted (last, on the same buffers)"""
    from clvae_amd import _lib, ops
    lib = _lib.lib()
    G, P, D, n, S, L, Cn, n_out = 2, 3, 88, 2, 1, 2, 4, 2
    R, Tn = G * P, S + n
    B = Outs(dev)
    poisoned = []

    def out(*shape, dtype=None):
        v = B.i32(*shape) if dtype == I32 else B.out(*shape, dtype=dtype)
        poisoned.append((v, F.I32_FILL if dtype == I32 else FILL_U8 if dtype == U8 else NAN))
        return v
    rng = np.random.default_rng(0)
    f32 = lambda *s: T(dev, rng.random(s).astype(np.float32))
    p, u = f32(R, D), f32(R, D)
    roll = T(dev, np.full((G, n, D), F.FREE, np.uint8))
    voices = T(dev, np.broadcast_to(np.array([1, 4], np.uint8), (G, n, 2)))
    voices_rows = T(dev, np.broadcast_to(np.array([1, 4], np.uint8), (R, n, 2)))
    ctr = counter(dev, S)
    ell_in = T(dev, -rng.random(R))
    anc = T(dev, np.tile(np.arange(R, dtype=np.int32), (n, 1)))
    flag = T(dev, np.ones(G, np.int32))
    hist_in = T(dev, (rng.random((n, R, D)) < 0.3).astype(np.uint8))
    zhist, brows = f32(Tn, R, L), f32(R, D)
    lw = T(dev, np.full((G, P), -np.log(P)))
    picks1, picks2 = T(dev, np.zeros(G, np.int32)), T(dev, np.zeros((G, n_out), np.int32))
    wr_in = f32(R, Cn)
    probs = T(dev, np.full((G, Cn), 1.0 / Cn))
    mean, lv = f32(G, Cn - 1), f32(G, Cn - 1)
    z_ref, x_ref_in, bridge = f32(G, Tn, L), T(dev, np.zeros((G, n, D), np.uint8)), f32(G, D)
    gbufs = [out(R, 7), out(R, 64)]
    two = (C.c_void_p * 2)(*[b.data_ptr() for b in gbufs])
    nine = (C.c_void_p * 9)(*[gbufs[i % 2].data_ptr() for i in range(9)])
    hole = (C.c_void_p * 2)(gbufs[0].data_ptr(), None)
    w_ok, w_zero, w_nine = (C.c_int * 2)(7, 64), (C.c_int * 2)(7, 0), (C.c_int * 9)(*([7, 64] * 5)[:9])
    as_p = lambda a: C.cast(a, C.c_void_p)

    resample = dict(G=G, P=P, nsteps=n, S=S, seed=5, m0=0, tau=0.5, ell=ell_in, logW=out(R, dtype=F64), logZ=out(G, dtype=F64),
                    ess=out(G, n, dtype=F64), nres=out(G, dtype=I32), flag=out(G, dtype=I32), anc=out(n, R, dtype=I32),
                    step_dev=ctr)
    resample_bad = ([dict(P=1025), dict(P=0), dict(G=0), dict(nsteps=0), dict(S=-1), dict(m0=-1), dict(tau=-0.1), dict(tau=1.1),
                     dict(tau=NAN)] + [{k: None} for k in ('ell', 'logW', 'logZ', 'ess', 'nres', 'flag', 'anc', 'step_dev')])
    dims = lambda *names: [{k: 0} for k in names]
    nulls = lambda *names: [{k: None} for k in names]
    specs = [
        ("clv_smc_sample", dict(R=R, D=D, P=P, nsteps=n, S=S, p=p, u=u, clamp=roll, step_dev=ctr, x=out(R, D),
                                ell=out(R, dtype=F64), hist=out(n, R, D, dtype=U8)),
         dims('R', 'D', 'P', 'nsteps') + [dict(P=4), dict(S=-1)] + nulls('p', 'u', 'clamp', 'step_dev', 'x', 'ell', 'hist')),
        ("clv_smc_resample", resample, resample_bad),
        ("clv_smc_resample_conditional", dict(resample), resample_bad),
        ("clv_smc_pin_z", dict(G=G, P=P, L=L, T=Tn, z_ref=z_ref, step_dev=ctr, z=out(R, L)),
         dims('G', 'P', 'L', 'T') + nulls('z_ref', 'step_dev', 'z')),
        ("clv_smc_pin_frame", dict(G=G, P=P, D=D, nsteps=n, S=S, x_ref=x_ref_in, bridge=bridge, step_dev=ctr, x=out(R, D),
                                   hist=out(n, R, D, dtype=U8)),
         dims('G', 'P', 'D', 'nsteps') + [dict(S=-1)] + nulls('x_ref', 'step_dev', 'x', 'hist')),
        ("clv_smc_backtrack_path", dict(G=G, P=P, nsteps=n, S=S, D=D, L=L, picks=picks1, anc=anc, hist=hist_in, zhist=zhist,
                                        bridge_rows=brows, x_ref=out(G, n, D, dtype=U8), z_ref=out(G, Tn, L),
                                        bridge_ref=out(G, D), renewed=out(G, n, dtype=U8)),
         dims('G', 'P', 'nsteps', 'D', 'L') + [dict(S=-1), dict(bridge_ref=None), dict(bridge_rows=None)] +
         nulls('picks', 'anc', 'hist', 'zhist', 'x_ref', 'z_ref', 'renewed')),
        ("clv_smc_gather", dict(R=R, P=P, nsteps=n, S=S, nbuf=2, bufs=as_p(two),
                                widths=as_p(w_ok), scratch=out(R * 71), anc=anc, flag=flag, step_dev=ctr),
         dims('R', 'P', 'nsteps', 'nbuf') + [dict(P=4), dict(S=-1), dict(nbuf=9, bufs=as_p(nine), widths=as_p(w_nine)),
                                             dict(widths=as_p(w_zero)), dict(bufs=as_p(hole))] +
         nulls('bufs', 'widths', 'scratch', 'anc', 'flag', 'step_dev')),
        ("clv_smc_backtrack", dict(G=G, P=P, nsteps=n, D=D, n_out=n_out, seed=5, m0=0, step=7, logW=lw, anc=anc, hist=hist_in,
                                   Xs=out(G, n_out, n, D), picks=out(G, n_out, dtype=I32)),
         dims('G', 'P', 'nsteps', 'D', 'n_out') + [dict(P=1025), dict(m0=-1), dict(step=-1)] + nulls('logW', 'anc', 'hist', 'Xs')),
        ("clv_smc_init_w", dict(G=G, P=P, C=Cn, mode=0, seed=5, m0=0, probs=probs, mean=mean, log_var=lv, wr=out(R, Cn)),
         dims('G', 'P') + [dict(P=1025), dict(C=1), dict(C=33), dict(m0=-1), dict(mode=2), dict(mode=-1), dict(probs=None),
                           dict(mode=1, mean=None), dict(mode=1, log_var=None), dict(wr=None)]),
        ("clv_smc_w_posterior", dict(G=G, P=P, C=Cn, nsteps=n, S=S, logW=lw, wr=wr_in, step_dev=ctr, out=out(G, n, Cn, dtype=F64)),
         dims('G', 'P', 'nsteps') + [dict(P=1025), dict(C=1), dict(C=33), dict(S=-1)] + nulls('logW', 'wr', 'step_dev', 'out')),
        ("clv_smc_take_w", dict(G=G, P=P, C=Cn, n_out=n_out, picks=picks2, wr=wr_in, w_out=out(G, n_out, Cn)),
         dims('G', 'P', 'n_out') + [dict(P=1025), dict(C=1), dict(C=33)] + nulls('picks', 'wr', 'w_out')),
        ("clv_bernoulli_sample_voices", dict(n=R * D, D=D, nsteps=n, S=S, p=p, u=u, clamp=None, voices=voices_rows, step_dev=ctr,
                                             x=out(R, D), logb=out(R, dtype=F64)),
         dims('n', 'D', 'nsteps') + [dict(D=129, n=R * 129), dict(n=R * D + 1), dict(S=-1)] + nulls('p', 'u', 'voices', 'step_dev', 'x')),
        ("clv_smc_sample_voices", dict(R=R, D=D, P=P, nsteps=n, S=S, p=p, u=u, clamp=roll, voices=voices, step_dev=ctr, x=out(R, D),
                                       ell=out(R, dtype=F64), hist=out(n, R, D, dtype=U8), logb=out(R, dtype=F64)),
         dims('R', 'D', 'P', 'nsteps') + [dict(D=129), dict(P=4), dict(S=-1)] + nulls('p', 'u', 'voices', 'step_dev', 'x', 'ell', 'hist')),
    ]

    def call(name, args):
        conv = [ops._ptr(v) if isinstance(v, torch.Tensor) else v for v in args.values()]
        return getattr(lib, name)(*conv, ops._stream())
    run = Cases()
    for name, good, bad in specs:
        for change in bad:
            def one():
                try:
                    ops.check(call(name, dict(good, **change)), name)
                except _lib.ClvError as e:
                    assert '(-1)' in str(e), "%s %r: %s" % (name, change, e)
                else:
                    raise AssertionError("%s %r: accepted" % (name, change))
                torch.cuda.synchronize()
                for v, fill in poisoned:
                    F.untouched("%s %r: an output" % (name, change), N(v), fill)
                B.check_canaries()
                return {}
            run.run('refusals', "%s %r" % (name, change), one)
    run.done()
    print("\n%d refusals over %d entry points" % (run.n, len(specs)), end="")
    for name, good, _ in specs:                           # the arguments every refusal started from are accepted
        assert call(name, good) == 0, name
    torch.cuda.synchronize()
    B.check_canaries()
    assert len(specs) == 13
