"""-m gpu: clv_lstm_seq_fwd / clv_lstm_seq_bwd / clv_lstm_seq_bwd_z (csrc/lstm.hip, csrc/lstm_any.hip) against the fp64 reference
of tests/seq_reference.py over its case tables: EVERY stored value of every step within its own bound -- a saving forward step
by step from the device's own previous state (and against the free recurrence's running bound), the backward on the device
forward's records and on crafted ones with every hard-sigmoid kink decided exactly, dzsum and dZ against the device's own dz --
and bit for bit where the result is exact: the impulse probes' pre-activations, the selection probes' dZ, hT / cT, bwd_z
against bwd, a second call.

Buffers (tests/seq_worker.py): every output a helpers.Bufs buffer (NaN inside, a canary tail, the canary in the lddz padding),
every input inside NaN, check_canaries() after every call.  A test goes through all its cases and reports every failure with
the first offending (row, step, gate, unit).  The KS = 8 forward instances run in one fresh child process with CLV_LSTM_KS=8.

Measured on an MI355X (the module's report, -s), worst error / bound per kernel and output (the honest fp32 evaluation of
tests/test_seq_reference.py stays below 0.5 everywhere):
  lstm_fwd_kernel      z / g 0.27, c 0.27, h 0.23 step by step, the same against the free recurrence; inference h 0.23,
                       cT 0.045; KS = 8: 0.16, 0.14, 0.23; impulse z_i, z_f, z_o bit for bit, g 0.33
  lstm_bwd_kernel      dz 0.32, dzsum 0.65, dZ 0.007 (records of the device forward, crafted records, selection probes);
                       bwd_z's dz and dzsum bit for bit those of bwd; selection dZ bit for bit
  lstm_any_fwd_kernel  z / g 0.23, c 0.23, h 0.15; impulse bit for bit, g 0.33      lstm_any_bwd_kernel  dz 0.29, dzsum 0.61
The derivative at z = -2.5 is 0 in every instance (the fused 0.2f z + 0.5f is -7.45e-9 there): S.DEVICE_TIE = 'fma'.  hT / cT
are the last stored step bit for bit, a second call gives the same bits, no canary moved; no defect was found.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import seq_reference as S
import seq_worker as W

pytestmark = pytest.mark.gpu

_REPORT = {}
f32, f64 = np.float32, np.float64
U88 = S.make_U(np.random.default_rng(5), 88)          # the recurrent kernel of the crafted records


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    yield torch.device("cuda:0")
    for k in sorted(_REPORT):
        print("\n%-24s worst error / bound: %s" % (k, ", ".join("%s %.3g" % kv for kv in sorted(_REPORT[k].items()))), end="")
    print()


class Cases:
    """runs the cases of a test, collects the ratios per kernel and every failure"""

    def __init__(self):
        self.fails, self.n = [], 0

    def run(self, kernel, name, fn):
        """fn() -> {output: ratio}; an AssertionError (a bound, a canary, a second call) is a failure of this case"""
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


def fwd_kernel(c):
    return 'lstm_any_fwd_kernel' if c['H'] != 88 or c.get('force') else 'lstm_fwd_kernel'


def bwd_kernel(c):
    return 'lstm_any_bwd_kernel' if c['H'] != 88 or c.get('force') else 'lstm_bwd_kernel'


def same_bits(name, a, b, H):
    for k in ('dz', 'dzsum'):
        S.check_bits("%s %s, bwd_z against bwd" % (name, k), a[k], b[k], H)


def forward_and_judge(dev, c, inp, name, state_inplace=False):
    got = W.twice(name, lambda: W.forward_once(torch, dev, c, inp, state_inplace))
    return got, S.judge_forward(name, inp, got)


# ------------------------------------------------------------------------------------------------------------ forward --
def test_lstm88_forward_table(dev):
    run = Cases()
    for c in S.CASES['fwd88']:
        inp = S.forward_inputs(c)
        run.run('lstm_fwd_kernel', repr(c), lambda: forward_and_judge(dev, c, inp, "fwd88 %r" % (c,))[1])
    run.done()


def test_impulse_probes(dev):
    """h0[b] = scale e_b, xproj = 0, T = 1: the stored z_i, z_f, z_o of row b are scale U[b] bit for bit, element by element
    of U: every k-slice, lane group and surplus group of lstm.hip, every slice and owner thread of lstm_any.hip"""
    run = Cases()
    for c in S.IMPULSE_88 + S.IMPULSE_ANY:
        for scale in S.IMPULSE_SCALES:
            inp = S.impulse_inputs(c, scale)
            name = "impulse %r x %g" % (c, scale)

            def one():
                got, rep = forward_and_judge(dev, c, inp, name)
                rep.update(S.judge_impulse(name, inp, got, scale))
                return {'impulse ' + k: v for k, v in rep.items()}
            run.run(fwd_kernel(c), name, one)
    run.done()


def test_the_stateful_single_step(dev):
    """T = 1, no cs / gates, hT and cT in the buffers of h0 and c0: what the host sampling loops call"""
    run = Cases()
    for c in S.STEP_CASES:
        inp = S.forward_inputs(c)
        name = "step %r" % (c,)
        run.run(fwd_kernel(c), name, lambda: {'step ' + k: v for k, v in forward_and_judge(dev, c, inp, name, True)[1].items()})
    run.done()


# ----------------------------------------------------------------------------------------------------------- backward --
def backward_and_judge(dev, c, name, rec, dhs, Uw, c0, Kz=None, pad=0, sum_terms=True, tie=None):
    """bwd, and with Kz bwd_z too: each twice, each judged, bwd_z's dz and dzsum bit for bit bwd's"""
    H, force = c['H'], c.get('force', 0)
    got = W.twice(name, lambda: W.backward_once(torch, dev, rec, dhs, Uw, c0, c['gate_act'], force=force))
    rep, _ = S.judge_backward(name, rec, dhs, Uw, c0, c['gate_act'], got, tie=tie, sum_terms=sum_terms)
    if Kz is not None:
        gz = W.twice(name + " bwd_z", lambda: W.backward_once(torch, dev, rec, dhs, Uw, c0, c['gate_act'], Kz, pad, force))
        same_bits(name, gz, got, H)
        rz, _ = S.judge_backward(name + " bwd_z", rec, dhs, Uw, c0, c['gate_act'], gz, Kz, tie=tie, sum_terms=sum_terms)
        rep['dZ'] = rz['dZ']
        got = gz
    return got, rep


def table_backward(dev, table):
    run = Cases()
    for c in S.CASES[table]:
        inp = S.forward_inputs(c)
        name = "%s %r" % (table, c)
        rec = {}

        def forward():
            got, rep = forward_and_judge(dev, c, inp, name)
            rec.update(got)
            return rep
        if not run.run(fwd_kernel(c), name, forward):
            continue
        d = S.backward_inputs(c)
        run.run(bwd_kernel(c), name, lambda: backward_and_judge(dev, c, name, rec, d['dhs'], inp['U'], inp['c0'], d.get('Kz'),
                                                                c.get('pad', 0))[1])
    run.done()


def test_lstm88_backward_table(dev):
    """on the device forward's own records; every case through clv_lstm_seq_bwd and clv_lstm_seq_bwd_z"""
    table_backward(dev, 'bwd88')


def test_any_width_table(dev):
    """lstm_any.hip at every slice count and every count of units per owner thread, forward and backward"""
    table_backward(dev, 'any')


def test_crafted_records(dev):
    """records no forward made: the kink ladder in every gate block at the first, the last and the surplus lane groups,
    g = +-1, |c| up to 100, dhs = 0, with and without c0"""
    run = Cases()
    for c in S.CRAFTED:
        rec, dhs, c0 = S.crafted_records(c)
        name = "crafted %r" % (c,)

        def one():
            Kz = None if c['force'] else S.backward_inputs(dict(c, nz=5))['Kz']
            got, rep = backward_and_judge(dev, c, name, rec, dhs, U88, c0, Kz, 3)
            if c['dh0']:
                assert not got['dz'].any() and not got['dzsum'].any(), name + ": dhs = 0 gives dz = 0"
            return {'crafted ' + k: v for k, v in rep.items()}
        run.run(bwd_kernel(c), name, one)
    run.done()


def test_backward_selection_probes(dev):
    """U with a single 1.0 per row: dh_0 picks single entries of dz_1, no summation term in the bound of dz_0.
    Kz a 0/1 matrix: dZ[:, l] is dz[:, sel[l]] at every step, all 352 columns in nine launches."""
    run = Cases()
    for c in S.SELECT_BWD:
        rec, dhs, Uw, _ = S.select_bwd_inputs(c)
        name = "select %r" % (c,)
        run.run(bwd_kernel(c), name, lambda: {'select ' + k: v for k, v in
                                              backward_and_judge(dev, c, name, rec, dhs, Uw, None, sum_terms=False)[1].items()})
    for c in S.SELECT_Z:
        rec, dhs, _ = S.crafted_records(dict(H=88, B=c['B'], T=c['T'], gate_act=c['gate_act'], c0=0, dh0=0, plain=1))
        Kz, sel = S.select_z(c)
        name = "select_z %r" % (c,)

        def one():
            got, rep = backward_and_judge(dev, c, name, rec, dhs, U88, None, Kz, 0)
            # + 0: a -0 of dz arrives as the +0 that 0 + (-0) 1 is
            S.check_bits(name + " dZ", got['dZ'] + f32(0), got['dz'][:, :, sel] + f32(0), 88)
            return {}
        run.run('lstm_bwd_kernel', name, one)
    run.done()


def test_the_tie_at_minus_2p5(dev):
    """z = -2.5 in the blocks i, f, o: separate rounding gives y = 0.2f z + 0.5f = 0 (the gradient passes), the fused
    multiply-add -7.45e-9 (clipped, gradient 0).  What the device takes is read off dz; it is the same in every
    lstm_bwd_kernel instance that has a kink (1, 2, 4 rows per workgroup, with and without latents) and in
    lstm_any_bwd_kernel, it is S.DEVICE_TIE, and the forward's clip agrees: every gate at z = -2.5 is 0."""
    seen = {}
    for c in S.TIE_CASES:
        rec, dhs, c0 = S.crafted_records(c)
        Kz = S.backward_inputs(dict(c, nz=9))['Kz']
        for with_z in ((0, 1) if not c['force'] else (0,)):
            got = W.backward_once(torch, dev, rec, dhs, U88, c0, S.HARD, Kz if with_z else None, 0, c['force'])
            fits = []
            for tie in ('separate', 'fma'):
                want, bound, flags = S.backward(rec, dhs, U88, c0, S.HARD, tie=tie)['dz']
                assert flags.sum() == c['B'] * 9
                S.check("tie %r" % (c,), got['dz'], want, bound, 88, flags)          # all but the flagged elements
                err = np.abs(got['dz'].astype(f64) - want)[flags]
                if (err <= bound[flags]).all():
                    fits.append(tie)
            assert len(fits) == 1, (c, with_z, fits)
            seen[(c['B'], c['force'], with_z)] = fits[0]
        # the forward at the same point: z = -2.5 everywhere, so i = f = o = 0 and c = h = 0 exactly, whatever c0
        inp = dict(gate_act=S.HARD, xproj=np.full((c['B'], 1, 352), -2.5, f32), U=np.zeros((88, 352), f32), rowbias=None,
                   h0=None, c0=c0)
        fw = W.forward_once(torch, dev, dict(c, save=1), inp)
        assert (fw['gates'][:, :, :88] == -2.5).all() and not fw['cs'].any() and not fw['hs'].any()
    print("\nthe derivative at z = -2.5 per (B, lstm_any, latents):", seen)
    assert set(seen.values()) == {S.DEVICE_TIE}, seen


# ------------------------------------------------------------------------------------------------------------- KS = 8 --
def test_ks8_forward_in_a_child_process(dev, tmp_path):
    """the twelve KS = 8 instances of lstm_fwd_kernel: CLV_LSTM_KS is read once per process, so one fresh child runs the
    lstm.hip forward table and the impulse probes with CLV_LSTM_KS=8 and this process judges what it wrote"""
    out = str(tmp_path / "ks8.npz")
    env = dict(os.environ, CLV_LSTM_KS="8")
    env.pop("CLV_LSTM_ANY", None)
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "seq_worker.py"), out],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "seq_worker failed (%d):\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    Z = np.load(out, allow_pickle=False)
    assert int(Z['ks']) == 8

    def load(tag, inp):
        for k, v in inp.items():
            if isinstance(v, np.ndarray):
                assert np.array_equal(Z["%s/in/%s" % (tag, k)].view(np.uint32), v.view(np.uint32)), (tag, k)
        pre = tag + "/out/"
        return {k[len(pre):]: Z[k] for k in Z.files if k.startswith(pre)}

    run = Cases()
    differs = False
    for n, c in enumerate(S.CASES['fwd88']):
        inp = S.forward_inputs(c)
        got = load("fwd%d" % n, inp)
        assert set(got) == set(S.outputs_of(c, dict(hs=0, cs=0, gates=0, hT=0, cT=0))) | ({'xproj_after'} if c['save'] and c['own'] else set())
        run.run('lstm_fwd_kernel KS=8', repr(c), lambda: S.judge_forward("KS=8 fwd88 %r" % (c,), inp, got))
        if c['T'] == 33 and not differs:                   # the other summation order shows in the bits: the knob was read
            here = W.forward_once(torch, dev, c, inp)
            differs = not np.array_equal(here['hs'].view(np.uint32), got['hs'].view(np.uint32))
    for n, c in enumerate(S.IMPULSE_88):
        for m, scale in enumerate(S.IMPULSE_SCALES):
            inp = S.impulse_inputs(c, scale)
            got = load("imp%d_%d" % (n, m), inp)
            name = "KS=8 impulse %r x %g" % (c, scale)

            def one():
                rep = S.judge_forward(name, inp, got)
                rep.update(S.judge_impulse(name, inp, got, scale))
                return {'impulse ' + k: v for k, v in rep.items()}
            run.run('lstm_fwd_kernel KS=8', name, one)
    run.done()
    if os.environ.get("CLV_LSTM_KS", "4") != "8":
        assert differs, "the child's results are bit for bit those of KS = 4"
