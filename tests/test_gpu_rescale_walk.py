"""-m gpu: the walk of wn_fast_rescale_kernel (csrc/optim.hip) over the partial ||V'||^2 rows -- rounds of 12 loads
requested together, row index clamped, the value masked to +0 beyond the range -- through clv_adam_wn_step's two-launch
route on ONE tall matrix, at the row counts where the walk can go wrong.  nunits = ceil(rows / 64) partial rows, 16 row
lanes, so a lane's round covers rows k, k + 16, .., k + 176:
  3          the smallest a tall matrix (more than 144 rows) can have: every lane's round is clamped from its first or second load on
  12, 13     fewer rows than row lanes: lanes 12.. (13..) add nothing and must still hold +0
  16, 17     16 +- 1 row lanes: the second load of lane 0 alone is in range
  25         a ragged second load
  176        configuration 3's own count (11 loads in range, the 12th clamped), last tile ragged
  192, 193   a whole round, and the first row of a second round (lane 0 alone)
nunits = 1 and 2 cannot reach the kernel: a matrix of at most 128 rows is not tall, and the launcher refuses the known-sums
form for it (CLV_EINVAL, nothing launched); those two cases assert exactly that.
cols 4, 88, 128 take the flat body (float4 tile), 90 the float2 row-lane body; both share the walk.

Per case: one known-sums step; params, m, v, mg, vg, s, vn2 against tests/optim_reference.py at test_gpu_optim.py's bounds
(its compare / check_sums); that the two-launch form ran, the way test_known_sums_are_consumed shows it (gdot 1 % too
large: within the bounds of the known-sums reference on these inputs, beyond those of the plain form); and a second run from
the same state, bit for bit.  The last tile is ragged in every case (rows = 64 (nunits - 1) + r, r < 64)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import optim_reference as R
import test_gpu_optim as TO

pytestmark = pytest.mark.gpu

COLS = (4, 88, 128, 90)
NUNITS = (3, 12, 13, 16, 17, 25, 176)
CASES = [(c, n) for c in COLS for n in NUNITS] + [(4, 192), (4, 193), (90, 192), (90, 193)]


@pytest.fixture(scope="module")
def dev():
    import clvae_amd  # noqa: F401
    from clvae_amd import _lib
    _lib.require_gpu()          # fail loudly: no CPU fallback
    return torch.device("cuda:0")


def rows_of(nunits):
    return 64 * (nunits - 1) + (7 * nunits) % 63 + 1          # last tile of 1..63 rows


def case_of(cols, nunits):
    rows = rows_of(nunits)
    assert (rows + 63) // 64 == nunits and rows % 64
    name = "%s_%dx%d" % ('flat' if cols % 4 == 0 else 'pair', rows, cols)
    return dict(name=name, shapes=[('t/kernel', (rows, cols)), ('a/bias', (3,))], routes=('fast',), only=None)


@pytest.mark.parametrize("cols,nunits", CASES, ids=["%dcols-%dunits" % c for c in CASES])
def test_rescale_walk(dev, cols, nunits):
    case = case_of(cols, nunits)
    table, n, n_cols, st = R.make_state(case, 'fast', history=1)
    TO.assert_rule('fast', table, case)
    hyp = R.hyper()
    g, _ = R.make_grads(table, n, 91)
    ti = R.tall_index(table)
    d = table[ti]
    ts = R.true_sums(st['params'], st['s'], g, d)
    st['vn2'][d.col_offset:d.col_offset + d.cols] = ts['A'].astype(np.float32)
    known = dict(tensor=ti, use=True, gdot=ts['gdot'].astype(np.float32) * np.float32(1.01))
    outs = []
    for run in range(2):
        D = TO.Dev(dev, table, st, g)
        before = D.read()
        D.step(table, hyp, 'advance', known)
        outs.append(D.read())
    after = outs[0]
    route = 'walk-%s' % R.fast_body(d)
    TO.compare(route, after, before, R.ref_step(before, g, table, hyp, 'advance', known), table, g)
    TO.check_sums(route, after, table, g)
    plain = R.ref_step(before, g, table, hyp, 'advance', dict(tensor=ti, use=False, gdot=None))
    bad = dict(R.violations(after, plain))
    assert 'params' in bad and 'mg' in bad, bad               # the chain would have recomputed gdot from the parameters
    for k in R.OUTPUTS:
        assert (outs[0][k].view(np.uint32) == outs[1][k].view(np.uint32)).all(), k
    assert (after['params'] != st['params']).any()


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("nunits", (1, 2))
def test_one_and_two_partial_rows_are_not_tall(dev, cols, nunits):
    """at most 128 rows: a small matrix, the known-sums form is refused on the host and every buffer stays bitwise"""
    rows = rows_of(nunits)
    case = dict(name='small_%dx%d' % (rows, cols), shapes=[('t/kernel', (rows, cols)), ('a/bias', (3,))], routes=('small',), only=None)
    table, n, n_cols, st = R.make_state(case, 'small', history=1)
    assert not R.is_tall(table[0]) and (rows + 63) // 64 == nunits
    g, _ = R.make_grads(table, n, 92)
    d = table[0]
    ts = R.true_sums(st['params'], st['s'], g, d)
    st['vn2'][d.col_offset:d.col_offset + d.cols] = ts['A'].astype(np.float32)
    D = TO.Dev(dev, table, st, g)
    before = D.read()
    D.step(table, R.hyper(), 'advance', dict(tensor=0, use=True, gdot=ts['gdot'].astype(np.float32)), expect=TO.EINVAL)
    after = D.read()
    for k in R.OUTPUTS + ('grads',):
        assert (after[k].view(np.uint32) == before[k].view(np.uint32)).all(), k
    assert after['t'] == before['t']
