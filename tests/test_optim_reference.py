"""tests/optim_reference.py held to the oracle (and through it to the G6 reference lines), an honest fp32 evaluation held to
its bounds in four summation orders, and planted faults that a named criterion must reject.  CPU only.

Criteria (criteria() below): 'bound X' -- an element of output X beyond its bound; 'rms X' -- rms(err / sigma) > 1 for a tensor
of at least 1000 elements; 'untouched X' -- an element of X that the step does not own was changed (bound 0); 'true sums'
-- the stored vn2 of the tall matrix is not sum_r (W / s)^2 of the stored parameters within that sum's bound.
Which criterion catches which planted fault (PLANTED: fault, case, route, summation order, criterion; the figures are
printed with -s):
  ragged_out         the ragged last unit's rows left out of the column sums             bound vn2
  partial_last       the unit partial at index nunits - 1 dropped                         bound vn2
  partial_704        the unit partial at index 704 dropped (two tall matrices)            bound vn2
  col_neighbour      a column's scalars taken from the next column                        bound params
  col_group16 / 64   ... from the same lane of the previous 16- / 64-column group         bound params
  t_plus1            t off by one                                                         bound params
  no_bias_corr       lr instead of lr_t                                                   bound params
  b1b2_swap          b1 and b2 swapped                                                    bound m
  eps_in_sqrt        sqrt(v + eps)                                                        bound params
  gov_once           grad_g / Vn taken as grad_g                                          bound m
  old_s              W' = s V'                                                            bound params
  mgvg_per_unit      mg, vg stepped once per 16-row unit                                  bound mg
  vn2_after_rescale  vn2' = sum W'^2                                                      bound vn2
  vn2_stale          vn2 of the step before, parameters rewritten in between              true sums
  m_under_rmsprop    m written under RMSprop                                              untouched m
  skip_last_float4   the last 16 bytes of every 64-row tile not written                   bound params
  float2_second      the second float of a pair takes the first's column scalars          bound params
"""
import numpy as np
import pytest

import optim_reference as R
from oracle import clvae_oracle as O
from test_g6_reference_lines import G, NAMES, NSTEPS, _opt_inputs


# ---------------------------------------------------------------------------------------------------------- helpers --
def start(case, route, seed=0, grad_seed=99):
    table, n, n_cols, st = R.make_state(case, route, seed)
    g, cnt = R.make_grads(table, n, grad_seed, zero=case['name'] == 'zero_gradient')
    known = dict(tensor=R.tall_index(table), use=False, gdot=None) if route in ('chain', 'fast') else None
    return table, st, g, R.hyper(opt=R.ROUTE_OPT[route]), known, cnt


def criteria(got, ref, table, grads=None):
    """the names of the criteria that reject `got`"""
    out = set()
    for k in R.OUTPUTS:
        e = np.abs(np.asarray(got[k], np.float64) - ref[k])
        own = ref['s_' + k] > 0
        if not (e[own] <= ref['b_' + k][own]).all():
            out.add('bound ' + k)
        if not (e[~own] == 0).all():
            out.add('untouched ' + k)
    out.update(k for k, _ in R.rms_violations(got, ref, table))
    ti = R.tall_index(table)
    if grads is not None and ti is not None and not R.sums_ratio(got['vn2'], got['params'], got['s'], grads, table[ti]) <= 1.0:
        out.add('true sums')
    return out


def unflatten(flat, table):
    return {d.name: np.asarray(flat[d.offset:d.offset + d.rows * d.cols], np.float64).reshape(d.shape) for d in table}


def cols_of(arr, table):
    return {d.name: np.asarray(arr[d.col_offset:d.col_offset + d.cols], np.float64) for d in table if d.is_matrix}


ALL = R.GPU_CASES + R.DEGENERATE_CASES
CASE_ROUTES = [(c, r) for c in R.GPU_CASES for r in c['routes']]
IDS = ["%s-%s" % (c['name'], r) for c, r in CASE_ROUTES]


# ------------------------------------------------------------------------------------------- reference == the oracle --
@pytest.mark.parametrize("opt", [R.OPT_ADAM_WN, R.OPT_ADAM, R.OPT_RMSPROP])
def test_ref_step_is_the_oracle(opt):
    """ref_step restarted from its own fp64 outputs equals oracle.adam_wn_step (weight norm on and off) and
    oracle.rmsprop_step over four steps: parameters and every piece of state, rtol 1e-12"""
    case = R.GPU_CASES[-1]
    table, n, n_cols = R.layout(case['shapes'])
    rng = np.random.default_rng(5)
    st = {k: np.zeros(n) for k in R.FLAT}
    st.update({k: np.zeros(n_cols) for k in R.COLS})
    st['s'][:] = 1
    st['params'] = rng.standard_normal(n) * 0.1
    st['t'] = 0
    hyp = dict(lr=1e-3, b1=0.9, b2=0.999 if opt != R.OPT_RMSPROP else 0.9, eps=1e-8, opt=opt)
    p = unflatten(st['params'], table)
    ost = O.adam_wn_init(p, weightnorm=opt == R.OPT_ADAM_WN)
    acc = {k: np.zeros_like(v) for k, v in p.items()}
    for step in range(4):
        g = rng.standard_normal(n)
        ref = R.ref_step(st, g, table, hyp)
        if opt == R.OPT_RMSPROP:
            O.rmsprop_step(p, unflatten(g, table), acc, lr=hyp['lr'], rho=hyp['b2'], eps=hyp['eps'])
        else:
            O.adam_wn_step(p, unflatten(g, table), ost, lr=hyp['lr'], b1=hyp['b1'], b2=hyp['b2'], eps=hyp['eps'])
        got = unflatten(ref['params'], table)
        for d in table:
            np.testing.assert_allclose(got[d.name], p[d.name], rtol=1e-12, atol=1e-300, err_msg="%s step %d" % (d.name, step))
        st = {k: ref[k] for k in R.OUTPUTS}
        st['t'] = ref['counter']
    m, v = unflatten(st['m'], table), unflatten(st['v'], table)
    for d in table:
        if opt == R.OPT_RMSPROP:
            np.testing.assert_allclose(v[d.name], acc[d.name], rtol=1e-12)
            assert (m[d.name] == 0).all()
            continue
        np.testing.assert_allclose(m[d.name], ost['m'][d.name], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(v[d.name], ost['v'][d.name], rtol=1e-12, atol=1e-300)
        if opt == R.OPT_ADAM_WN and d.is_matrix:
            for k in ('mg', 'vg', 's'):
                np.testing.assert_allclose(cols_of(st[k], table)[d.name], ost[k][d.name], rtol=1e-12, atol=1e-300)
    assert st['t'] == 4 and (opt == R.OPT_RMSPROP or ost['t'] == 4)


def test_ref_step_matches_the_reference_lines():
    """ref_step against the numbers the reference's own optimizer lines produced (tests/golden/g6_reference_lines.npz):
    parameters after each of the four steps and the whole state at the end"""
    p0, grads = _opt_inputs()
    table, n, n_cols = R.layout([(nm, p0[nm].shape) for nm in NAMES])
    st = {k: np.zeros(n) for k in R.FLAT}
    st.update({k: np.zeros(n_cols) for k in R.COLS})
    st['s'][:] = 1
    st['t'] = 0
    for d in table:
        st['params'][d.offset:d.offset + d.rows * d.cols] = p0[d.name].reshape(-1)
    hyp = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, opt=R.OPT_ADAM_WN)
    for s in range(NSTEPS):
        g = np.zeros(n)
        for d in table:
            g[d.offset:d.offset + d.rows * d.cols] = grads[s][d.name].reshape(-1)
        ref = R.ref_step(st, g, table, hyp)
        got = unflatten(ref['params'], table)
        for nm in NAMES:
            np.testing.assert_allclose(got[nm], G['opt/p%d/%s' % (s + 1, nm)], rtol=1e-12, atol=1e-15, err_msg="%s step %d" % (nm, s))
        st = {k: ref[k] for k in R.OUTPUTS}
        st['t'] = ref['counter']
    k = len(NAMES)
    m, v = unflatten(st['m'], table), unflatten(st['v'], table)
    for i, nm in enumerate(NAMES):
        np.testing.assert_allclose(m[nm], G['opt/state/%02d' % i], rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(v[nm], G['opt/state/%02d' % (k + i)], rtol=1e-12, atol=1e-300)
    j = 2 * k
    for d in table:
        if d.is_matrix:
            for q, key in enumerate(('s', 'mg', 'vg')):
                np.testing.assert_allclose(cols_of(st[key], table)[d.name], G['opt/state/%02d' % (j + q)], rtol=1e-12, atol=1e-300)
            j += 3
    assert j == int(G['opt/n_state']) and st['t'] == NSTEPS


def test_known_sums_form_is_the_plain_form():
    """with the true sums as inputs (vn2 = A, gdot = sum_r g W) the known-sums form gives the plain form's outputs to 1e-12"""
    for case in R.GPU_CASES:
        if 'fast' not in case['routes']:
            continue
        table, st, g, hyp, known, _ = start(case, 'fast')
        ti = known['tensor']
        ts = R.true_sums(st['params'], st['s'], g, table[ti])
        d = table[ti]
        st64 = {k: np.asarray(st[k], np.float64) for k in R.OUTPUTS}
        st64['t'] = st['t']
        st64['vn2'][d.col_offset:d.col_offset + d.cols] = ts['A']
        plain = R.ref_step(st64, g, table, hyp, known=known)
        fast = R.ref_step(st64, g, table, hyp, known=dict(tensor=ti, use=True, gdot=ts['gdot']))
        # 1e-12 of the value, or, where grad_V = s (g - gov V) or the moment's own sum cancels, of the operands |s g| + |s gov V|
        # and the old moment (fp64 itself cannot do better there); params' through the largest possible update
        sl = slice(d.offset, d.offset + d.rows * d.cols)
        cs = slice(d.col_offset, d.col_offset + d.cols)
        ops_ = np.zeros_like(plain['m'])
        g2 = np.asarray(g, np.float64)[sl].reshape(d.rows, d.cols)
        ops_[sl] = (st64['s'][cs] * (np.abs(g2) + np.abs(ts['B'] / ts['A'] * ts['V']))).reshape(-1)
        scale = dict(m=(1 - hyp['b1']) * ops_ + np.abs(st64['m']), v=(1 - hyp['b2']) * ops_ ** 2 + np.abs(st64['v']),
                     params=np.where(ops_ > 0, plain['lr_t'] * R.cap(hyp), 0.0))
        for k in R.OUTPUTS:
            tol = 1e-12 * (np.abs(plain[k]) + scale.get(k, 0.0))
            assert (np.abs(fast[k] - plain[k]) <= tol).all(), (case['name'], k)
        assert fast['counter'] == plain['counter'] == st['t'] + 1


def test_step_rules():
    h = R.hyper()
    assert R.step_of(5, 'advance') == (6, 6) and R.step_of(5, 'readonly') == (6, 5)
    assert R.step_of(5, 'advanced') == (5, 5) and R.step_of(5, ('explicit', 9)) == (9, None)
    assert abs(R.lr_t64(h, 1) / (h['lr'] * np.sqrt(1 - h['b2']) / (1 - h['b1'])) - 1) < 1e-15
    # the four digits of the docstring, and a bound that falls to a few roundings once b^t is small
    assert 5e-4 < R.rel_lr(h, 1) < 2e-3 and R.rel_lr(h, 10 ** 5) < 6 * R.U


# ----------------------------------------------------------------------------------------- an honest fp32 evaluation --
@pytest.mark.parametrize("case,route", CASE_ROUTES, ids=IDS)
def test_honest_fp32_passes_in_every_order(case, route):
    """numpy fp32, column sums row after row, as a tree, and through per-unit partials of 16 and of 64 rows; the fast route
    with the true sums rounded to fp32 as its inputs: no element beyond its bound, rms(err / sigma) <= 1; and the share of
    insensitive elements of params' is at most 1 %"""
    table, st, g, hyp, known, cnt = start(case, route)
    ti = R.tall_index(table)
    if route == 'fast':
        d = table[ti]
        ts = R.true_sums(st['params'], st['s'], g, d)
        st['vn2'][d.col_offset:d.col_offset + d.cols] = ts['A'].astype(np.float32)
        known = dict(tensor=ti, use=True, gdot=ts['gdot'].astype(np.float32))
    ref = R.ref_step(st, g, table, hyp, known=known)
    assert all(np.isfinite(ref[k]).all() and np.isfinite(ref['b_' + k]).all() for k in R.OUTPUTS)
    share = R.insensitive_share(ref, table)
    print("\n%s/%s: insensitive %.4f %% of params', zero rows %d, zero columns %d" % (case['name'], route, 100 * share, cnt['zero_rows'], cnt['zero_cols']))
    assert share <= 0.01
    assert cnt['zero_cols'] == sum(1 for d in table if d.is_matrix and d.cols >= 2)
    for order in R.ORDERS:
        got = R.eval32(st, g, table, hyp, known=known, order=order)
        ra, rm = R.ratios(got, ref), R.rms(got, ref, table)
        print("  %-4s worst error / bound: %s | rms: %s" % (order, ", ".join("%s %.3g" % kv for kv in ra.items()),
                                                          ", ".join("%s %.3g" % kv for kv in rm.items())))
        assert not criteria(got, ref, table, g if known is not None else None), (order, ra, rm)
        assert got['counter'] == ref['counter'] == st['t'] + 1


@pytest.mark.parametrize("case", R.DEGENERATE_CASES, ids=[c['name'] for c in R.DEGENERATE_CASES])
def test_degenerate_cases(case):
    """one-row matrices (grad_V is an exact 0, in fp32 rounding noise that Adam normalises: params' is insensitive) and all-zero
    gradients: everything finite, m' and v' within their bounds; under zero gradients nothing moves at all"""
    for route in case['routes']:
        table, st, g, hyp, known, _ = start(case, route)
        ti = R.tall_index(table)
        if route == 'fast':
            d = table[ti]
            ts = R.true_sums(st['params'], st['s'], g, d)
            st['vn2'][d.col_offset:d.col_offset + d.cols] = ts['A'].astype(np.float32)
            known = dict(tensor=ti, use=True, gdot=ts['gdot'].astype(np.float32))
        ref = R.ref_step(st, g, table, hyp, known=known)
        for order in R.ORDERS:
            got = R.eval32(st, g, table, hyp, known=known, order=order)
            assert all(np.isfinite(got[k]).all() for k in R.OUTPUTS)
            assert not R.violations(got, ref, ('m', 'v')), R.ratios(got, ref, ('m', 'v'))
            if case['name'] == 'zero_gradient':
                for k in ('m', 'v', 'mg', 'vg'):
                    assert (got[k] == st[k]).all()
                assert np.abs(got['params'].astype(np.float64) - st['params']).max() <= 4 * R.U * np.abs(st['params'][st['params'] != R.SENTINEL]).max()
                assert not R.violations(got, ref)
            else:
                assert R.insensitive_share(ref, table) > 0.01


# --------------------------------------------------------------------------------------------------- planted faults --
BY_NAME = {c['name']: c for c in ALL}
PLANTED = [
    ('ragged_out', 'chain_tall_last', 'chain', 'u16', 'bound vn2'),
    ('partial_last', 'chain_704_units', 'chain', 'u16', 'bound vn2'),
    ('partial_704', 'chain_two_tall_main_loop', 'chain', 'u16', 'bound vn2'),
    ('col_neighbour', 'chain_tall_last', 'chain', 'u16', 'bound params'),
    ('col_group16', 'small', 'small', 'seq', 'bound params'),
    ('col_group64', 'chain_tall_last', 'chain', 'u16', 'bound params'),
    ('t_plus1', 'small', 'small', 'seq', 'bound params'),
    ('no_bias_corr', 'small', 'small', 'seq', 'bound params'),
    ('b1b2_swap', 'small', 'small', 'seq', 'bound m'),
    ('eps_in_sqrt', 'chain_tall_last', 'chain', 'u16', 'bound params'),
    ('gov_once', 'chain_tall_last', 'chain', 'u16', 'bound m'),
    ('old_s', 'chain_tall_last', 'chain', 'u16', 'bound params'),
    ('mgvg_per_unit', 'chain_tall_last', 'chain', 'u16', 'bound mg'),
    ('vn2_after_rescale', 'chain_tall_last', 'chain', 'u16', 'bound vn2'),
    ('m_under_rmsprop', 'mixed_plain', 'rmsprop', 'seq', 'untouched m'),
    ('skip_last_float4', 'flat_193x100', 'fast', 'u64', 'bound params'),
    ('float2_second', 'pair_193x126', 'fast', 'u64', 'bound params'),
]


@pytest.mark.parametrize("fault,cname,route,order,criterion", PLANTED, ids=[p[0] for p in PLANTED])
def test_planted_fault_is_rejected(fault, cname, route, order, criterion):
    table, st, g, hyp, known, _ = start(BY_NAME[cname], route)
    if route == 'fast':
        ti = R.tall_index(table)
        d = table[ti]
        ts = R.true_sums(st['params'], st['s'], g, d)
        st['vn2'][d.col_offset:d.col_offset + d.cols] = ts['A'].astype(np.float32)
        known = dict(tensor=ti, use=True, gdot=ts['gdot'].astype(np.float32))
    ref = R.ref_step(st, g, table, hyp, known=known)
    assert not criteria(R.eval32(st, g, table, hyp, known=known, order=order), ref, table, g if known else None)
    got = R.eval32(st, g, table, hyp, known=known, order=order, faults=(fault,))
    fired = criteria(got, ref, table, g if known else None)
    ra = R.ratios(got, ref)
    print("\n%s: rejected by %s; worst error / bound: %s" % (fault, sorted(fired), ", ".join("%s %.3g" % kv for kv in ra.items())))
    assert criterion in fired, (fault, fired)


def test_stale_vn2_is_rejected_by_the_true_sums():
    """the known-sums form takes vn2 on trust: a step whose vn2 is the previous step's although the parameters were rewritten in
    between agrees with the reference of the same (wrong) inputs; the comparison of the stored vn2 with the true sums
    of the stored parameters is what rejects it -- before the step and, since the fast step's own vn2' is computed afresh,
    not after it.  No step is run with the stale value here: the test shows that the check fires on the stored state.  On the
    GPU, tests/test_gpu_optim.py makes that comparison after every step, i.e. in front of every fast step, and
    test_known_sums_are_consumed runs steps with a vn2 that is 1 % off"""
    table, st, g, hyp, known, _ = start(BY_NAME['flat_193x100'], 'fast')
    ti = R.tall_index(table)
    d = table[ti]
    first = R.eval32(st, g, table, hyp, known=known, order='u16')            # a chain step leaves vn2
    assert R.sums_ratio(first['vn2'], first['params'], first['s'], g, d) <= 1.0
    st2 = {k: first[k].copy() for k in R.OUTPUTS}
    st2['t'] = first['counter']
    sl = slice(d.offset, d.offset + d.rows * d.cols)
    st2['params'][sl] *= np.float32(1.0 + 1e-4)                              # set_weights of slightly different values
    q = R.sums_ratio(st2['vn2'], st2['params'], st2['s'], g, d)
    print("\nstale vn2 after a 1e-4 rewrite: |vn2 - true| / bound = %.3g" % q)
    assert q > 1.0
