"""CPU: tests/wgrad_reference.py checked against itself and against the oracle before the GPU tests rely on it.

  * the reference equals the LSTM kernel gradients of oracle/clvae_oracle.py on a small LSTM backward (1e-12): H', the window
    zero and the Z columns are the oracle's, not only the header's;
  * every honest fp32 order of `evaluate32` stays below HALF of every element's bound on every case of both tables;
  * every planted fault is rejected (at least one element beyond its bound) on every case where `can_act` says it acts, and
    changes nothing at all where it says it cannot -- no other case is let through;
  * the tables: the row counts are those of tests/test_gpu_wgrad_edges.py, and every value of every list meets a one-stage K
    and a many-stage K.
Cases above 1000 rows are evaluated on four output rows per tensor (`some_rows`): a fault rejected there is rejected on all
rows, and the row-by-row orders would otherwise cost minutes.  Measured here: worst honest |err| / bound 0.49 ('seq', one
accumulator per row range), 0.19 ('stage'), 0.19 ('pair')."""
import os
import re

import numpy as np
import pytest

import wgrad_reference as W
from oracle import clvae_oracle as O

SINGLE = W.single_cases()
PAIRS = W.pair_cases()
PROBLEMS = SINGLE + [c for pq in PAIRS for c in pq]
IDS = ["%s%d-K%d-nx%d-nh%d-nz%d-%s-%s" % ('s' if c.base == 128 else 'p', n, c.K, c.nx, c.nh, c.nz, c.frames, c.family)
       for n, c in enumerate(PROBLEMS)]
WORST = {}                       # order -> worst |err| / bound of the honest evaluations (printed by the last test)


def prepared(c):
    D = W.build(c)
    rows = W.some_rows(c) if c.K > 1000 else W.all_rows(c)
    return D, rows, W.reference(c, D, rows), W.bound(c, D, rows)


def ratio(got, ref, bnd):
    return max(W.worst_ratio(got[t], ref[t], bnd[t][0]) for t in got)


# --------------------------------------------------------------------------------------------------------- the tables --
def test_row_counts_are_those_of_the_edges_test():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_wgrad_edges.py")).read()
    ns = {}
    for name in ("K_ONE_STAGE", "K_SINGLE", "K_PAIR"):
        exec(re.search(r"^%s = .*$" % name, src, re.M).group(0), ns)
        assert ns[name] == getattr(W, name)


def test_every_value_meets_one_stage_and_many_stage_row_counts():
    assert 80 <= len(PROBLEMS) <= 110
    for many in (False, True):
        cs = [c for c in PROBLEMS if (c.K > 160) == many]
        assert {c.nx for c in cs} == set(W.NXS)
        assert {(c.nh, c.nz) for c in cs} == set(W.HZ)
        assert {c.frames for c in cs} == set(W.FRAMES)
        assert {c.h_shift for c in cs} == set(W.SHIFTS)
        assert {c.beta for c in cs} == set(W.BETAS)
        assert {c.family for c in cs} == set(W.FAMILIES)
        assert {c.pads for c in cs} == set(W.PADS)
        assert {c.scale for c in cs} == {1, 2}
        assert {0 if c.period == 0 else (-1 if c.period == c.K else c.period) for c in cs} == set(W.WINDOWS)
    for i in range(7):                                   # every operand and every output is padded somewhere
        assert any(p[i] for p in W.PADS)
    for c in PROBLEMS:
        assert c.nx % 4 == 0 and c.nh % 4 == 0 and all(W.strides(c)[k] % 4 == 0 for k in ('ldx', 'ldh', 'lddz'))
        assert c.frames != 'general' or not W.wide(c.nh, c.nz)
    for p, q in PAIRS:
        assert (p.K, p.frames, p.scale, W.wide(p.nh, p.nz)) == (q.K, q.frames, q.scale, W.wide(q.nh, q.nz))
    for base, cs in ((128, SINGLE), (64, [c for pq in PAIRS for c in pq])):
        assert {W.instance(c) for c in cs} == {(6, 1, True), (6, 1, False), (6, 3, False), (8, 1, True), (8, 1, False)}
        # 1 ... 5 stages per workgroup, one slab and many
        assert {W.kc_rule(c.K, c.scale, base) // 32 for c in cs} >= {1, 2, 3, 4, 5}


# --------------------------------------------------------------------------------------------------------- the oracle --
@pytest.mark.parametrize("nz,h_shift_rows", [(0, 1), (3, 1)])
def test_reference_equals_the_oracles_lstm_kernel_gradients(nz, h_shift_rows):
    rng = np.random.default_rng(nz)
    B, T, H, nx = 3, 5, 88, 8
    xs = rng.standard_normal((B, T, nx + nz)).astype(np.float32).astype(np.float64)
    f = lambda *s: (rng.standard_normal(s) * 0.3).astype(np.float32).astype(np.float64)
    kernel, rec, bias = f(nx + nz, 4 * H), f(H, 4 * H), f(4 * H)
    hs, cache = O.lstm_forward(xs, kernel, rec, bias)
    dHs = f(B, T, H)
    _, dkernel, drec, _, dZ = O.lstm_backward(dHs, cache, kernel, rec)
    K = B * T
    c = W.Case(K=K, nx=nx, nh=H, nz=nz, frames='general', period=T, h_shift=1, beta=0.0, scale=1, base=128,
               pads=(0, 0, 0, 0, 0, 0, 0), family='wide', seed=0)
    flat = xs.reshape(K, nx + nz)                        # X and Z as views of the LSTM's own input rows
    D = W.Data(flat, hs.reshape(K, H), flat[:, nx:] if nz else None, dZ.reshape(K, 4 * H), {})
    ref = W.reference(c, D)
    assert np.abs(ref['dKx'] - dkernel[:nx]).max() <= 1e-12
    assert np.abs(ref['dU'] - drec).max() <= 1e-12
    if nz:
        assert np.abs(ref['dKz'] - dkernel[nx:]).max() <= 1e-12
    # ... and the contract's other window forms against plain loops over the same rows
    for shift, period in ((0, 0), (2, 4), (1, 0), (2, K)):
        c2 = c._replace(h_shift=shift, period=period)
        want = np.zeros((H, 4 * H))
        for k in range(K):
            if k - shift >= 0 and not (period and k % period == 0):
                want += np.outer(D.H[k - shift], D.dz[k])
        assert np.abs(W.reference(c2, D)['dU'] - want).max() <= 1e-12


def test_reference_applies_beta_and_reads_only_the_first_columns():
    c = SINGLE[1]
    assert c.beta != 0 and c.pads[0] and c.pads[4]
    D = W.build(c)
    ref = W.reference(c, D)
    X, dz = D.X[:, :c.nx].astype(np.float64), D.dz[:, :W.N].astype(np.float64)
    want = c.beta * D.C0['dKx'][:, :W.N].astype(np.float64) + X.T @ dz
    assert np.abs(ref['dKx'] - want).max() <= 1e-12 * np.abs(want).max()
    D.X[:, c.nx:], D.dz[:, W.N:], D.H[:, c.nh:] = 9, 9.0, 9.0
    again = W.reference(c, D)
    assert all(np.array_equal(ref[t], again[t]) for t in ref)


# --------------------------------------------------------------------------------------------------------- the pieces --
def test_three_pieces_are_exact_and_the_dropped_pairs_keep_the_promise():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.standard_normal(100000) * np.exp(rng.standard_normal(100000) * 8), W.rich(rng.standard_normal(1000))]).astype(np.float32)
    p = W.split3(x)
    assert np.array_equal(p[0].astype(np.float64) + p[1] + p[2], x.astype(np.float64))
    for q in p:
        assert np.array_equal(q.view(np.uint32) & 0xffff, np.zeros(len(x), np.uint32))      # bf16 numbers
    assert (np.abs(p[1]) <= 2.0 ** -8 * np.abs(x)).all() and (np.abs(p[2]) <= 2.0 ** -16 * np.abs(x)).all()
    worst = 0.0
    for c in PROBLEMS:
        if c.K <= 4225:
            worst = max(worst, W.promise(c, W.build(c)))
    print("largest dropped share of a product on the cases: 2^%.2f" % np.log2(worst))
    assert 0 < worst < 2.0 ** -23


# ------------------------------------------------------------------------------------------- honest orders and faults --
@pytest.mark.parametrize("n", range(len(PROBLEMS)), ids=IDS)
def test_honest_orders_stay_below_half_of_every_bound(n):
    c = PROBLEMS[n]
    D, rows, ref, bnd = prepared(c)
    for order in W.ORDERS:
        r = ratio(W.evaluate32(c, D, order, (), rows), ref, bnd)
        WORST[order] = max(WORST.get(order, 0.0), r)
        assert r <= 0.5, (order, r)


@pytest.mark.parametrize("n", range(len(PROBLEMS)), ids=IDS)
def test_every_planted_fault_is_rejected_wherever_it_can_act(n):
    c = PROBLEMS[n]
    D, rows, ref, bnd = prepared(c)
    honest = W.evaluate32(c, D, 'stage', (), rows)
    r3 = {t: np.arange(min(len(W.all_rows(c)[t]), 3)) for t in rows}          # the stride fault moves whole rows: rows 0, 1, 2
    for fault in W.FAULTS:
        if fault == 'stride_N':
            got = W.evaluate32(c, D, 'stage', (fault,), r3)
            rf, bf = W.reference(c, D, r3), W.bound(c, D, r3)
            same = all(np.array_equal(got[t], W.evaluate32(c, D, 'stage', (), r3)[t]) for t in got) if not W.can_act(c, fault) else None
        else:
            got, rf, bf = W.evaluate32(c, D, 'stage', (fault,), rows), ref, bnd
            same = all(np.array_equal(got[t], honest[t]) for t in got)
        if W.can_act(c, fault):
            hit = [(t,) + W.first_offender(got[t], rf[t], bf[t][0]) for t in got if W.first_offender(got[t], rf[t], bf[t][0])]
            assert hit, ("not rejected", fault, ratio(got, rf, bf))
            print("%s: %s[%d, %d] is %.1f times its bound" % (fault, hit[0][0], hit[0][1], hit[0][2], hit[0][3] / max(hit[0][4], 1e-300)))
        else:
            assert same, ("listed as unable to act, but it changes the result", fault)


def test_worst_honest_ratio_is_recorded():
    if WORST:
        print("worst honest |err| / bound per order:", {k: round(v, 3) for k, v in WORST.items()})
        assert max(WORST.values()) <= 0.5


# ------------------------------------------------------------------------------------------------------ the motivation --
def test_what_the_old_bar_accepts_and_the_bound_rejects():
    """Why the per-element bound: on the first K >= 4096 case with general frames, which planted faults does the older
    2e-6 x sum|a b| bar accept?  Recorded outcome (K = 4225, wide-range dz, four rows per tensor): of the 34 faults that can
    act there the old bar accepts two -- the a0 b2 and the a2 b0 pair of the Z rows left out -- and rejects the rest; the new
    bound rejects all 34.  (The operands carry the largest lower pieces there are, so a missing pair is a coherent 2^-17 of
    every product; the old bar would accept more on random mantissas, where no per-element bound sees the smallest pairs.)
    The new tests are needed for the ABI and the shape holes either way."""
    n = next(i for i, c in enumerate(SINGLE) if c.K >= 4096 and c.frames == 'general')
    c = SINGLE[n]
    D, rows, ref, bnd = prepared(c)
    old = W.old_bar(c, D, rows)
    passed_old, acting = [], 0
    for fault in W.FAULTS:
        if fault == 'stride_N' or not W.can_act(c, fault):
            continue
        acting += 1
        got = W.evaluate32(c, D, 'stage', (fault,), rows)
        assert ratio(got, ref, bnd) > 1, fault
        if all((np.abs(got[t] - ref[t]) <= old[t]).all() for t in got):
            passed_old.append(fault)
    print("K = %d %s: the 2e-6 bar accepts %d of %d acting faults, all rejected by the bound: %s" % (c.K, c.family, len(passed_old), acting, passed_old))
