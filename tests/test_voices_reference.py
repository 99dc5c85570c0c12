"""No GPU: the fp64 definition of voice-count constraints (tests/voices_reference.py) against enumeration, its
corner rules, and the margin the GPU test's own inputs keep from every threshold."""
import itertools

import numpy as np
import pytest

import smc_reference as SR
import voices_reference as VR

FREE = VR.FREE


def _enumerate(q, lo, hi, roll_row=None):
    """p(x) over every outcome of D notes that honours the roll and has its count in range, and their total"""
    D = len(q)
    out, tot = {}, 0.0
    for xs in itertools.product((0, 1), repeat=D):
        if not lo <= sum(xs) <= hi:
            continue
        if roll_row is not None and any(c <= 1 and x != c for x, c in zip(xs, roll_row)):
            continue
        free = [j for j in range(D) if roll_row is None or roll_row[j] > 1]
        px = float(np.prod([q[j] if xs[j] else 1.0 - q[j] for j in free]))
        out[xs] = px
        tot += px
    return out, tot


@pytest.mark.parametrize("lo,hi", [(2, 3), (0, 0), (8, 8), (0, 8), (1, 1), (5, 7)])
@pytest.mark.parametrize("forced", [False, True])
def test_chain_probabilities_equal_enumeration(lo, hi, forced):
    """D = 8: the product of the chain's conditionals is p(x) / P(range) for every outcome, and they sum to 1.  (0, 0) walks
    the a == 0 rule at every note, (8, 8) the b == 0 rule; with forced notes the table runs on q = 0 / 1 there."""
    rng = np.random.default_rng(lo * 16 + hi)
    D = 8
    p = rng.uniform(0.05, 0.9, D).astype(np.float32)
    roll_row = None
    if forced:
        roll_row = np.full(D, FREE, np.uint8)
        n_on = min(hi, 2)
        roll_row[[1, 6][:n_on]] = 1
        if D - n_on - 1 >= lo:
            roll_row[3] = 0
        assert VR.feasible(roll_row, lo, hi)
    q = VR.clipped(p)
    px, tot = _enumerate(q, lo, hi, roll_row)
    B = VR.table(VR.recursion_q(p, roll_row), lo, hi)
    assert abs(B[0, 0] - tot) <= 1e-13 * max(tot, 1e-300) + 1e-300
    total = 0.0
    for xs in itertools.product((0, 1), repeat=D):
        pr = VR.outcome_probability(p, xs, lo, hi, roll_row)
        want = px.get(xs, 0.0) / tot
        assert abs(pr - want) <= 1e-13, (xs, pr, want)
        total += pr
    assert abs(total - 1.0) <= 1e-13


def test_draw_follows_its_own_conditionals_and_the_corner_rules():
    rng = np.random.default_rng(3)
    D = 8
    p = rng.uniform(0.05, 0.9, D).astype(np.float32)
    # (0, 0): a == 0 at every note, whatever the uniforms; (8, 8): b == 0 at every note
    for u in (np.zeros(D, np.float32), np.ones(D, np.float32), rng.random(D).astype(np.float32)):
        x, logb, margin = VR.draw(p, u, 0, 0)
        assert not x.any() and margin == np.inf and np.isclose(logb, np.log(np.prod(1 - VR.clipped(p))), rtol=1e-14)
        x, logb, margin = VR.draw(p, u, D, D)
        assert x.all() and margin == np.inf and np.isclose(logb, np.log(np.prod(VR.clipped(p))), rtol=1e-14)
    # forced notes keep their value and count; the rest fills the range
    roll_row = np.array([1, FREE, 0, FREE, FREE, 1, FREE, 0], np.uint8)
    for _ in range(200):
        u = rng.random(D).astype(np.float32)
        lo = int(rng.integers(2, 5))
        hi = int(rng.integers(lo, 6))
        x, logb, _ = VR.draw(p, u, lo, hi, roll_row)
        assert x[0] == 1 and x[5] == 1 and x[2] == 0 and x[7] == 0 and lo <= x.sum() <= hi and logb <= 0
    # frequencies of a small case against the enumeration (the chain is exact, so this is a test of draw's bookkeeping)
    n, hits = 20000, {}
    for _ in range(n):
        x, _, _ = VR.draw(p[:4], rng.random(4).astype(np.float32), 1, 2)
        hits[tuple(int(v) for v in x)] = hits.get(tuple(int(v) for v in x), 0) + 1
    px, tot = _enumerate(VR.clipped(p[:4]), 1, 2)
    for xs, v in px.items():
        f, w = hits.get(xs, 0) / n, v / tot
        assert abs(f - w) < 4 * np.sqrt(w * (1 - w) / n) + 1e-9, (xs, f, w)
    with pytest.raises(ValueError):
        VR.draw(p, rng.random(D).astype(np.float32), 0, 1, roll_row)          # two forced on, hi = 1


def test_free_pair_is_the_plain_draw():
    rng = np.random.default_rng(5)
    R, D = 7, 88
    xhat, u = rng.random((R, D)).astype(np.float32), rng.random((R, D)).astype(np.float32)
    rows = np.where(rng.random((R, D)) < 0.3, (rng.random((R, D)) < 0.5).astype(np.uint8), np.uint8(FREE)).astype(np.uint8)
    pairs = np.tile(np.array(VR.FREE_PAIR, np.uint8), (R, 1))
    x, ell, logb, margin = VR.sample_frame(xhat, u, rows, pairs)
    assert np.array_equal(x, SR.sample_frame(xhat, u, rows)) and np.array_equal(ell, SR.increment(xhat, rows))
    assert not logb.any() and margin == np.inf
    x, ell, _, _ = VR.sample_frame(xhat, u, None, pairs)
    assert np.array_equal(x, (u <= xhat).astype(np.float64)) and not ell.any()


def test_clipped_probabilities_at_88_notes():
    """the issue's own figures: 2000 random frames with up to 20 notes at the clip stay in range; all 88 at the clip with
    lo = hi = 15 still has a normal B[0][0]"""
    rng = np.random.default_rng(0)
    lo_clip = np.float32(1e-7)
    for _ in range(300):
        p = (1 / (1 + np.exp(-rng.normal(-3, 2.5, 88)))).astype(np.float32)
        p[rng.choice(88, int(rng.integers(0, 20)), replace=False)] = lo_clip
        lo = int(rng.integers(0, 16))
        hi = int(rng.integers(lo, 16))
        x, logb, _ = VR.draw(p, rng.random(88).astype(np.float32), lo, hi)
        assert lo <= x.sum() <= hi and np.isfinite(logb)
    B = VR.table(VR.clipped(np.full(88, lo_clip)), 15, 15)
    assert 1e-89 < B[0, 0] < 1e-88


@pytest.mark.parametrize("R,P", [(1, 1), (5, 1), (5, 5), (67, 1), (66, 11)])
@pytest.mark.parametrize("with_roll", [False, True])
def test_gpu_inputs_keep_the_margin(R, P, with_roll):
    """tests/test_gpu_voices.py compares note for note: on its direct inputs no free note of the reference has
    |u - a / B| < 1e-9, so a fused multiply-add in the recursion cannot flip one"""
    nsteps = 5
    xhat, u, roll, voices = VR.kernel_case(R, P, nsteps, with_roll, seed=R + P)
    assert set(map(tuple, voices.reshape(-1, 2))) >= (set(VR.KERNEL_PAIRS) if R // P * nsteps >= len(VR.KERNEL_PAIRS) else set())
    for k in range(nsteps):
        rows = None if roll is None else np.repeat(roll[:, k], P, axis=0)
        pairs = np.repeat(voices[:, k], P, axis=0)
        x, ell, logb, margin = VR.sample_frame(xhat, u, rows, pairs)
        assert margin >= 1e-9
        n = x.sum(-1)
        free = (pairs[:, 0] == 0) & (pairs[:, 1] == 255)
        assert np.all(free | ((n >= pairs[:, 0]) & (n <= pairs[:, 1])))
        assert rows is None or np.all((rows > 1) | (x == rows))
        assert np.all(np.isfinite(ell))
