"""CPU tests of tests/novelty_reference.py, the yardstick of the novelty audit: the matrix-product reference
against the loop-by-loop definition on random tiny cases, and hand-made cases for every rule of the contract."""
import numpy as np
import pytest

import novelty_reference as NR


def rolls(rng, lengths, D, density=0.3):
    return [(rng.random((P, D)) < density).astype(np.uint8) for P in lengths]


def same(a, b):
    assert len(a) == len(b)
    for (d0, s0, g0), (d1, s1, g1) in zip(a, b):
        np.testing.assert_array_equal(d0, d1)
        np.testing.assert_array_equal(s0, s1)
        np.testing.assert_array_equal(g0, g1)


@pytest.mark.parametrize("D", [1, 5, 33])
@pytest.mark.parametrize("W", [1, 2, 5])
@pytest.mark.parametrize("S", [0, 1, 3])
@pytest.mark.parametrize("hop", [1, 2])
def test_fast_reference_equals_the_loops(D, W, S, hop):
    rng = np.random.default_rng(1000 * D + 100 * W + 10 * S + hop)
    q = rolls(rng, [W + 3, W - 1, W, 0, 7], D, 0.25)
    c = rolls(rng, [6, W, W - 1, 0, 9], D, 0.25)
    q[0][:] = c[4][1:1 + W + 3] if W + 4 <= 9 else q[0]                # an excerpt: exact matches exist
    if D > 2:
        q[4][:, 0] = 1                                                 # a note on key 0: no shift down
        q[2][:, D - 1] = 1
    same(NR.nearest(q, c, W, hop, S), NR.nearest_loops(q, c, W, hop, S))
    ex = [4, -1, 0, 2, 1]
    same(NR.nearest(q, c, W, hop, S, ex), NR.nearest_loops(q, c, W, hop, S, ex))


D, W = 24, 6


def corpus3(seed=0):
    rng = np.random.default_rng(seed)
    c = rolls(rng, [20, 31, 17], D, 0.2)
    for p in c:                                                        # notes in the middle: every shift in +-5 is allowed
        p[:, :6] = 0
        p[:, D - 6:] = 0
    return c


def test_a_planted_copy_is_found_where_it_was_taken():
    c = corpus3()
    q = [c[1][9:9 + W + 2].copy()]
    for fn in (NR.nearest, NR.nearest_loops):
        dist, shift, cframe = fn(q, c, W, 1, 0)[0]
        assert dist.tolist() == [0, 0, 0] and shift.tolist() == [0, 0, 0]
        song, frame = NR.song_frame(cframe, NR.offsets(c))
        assert song.tolist() == [1, 1, 1] and frame.tolist() == [9, 10, 11]


def test_a_copy_a_fourth_up_needs_five_semitones():
    c = corpus3(1)
    q = [NR.shifted(c[2][4:4 + W], -5)]                                # the corpus passage is the query a fourth UP
    assert q[0].sum() == c[2][4:4 + W].sum() > 0
    dist, shift, cframe = NR.nearest(q, c, W, 1, 5)[0]
    assert (dist[0], shift[0]) == (0, 5)
    assert NR.song_frame(cframe, NR.offsets(c))[0][0] == 2 and NR.song_frame(cframe, NR.offsets(c))[1][0] == 4
    d4, s4, _ = NR.nearest(q, c, W, 1, 4)[0]
    assert d4[0] > 0 and abs(s4[0]) <= 4
    same(NR.nearest(q, c, W, 1, 5), NR.nearest_loops(q, c, W, 1, 5))


def test_notes_on_the_edge_keys_pin_the_shift():
    rng = np.random.default_rng(2)
    c = rolls(rng, [30], D, 0.2)
    low, high = rolls(rng, [12, 12], D, 0.1)
    low[:, 0] = 1
    high[:, D - 1] = 1
    # the passage that a downward (upward) shift of the query would match exactly
    c.append(NR.shifted(low, -2))
    c.append(NR.shifted(high, 2))
    res = NR.nearest([low, high], c, W, 1, 3)
    assert (res[0][1] >= 0).all() and (res[1][1] <= 0).all()
    assert (res[0][0] > 0).all() and (res[1][0] > 0).all()
    both = low.copy()
    both[:, D - 1] = 1
    assert (NR.nearest([both], c, W, 1, 3)[0][1] == 0).all()
    silent = np.zeros((W, D), np.uint8)                                # every shift allowed, all equally far: shift 0
    d, s, g = NR.nearest([silent], [silent.copy()], W, 1, 3)[0]
    assert (d[0], s[0], g[0]) == (0, 0, 0)


def test_ties_go_to_the_lower_piece_the_smaller_shift_and_down_before_up():
    c = corpus3(3)
    twice = [c[0], c[1], c[1].copy(), c[2]]
    dist, shift, cframe = NR.nearest([c[1][3:3 + W]], twice, W, 1, 0)[0]
    assert dist[0] == 0 and NR.song_frame(cframe, NR.offsets(twice))[0][0] == 1
    # one note per frame on key 10; the corpus holds it on 9 and 10 (s = -1 and s = 0 both at distance 0), then on 8 and 12
    q = np.zeros((W, D), np.uint8)
    q[:, 10] = 1
    at = lambda k: NR.shifted(q, k - 10)
    d, s, g = NR.nearest([q], [at(9), at(10)], W, 1, 2)[0]
    assert (d[0], s[0], g[0]) == (0, 0, W)
    d, s, g = NR.nearest([q], [at(12), at(8)], W, 1, 2)[0]
    assert (d[0], s[0], g[0]) == (0, -2, W)
    same(NR.nearest([q], [at(12), at(8)], W, 1, 2), NR.nearest_loops([q], [at(12), at(8)], W, 1, 2))


def test_exclude_removes_the_self_match():
    c = corpus3(4)
    plain = NR.nearest(c, c, W, 1, 0)
    loo = NR.nearest(c, c, W, 1, 0, exclude=[0, 1, 2])
    off = NR.offsets(c)
    for n in range(3):
        assert (plain[n][0] == 0).all()
        song, frame = NR.song_frame(plain[n][2], off)
        assert (song == n).all() and (frame == np.arange(len(frame))).all()
        assert (loo[n][0] > 0).all() and (NR.song_frame(loo[n][2], off)[0] != n).all()
    same(loo, NR.nearest_loops(c, c, W, 1, 0, exclude=[0, 1, 2]))


def test_no_window_straddles_two_corpus_pieces():
    c = corpus3(5)
    h = W // 2
    trap = np.concatenate([c[0][-h:], c[1][:h]], 0)                    # contiguous in the corpus's string of frames
    dist, _, cframe = NR.nearest([trap], c, W, 1, 0)[0]
    assert dist[0] > 0
    glued = [np.concatenate([c[0], c[1]], 0), c[2]]                    # the same frames as ONE piece: found
    dist, _, cframe = NR.nearest([trap], glued, W, 1, 0)[0]
    assert dist[0] == 0 and cframe[0] == c[0].shape[0] - h


def test_short_pieces_and_an_empty_corpus():
    rng = np.random.default_rng(6)
    q = rolls(rng, [W - 1, W, 0], D)
    c = rolls(rng, [W - 1, 0, W - 1], D)
    for fn in (NR.nearest, NR.nearest_loops):
        res = fn(q, c, W, 1, 2)
        assert [len(r[0]) for r in res] == [0, 1, 0]
        assert (res[1][0][0], res[1][1][0], res[1][2][0]) == (-1, 0, -1)
    res = NR.nearest(q, rolls(rng, [W], D), W, 1, 2, exclude=[0, 0, 0])          # the only piece excluded
    assert (res[1][0][0], res[1][1][0], res[1][2][0]) == (-1, 0, -1)
    assert NR.n_windows(W - 1, W, 1) == 0 and NR.n_windows(W, W, 3) == 1 and NR.n_windows(W + 3, W, 3) == 2
    assert NR.song_frame([-1, 0, W - 2, W - 1], NR.offsets(c))[0].tolist() == [-1, 0, 0, 2]       # the empty piece owns no frame
    np.testing.assert_array_equal(NR.notes_per_window(np.ones((5, 3)), 2, 2), [6, 6])
