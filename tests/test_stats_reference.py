"""CPU tests of tests/stats_reference.py, the yardstick of the roll statistics audit: the reference against
rows counted by hand on rolls of a few frames."""
import numpy as np

import stats_reference as SR


def roll(D, *frames):
    r = np.zeros((len(frames), D), np.uint8)
    for t, f in enumerate(frames):
        r[t, list(f)] = 1
    return r


def hist(n, **at):
    """n zeros with the counts `at` = {bin: count} (keys as b<bin>)"""
    h = np.zeros(n, np.int64)
    for k, v in at.items():
        h[int(k[1:])] = v
    return h


def test_columns_and_sections():
    assert (SR.V, SR.C, SR.M) == (16, 16, 24)
    assert SR.columns(88, 32) == 3 * 88 + 32 + 12 + 17 + 17 + 2 * 49 == 440
    assert SR.columns(1, 1) == 3 + 1 + 12 + 17 + 17 + 98
    s = SR.sections(5, 3)
    assert list(s) == list(SR.NAMES)
    assert s['pitch'] == (0, 5) and s['degree'] == (5, 12) and s['voices'] == (17, 17) and s['interval'] == (34, 5)
    assert s['duration'] == (39, 3) and s['change'] == (42, 17) and s['top_step'] == (59, 49) and s['bottom_step'] == (108, 49)
    assert s['span'] == (157, 5) and SR.columns(5, 3) == 162


def test_a_roll_counted_by_hand():
    """D = 5, four frames {0, 2}, {0, 2, 4}, {}, {1, 4}; low 21 and tonic 9 (A) make the degree of note d just d"""
    p = roll(5, (0, 2), (0, 2, 4), (), (1, 4))
    r = SR.piece_row(p, 5, 3, low=21, tonic=9)
    assert np.array_equal(r['pitch'], [2, 1, 2, 0, 2])
    assert np.array_equal(r['degree'], [2, 1, 2, 0, 2, 0, 0, 0, 0, 0, 0, 0])
    assert np.array_equal(r['voices'], hist(17, b0=1, b2=2, b3=1))
    assert np.array_equal(r['interval'], [0, 0, 3, 1, 1])            # (0,2) twice, (2,4); (1,4); (0,4)
    assert np.array_equal(r['duration'], [3, 2, 0])                  # notes 0 and 2 last two frames; 4, 4 and 1 one frame
    assert np.array_equal(r['change'], hist(17, b1=1, b3=1, b2=1))   # +4; all three off; two on
    assert np.array_equal(r['top_step'], hist(49, b26=1))            # 2 -> 4; the empty frame breaks the other two
    assert np.array_equal(r['bottom_step'], hist(49, b24=1))         # 0 -> 0
    assert np.array_equal(r['span'], [0, 0, 1, 1, 1])
    # the same through table(), in the row's order; low 21 with tonic 0: note d is pitch class (d + 9) % 12
    t = SR.table([p], 5, 3, low=21, tonics=[9])
    assert t.shape == (1, 162) and np.array_equal(t[0], np.concatenate([r[n] for n in SR.NAMES]))
    r0 = SR.piece_row(p, 5, 3, low=21, tonic=0)
    assert np.array_equal(r0['degree'], hist(12, b9=2, b10=1, b11=2, b1=2))
    assert np.array_equal(SR.piece_row(p, 5, 3, low=21, tonic=-1)['degree'], r0['degree'])          # unknown counts as 0
    assert np.array_equal(SR.piece_row(p * 7, 5, 3, low=21, tonic=0)['pitch'], r0['pitch'])         # any non-zero byte sounds


def test_a_held_note_across_a_piece_boundary_is_two_notes():
    a, b = roll(3, (1,), (1,)), roll(3, (1,), (1,))
    t = SR.table([a, b], 3, 8)
    at, n = SR.sections(3, 8)['duration']
    assert np.array_equal(t[0, at:at + n], [0, 1, 0, 0, 0, 0, 0, 0]) and np.array_equal(t[1], t[0])
    one = SR.piece_row(np.concatenate([a, b]), 3, 8)
    assert np.array_equal(one['duration'], [0, 0, 0, 1, 0, 0, 0, 0])
    # neither `change` nor a step sees the other piece: one entry per piece, not three in all
    c, _ = SR.sections(3, 8)['change']
    assert t[:, c].tolist() == [1, 1] and one['change'][0] == 3


def test_a_run_longer_than_lmax_lands_in_the_last_bin():
    p = np.zeros((10, 2), np.uint8)
    p[:, 1] = 1
    p[2:6, 0] = 1
    assert np.array_equal(SR.piece_row(p, 2, 4)['duration'], [0, 0, 0, 2])     # lengths 10 and 4
    assert np.array_equal(SR.piece_row(p, 2, 1)['duration'], [2])
    assert np.array_equal(SR.piece_row(p, 2, 12)['duration'], hist(12, b9=1, b3=1))


def test_steps_are_clamped_and_need_two_sounding_frames():
    up = SR.piece_row(roll(60, (0, 3), (50, 55)), 60, 2)
    assert np.array_equal(up['top_step'], hist(49, b48=1)) and np.array_equal(up['bottom_step'], hist(49, b48=1))
    down = SR.piece_row(roll(60, (50, 55), (0, 30)), 60, 2)
    assert np.array_equal(down['top_step'], hist(49, b0=1)) and np.array_equal(down['bottom_step'], hist(49, b0=1))
    edge = SR.piece_row(roll(60, (30,), (6, 54)), 60, 2)                       # exactly -24 and +24
    assert np.array_equal(edge['top_step'], hist(49, b48=1)) and np.array_equal(edge['bottom_step'], hist(49, b0=1))
    gap = SR.piece_row(roll(8, (3,), (), (5,)), 8, 2)
    assert gap['top_step'].sum() == 0 and gap['bottom_step'].sum() == 0        # the empty frame breaks the steps
    assert np.array_equal(gap['change'], hist(17, b1=2))                       # but not `change`
    assert np.array_equal(gap['voices'], hist(17, b0=1, b1=2)) and gap['span'][0] == 2


def test_voices_and_change_clip_and_a_full_frame_gives_the_largest_interval():
    D = 20
    p = np.zeros((3, D), np.uint8)
    p[1] = 1
    r = SR.piece_row(p, D, 4)
    assert np.array_equal(r['voices'], hist(17, b0=2, b16=1))
    assert np.array_equal(r['change'], hist(17, b16=2))
    assert np.array_equal(r['interval'], [0] + [D - k for k in range(1, D)])
    assert r['span'][D - 1] == 1 and r['span'].sum() == 1
    assert np.array_equal(r['duration'], [D, 0, 0, 0]) and np.array_equal(r['pitch'], np.ones(D))


def test_empty_pieces_and_offsets():
    t = SR.table([np.zeros((0, 7), np.uint8), roll(7, (1,)), np.zeros((0, 7), np.uint8)], 7, 5)
    assert not t[0].any() and not t[2].any() and t[1].sum() == 1 + 1 + 1 + 1 + 1          # pitch, degree, voices, duration, span
    assert SR.offsets([np.zeros((0, 7)), np.zeros((3, 7)), np.zeros((2, 7))]).tolist() == [0, 0, 3, 5]
