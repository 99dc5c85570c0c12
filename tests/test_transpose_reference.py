"""No GPU: the numpy reference of clv_gather_transposed (tests/transpose_reference.py) on hand-written cases -- the k-th-set-bit
rule, the empty mask, label accumulation through a map that is not injective, the frame edges -- and the uniformity of its draw."""
import numpy as np
import pytest

import transpose_reference as TR

D = 88


def test_kth_set_bit_on_hand_written_masks():
    assert [TR.kth_set_bit(0b1, 0), TR.kth_set_bit(0b1000, 0), TR.kth_set_bit(0b1010, 1)] == [0, 3, 3]
    m = 0b1_0010_0110_0001
    assert [TR.kth_set_bit(m, k) for k in range(5)] == [0, 5, 6, 9, 12]
    assert TR.kth_set_bit((1 << 25) - 1, 24) == 24
    with pytest.raises(ValueError):
        TR.kth_set_bit(0b101, 2)


def test_pick_maps_the_uniform_onto_the_set_bits():
    K = 2                                            # bits 0..4 = shifts -2..2
    m = 0b10110                                      # shifts -1, 0, 2
    assert TR.pick(m, K, 0.0) == -1 and TR.pick(m, K, 0.33) == -1
    assert TR.pick(m, K, 0.34) == 0 and TR.pick(m, K, 0.66) == 0
    assert TR.pick(m, K, 0.67) == 2 and TR.pick(m, K, np.float32(1.0) - np.float32(2 ** -24)) == 2
    assert TR.pick(m, K, 1.0) == 2                   # k is clamped to n - 1
    assert TR.pick(m | 0b1100000, K, 0.99) == 2      # bits above 2K are masked away
    assert TR.pick(0b00100, K, 0.7) == 0
    # the clamp is live: the largest 24-bit word gives (16777215 + 0.5) * 2^-24, which fp32 rounds to exactly 1.0
    assert (np.float32(16777215) + np.float32(0.5)) * np.float32(1.0 / 16777216.0) == np.float32(1.0)


def test_an_empty_mask_gives_shift_zero():
    assert TR.pick(0, 6, 0.5) == 0
    assert TR.pick(0b11 << 13, 6, 0.5) == 0          # only bits above 2K
    got = TR.draw_shifts([0, 0, 0], 4, seed=7, step=3)
    assert got.dtype == np.int32 and (got == 0).all()


def test_labels_accumulate_through_a_non_injective_map():
    K, C = 1, 4
    cmap = np.array([[1, 1, -1, 1],        # shift -1: classes 0, 1 and 3 all land on 1, class 2 is dropped
                     [0, 1, 2, 3],
                     [3, -1, 3, 0]], np.int32)
    w = np.array([[0.25, 0.5, 0.125, 0.0625]], np.float32)
    store = np.zeros((1, D), np.uint8)
    for bit, want in ((0, [0, 0.8125, 0, 0]), (1, [0.25, 0.5, 0.125, 0.0625]), (2, [0.0625, 0, 0, 0.375])):
        _, w_out, shifts = TR.gather_transposed(1, None, 0, 0, [(store, D, D, 0, None)], w, [1 << bit], cmap, K, seed=1, step=0)
        assert shifts[0] == bit - K
        np.testing.assert_array_equal(w_out[0], np.array(want, np.float32))


def test_no_byte_crosses_a_frame_edge():
    # frame 0 ends with note 87 on, frame 1 starts with note 0 on, frame 2 is full
    store = np.zeros((3, D), np.uint8)
    store[0, 87] = store[1, 0] = 1
    store[2, :] = 1
    for s in (1, -1, 12, -12):
        K = abs(s)
        outs, _, shifts = TR.gather_transposed(1, None, 0, 0, [(store, 3 * D, 3 * D, 0, None)], None, [1 << (s + K)], None, K, 5, 0)
        assert shifts[0] == s
        f = outs[0][0]
        if s > 0:
            assert f[0].sum() == 0 and f[1, s] == 1 and f[1].sum() == 1          # note 87 left the keyboard, nothing came in
            assert (f[2, :s] == 0).all() and (f[2, s:] == 1).all()
        else:
            assert f[0, 87 + s] == 1 and f[0].sum() == 1 and f[1].sum() == 0
            assert (f[2, D + s:] == 0).all() and (f[2, :D + s] == 1).all()
    np.testing.assert_array_equal(TR.shift_frame(np.arange(D, dtype=np.uint8), 0), np.arange(D, dtype=np.uint8))


def test_rows_idx_cursor_and_tables_pick_the_source_row():
    assert TR.cursor_base(0, None) == 0
    assert [TR.cursor_base(s, (2, 3, 10, 4)) for s in (2, 3, 4, 5, 1)] == [4, 14, 24, 4, 24]
    idx = np.array([5, 3, 9, 1])
    np.testing.assert_array_equal(TR.source_rows(2, idx, 0, 1), [3, 9])
    np.testing.assert_array_equal(TR.source_rows(3, None, 2, 10), [12, 13, 14])
    rng = np.random.default_rng(0)
    store = (rng.random((12, D)) < 0.2).astype(np.uint8)
    table = np.array([4, 0, 7])
    allowed = np.full(3, 1 << 6, np.uint32)          # K = 6, shift 0 only
    outs, _, sh = TR.gather_transposed(2, np.array([2, 0]), 0, 0, [(store, 2 * D, D, D, table)], None, allowed, None, 6, 1, 0)
    assert (sh == 0).all()
    np.testing.assert_array_equal(outs[0][0], store[8:10])
    np.testing.assert_array_equal(outs[0][1], store[5:7])


UNIFORM_SEED, UNIFORM_ROWS = 20261, 65536


@pytest.mark.parametrize("n", [2, 3, 11, 13, 25])
def test_the_draw_is_uniform_over_the_allowed_shifts(n):
    """65 536 rows with the same mask of n set bits: every allowed shift's share is within 4 standard deviations of 1 / n"""
    K = 12
    rng = np.random.default_rng(n)
    bits = np.sort(rng.choice(2 * K + 1, n, replace=False))
    m = int(sum(1 << int(b) for b in bits))
    sh = TR.draw_shifts(np.full(UNIFORM_ROWS, m, np.uint32), K, UNIFORM_SEED, step=n, first_row=1000 * n)
    assert set(np.unique(sh).tolist()) <= set((bits - K).tolist())
    sd = np.sqrt((1.0 / n) * (1 - 1.0 / n) / UNIFORM_ROWS)
    for b in bits:
        share = float(np.mean(sh == b - K))
        assert abs(share - 1.0 / n) <= 4 * sd, (n, int(b) - K, share, 1.0 / n, sd)
