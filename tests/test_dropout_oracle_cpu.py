"""The numpy restatement of the kernels' dropout generator (oracle/dropout_oracle.py): properties that hold without a GPU.
That it is the SAME function as csrc/common.h is what the exact-mask GPU tests check."""
import math

import numpy as np
import pytest

from oracle import dropout_oracle as do


def test_mask_is_deterministic_and_depends_on_the_seed():
    a = do.keep(np.arange(64), np.arange(768), 77, 0.1)
    b = do.keep(np.arange(64), np.arange(768), 77, 0.1)
    c = do.keep(np.arange(64), np.arange(768), 78, 0.1)
    assert a.dtype == np.bool_ and a.shape == (64, 768)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    assert do.seed_mix(77) == do.seed_mix(77) and do.seed_mix(77) != do.seed_mix(78)
    assert 0 <= do.seed_mix(0xFFFFFFFF) < 2 ** 32


def test_p_zero_keeps_everything():
    assert do.thr32(0.0) == 0
    assert do.keep(np.arange(300), np.arange(520), 5, 0.0).all()
    assert do.keep_flat(1000, 5, 0.0).all()


def test_threshold_is_taken_from_the_float32_probability():
    assert do.thr32(0.5) == 2 ** 31
    assert do.thr32(0.1) == int(float(np.float32(0.1)) * 2.0 ** 32 + 0.5)
    assert do.thr32(0.1) != int(0.1 * 2.0 ** 32 + 0.5)      # the launchers' `float p`, not the Python double
    assert do.thr32(1.5) == 2 ** 32 - 1 and do.thr32(-1.0) == 0


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_keep_rate_within_five_sigma(p):
    rows, cols = 4096, 512
    n = rows * cols
    rate = do.keep(np.arange(rows), np.arange(cols), 1234, p).mean()
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(rate - (1 - p)) <= 5 * sigma, (rate, 1 - p, sigma)


def test_rows_and_columns_in_any_order():
    rng = np.random.default_rng(0)
    rows, cols = np.arange(200), np.arange(136)
    full = do.keep(rows, cols, 9, 0.25)
    pr, pc = rng.permutation(rows), rng.permutation(cols)
    assert np.array_equal(do.keep(pr, pc, 9, 0.25), full[np.ix_(pr, pc)])
    assert np.array_equal(do.keep([7, 3, 7], [5], 9, 0.25)[:, 0], full[[7, 3, 7], 5])
    # the flat form of stonk_dropout_f32 is row 0 with the element index as the column
    assert np.array_equal(do.keep_flat(136, 9, 0.25), full[0])
    big = do.keep([0], [262146, 1], 9, 0.25)[0]
    assert big[0] == do.keep_flat(262147, 9, 0.25)[262146] and big[1] == full[0, 1]


# ---- the 4 x 4 block form of the attention probabilities (stonk_blk_round1 / stonk_blk_keep)

def test_block_mask_is_deterministic_and_depends_on_the_seed():
    a = do.keep_block(np.arange(64), np.arange(768), 77, 0.1)
    b = do.keep_block(np.arange(64), np.arange(768), 77, 0.1)
    c = do.keep_block(np.arange(64), np.arange(768), 78, 0.1)
    assert a.dtype == np.bool_ and a.shape == (64, 768)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    assert not np.array_equal(a, do.keep(np.arange(64), np.arange(768), 77, 0.1))   # not the element form
    assert len(set(int(c2) for c2 in do.C2_BLK)) == 16 and all(0 < int(c2) < 2 ** 24 and int(c2) & 1 for c2 in do.C2_BLK)


def test_block_p_zero_keeps_everything():
    assert do.keep_block(np.arange(300), np.arange(520), 5, 0.0).all()
    assert do.attention_keep(3, 1, 2, 256, 65, 65, 5, 0.0).all()


@pytest.mark.parametrize("p", [0.1, 0.25, 0.5])
def test_block_keep_rate_within_five_sigma(p):
    rows, keys = 4096, 512
    n = rows * keys
    rate = do.keep_block(np.arange(rows), np.arange(keys), 1234, p).mean()
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(rate - (1 - p)) <= 5 * sigma, (rate, 1 - p, sigma)


def test_block_members_drop_pairwise_independently():
    """All 120 pairs of the sixteen members of a block, over 2^20 blocks at p = 0.25: every joint drop rate within what
    common.h states for its multipliers (0.3 % of p^2) plus five sigma of the sample."""
    p, row_quads, key_quads = 0.25, 1024, 1024
    blocks = row_quads * key_quads
    joint = np.zeros((16, 16))
    for r0 in range(0, 4 * row_quads, 512):             # (in slabs: 2^24 elements of uint64 intermediates at once otherwise)
        d = ~do.keep_block(np.arange(r0, r0 + 512), np.arange(4 * key_quads), 99, p)
        d = d.reshape(128, 4, key_quads, 4).transpose(0, 2, 1, 3).reshape(-1, 16).astype(np.float32)   # [block, 4 (row & 3) + (key & 3)]
        joint += (d.T @ d).astype(np.float64)
    joint /= blocks
    sigma1 = math.sqrt(p * (1 - p) / blocks)
    assert np.abs(np.diag(joint) - p).max() <= 5 * sigma1, np.diag(joint)
    pairs = joint[np.triu_indices(16, 1)]
    assert pairs.size == 120
    margin = 0.003 * p * p + 5 * math.sqrt(p * p * (1 - p * p) / blocks)
    assert np.abs(pairs - p * p).max() <= margin, (np.abs(pairs - p * p).max(), margin)


def test_block_rows_and_keys_in_any_order():
    rng = np.random.default_rng(0)
    rows, keys = np.arange(200), np.arange(136)
    full = do.keep_block(rows, keys, 9, 0.25)
    pr, pc = rng.permutation(rows), rng.permutation(keys)
    assert np.array_equal(do.keep_block(pr, pc, 9, 0.25), full[np.ix_(pr, pc)])
    assert np.array_equal(do.keep_block([7, 3, 7], [5], 9, 0.25)[:, 0], full[[7, 3, 7], 5])
    # the attention form: row = (b * NH + h) * S + q with the launch's S, key = the index inside the sequence
    a = do.attention_keep(2, 1, 3, 256, 65, 129, 9, 0.25)
    assert a.shape == (65, 129)
    assert np.array_equal(a, do.keep_block((2 * 3 + 1) * 256 + np.arange(65), np.arange(129), 9, 0.25))
    assert np.array_equal(do.attention_keep(0, 0, 3, 256, 65, 129, 9, 0.25), full[:65, :129])
