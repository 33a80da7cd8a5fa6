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
