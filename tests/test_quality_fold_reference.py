"""tests/quality_fold_reference.py pinned: fold_sum against a scalar, loop-by-loop emulation of qPass / qBlockReduce / qFold
(csrc/kernels_quality.hpp) by bits, and lowest_extreme on hand-made arrays.  No GPU."""
import math

import numpy as np
import pytest

from quality_fold_reference import fold_sum, fold_sum_scalar, lowest_extreme, same_bits, tied

# under one wave, under one round, one full workgroup, one element into the second, three workgroups, more than 256 records
SIZES = (1, 63, 255, 2048, 2049, 5000, 531441)


@pytest.mark.parametrize("n", SIZES)
def test_fold_sum_is_the_scalar_emulation(n):
    x = np.random.default_rng(n).standard_normal(n) * 10.0 ** np.random.default_rng(n + 1).integers(-3, 4, n)
    v, s = fold_sum(x), fold_sum_scalar(x)
    print(f"    n {n}: fold {v!r} scalar {s!r} numpy {float(np.sum(x))!r} fsum {math.fsum(x)!r}")
    assert same_bits(v, s), (n, v, s)
    assert abs(v - math.fsum(x)) <= 1e-12 * float(np.abs(x).sum())          # (a sum of x at all)


def test_fold_sum_is_an_order_not_just_a_sum():
    """the check discriminates: at some of the sizes the fold differs from numpy's and from the exact sum in the last bits"""
    differs = 0
    for n in SIZES:
        x = np.random.default_rng(n).standard_normal(n) * 10.0 ** np.random.default_rng(n + 1).integers(-3, 4, n)
        differs += not (same_bits(fold_sum(x), np.sum(x)) and same_bits(fold_sum(x), math.fsum(x)))
    assert differs >= 2


def test_fold_sum_edges():
    assert fold_sum(np.zeros(0)) == 0.0
    assert same_bits(fold_sum([-0.0]), 0.0)                                  # the lane starts from +0.0
    x = np.arange(1.0, 4097.0)
    assert fold_sum(x) == 4096 * 4097 / 2                                    # exact in any order
    big = np.zeros(2049); big[0], big[1], big[2048] = 1e16, 1.0, -1e16       # 1e16 + 0 ... in lane 0, 1.0 in lane 1, -1e16 in workgroup 1
    assert same_bits(fold_sum(big), fold_sum_scalar(big))


def test_lowest_extreme_ties_and_empty():
    x = np.array([3.0, 1.0, 2.0, 1.0, 5.0, 5.0, 1.0])
    assert lowest_extreme(x, kind="min") == (1.0, 1)
    assert lowest_extreme(x, kind="max") == (5.0, 4)
    assert list(tied(x, kind="min")) == [1, 3, 6] and list(tied(x, kind="max")) == [4, 5]
    # the tie in first, middle and last position of the domain
    assert lowest_extreme(np.array([1.0, 1.0, 2.0]), kind="min") == (1.0, 0)
    assert lowest_extreme(np.array([2.0, 1.0, 1.0, 3.0]), kind="min") == (1.0, 1)
    assert lowest_extreme(np.array([2.0, 3.0, 1.0, 1.0]), kind="min") == (1.0, 2)
    assert lowest_extreme(np.array([2.0, 3.0, 1.0, 3.0]), kind="max") == (3.0, 1)
    # the domain decides, not the array
    m = np.array([False, False, True, False, True, True, True])
    assert lowest_extreme(x, m, "min") == (1.0, 6)
    assert lowest_extreme(x, m, "max") == (5.0, 4)
    assert list(tied(x, m, "min")) == [6]
    # empty: the documented value and no id
    none = np.zeros(7, dtype=bool)
    assert lowest_extreme(x, none, "min", empty=1.0) == (1.0, -1)
    assert lowest_extreme(x, none, "max") == (0.0, -1)
    assert lowest_extreme(np.zeros(0), kind="min", empty=1.0) == (1.0, -1)
    assert tied(x, none).size == 0
    # the value is the winning element's own bits
    v, i = lowest_extreme(np.array([0.5, -0.0, 0.0]), kind="min")
    assert i == 1 and same_bits(v, -0.0)
