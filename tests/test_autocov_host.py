"""autocov / autocor (src/autocov.jl): what is decided before any device is needed -- isequidistant on the reference's cases
(test/runtests.jl:306-311 and the [0,1,0,1] quirk of the inner abs), argument errors, and the restatement the GPU tests check
against.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _autocov_ref as R  # noqa: E402


def _collect(a, b, s):
    """Julia's collect(a:s:b) for a decimal step: the doubles nearest to a + k*s computed exactly (the range's twice-precision
    arithmetic recovers s = 33/100 from 0.33), k = 0 .. floor((b-a)/s)."""
    from decimal import Decimal
    a, b, s = Decimal(str(a)), Decimal(str(b)), Decimal(str(s))
    return np.array([float(a + k * s) for k in range(int((b - a) / s) + 1)])


def test_isequidistant_reference_cases(L):
    assert L.isequidistant(range(1, 6))
    assert L.isequidistant(range(1, 10, 2))
    assert not L.isequidistant(range(9, 0, -2))                      # reverse(1:2:10)
    assert L.isequidistant(np.arange(1, 6))
    assert L.isequidistant(np.arange(1, 10, 2))
    assert L.isequidistant(_collect(1, 10, 0.33))
    assert L.isequidistant(np.array([0.0, 1.0, 0.0, 1.0]))            # abs(abs(t[i]-t[i-1]) - d): the inner abs
    assert L.isequidistant(np.float32([0, 1, 0, 1]))
    assert not L.isequidistant(np.array([0.0, 1.0, 3.0]))
    assert not L.isequidistant(np.array([1.0, 0.0, -1.0]))
    assert not L.isequidistant(np.array([0.0, np.nan, 2.0]))
    assert not L.isequidistant(100 * np.random.default_rng(0).random(100))


def test_isequidistant_agrees_with_the_restatement(L):
    rng = np.random.default_rng(1)
    for t in (np.arange(50) * 0.1, np.arange(50, dtype=np.float32) * np.float32(0.1), _collect(1, 10, 0.33), np.array([2, 4, 6, 9]),
              np.cumsum(1 + 1e-15 * rng.random(30)), np.cumsum(1 + 1e-13 * rng.random(30)), np.array([0.0, 1.0])):
        assert L.isequidistant(t) == R.isequidistant(t), t


def test_short_series_is_an_argument_error(L):
    with pytest.raises(ValueError):
        L.isequidistant(np.array([1.0]))
    with pytest.raises(ValueError):
        L.autocov(np.array([1.0]), np.array([2.0]), np.inf)
    with pytest.raises(ValueError):
        L.autocor([np.arange(5.0), np.array([1.0])], [np.ones(5), np.ones(1)], np.inf)


def test_length_mismatch_is_an_argument_error(L):
    with pytest.raises(ValueError, match="same length"):
        L.autocov(np.arange(5.0), np.ones(4), np.inf)
    with pytest.raises(ValueError, match="same length"):
        L.autocor(range(1, 4), np.ones(5), 2.0)


def test_restatement_semantics():
    """The checker itself on hand-computable cases."""
    tau, acf, _ = R.autofun("cov", np.array([0.0, 2.0, 1.0]), np.array([1.0, 2.0, 3.0]), np.inf)
    # pairs (i, i+j) in enumeration order: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); tau 0 2 1 0 1 0
    assert tau.tolist() == [0, 0, 0, 1, 1, 2] and acf.tolist() == [1, 4, 9, 3, 6, 2]
    tau, acf, _ = R.autofun("cov", range(1, 4), np.array([1.0, 2.0, 3.0]), np.inf, normalize=True)
    assert tau.dtype == np.int64 and tau.tolist() == [0, 0, 0, 1, 1, 2]
    assert np.allclose(acf, [14 / 4, 14 / 4, 14 / 4, 8 / 3, 8 / 3, 3 / 2])   # divisor N - (j-1)
