"""The long-double reference of lombscargle (tests/_lomb_ref.py) held to what does not depend on it; CPU only.

    1  scipy.signal.lombscargle where scipy imports: unit weights, no floating mean, scipy = p N / 2, to 1e-13
    2  a pure sinusoid on a frequency of the grid: a, b, c come back and the standard power is 1 (fit_mean)
    3  the standard power does not change under y -> alpha y + beta (fit_mean)
    4  the degenerate rule at f = 0 and at the Nyquist alias of a uniform record
    5  the phases: exact products, so a shift of t by whole periods of f changes nothing
    6  the phases of INEXACT products at 3e6 turns (the GPU tests' late records) against rational arithmetic"""
import numpy as np
import pytest

from _lomb_ref import LD, exact_turns, lomb_ref


def _record(seed=0, N=400, periods=40.0):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, int(periods * 1024), N)) / 1024.0        # multiples of 2^-10 over `periods` units
    y = np.cos(2 * np.pi * 1.25 * t + 0.3) + 0.5 * rng.standard_normal(N)
    f = np.arange(1, 97) / 64.0 * 2.0                                    # multiples of 2^-5 up to 3
    return t, y, f


def test_scipy_agrees_on_the_classical_periodogram():
    signal = pytest.importorskip("scipy.signal")
    t, y, f = _record()
    r = lomb_ref(y, t, f, fit_mean=False, center_data=False, normalization="psd")
    want = signal.lombscargle(t, y, 2 * np.pi * f)
    got = r["power"][:, 0].astype(np.float64)
    assert np.max(np.abs(got - want) / np.max(np.abs(want))) < 1e-13
    assert np.max(np.abs(got - want) / np.abs(want)) < 1e-11             # every frequency, also the small ones


def test_pure_sinusoid_on_a_grid_frequency_comes_back():
    t, _, f = _record(1)
    a0, b0, c0, k = 0.75, -1.5, 3.25, 17
    y = c0 + a0 * np.cos(2 * np.pi * f[k] * t) + b0 * np.sin(2 * np.pi * f[k] * t)
    for center in (True, False):
        r = lomb_ref(y, t, f, fit_mean=True, center_data=center)
        assert abs(float(r["a"][k, 0]) - a0) < 1e-13 and abs(float(r["b"][k, 0]) - b0) < 1e-13 and abs(float(r["c"][k, 0]) - c0) < 1e-13
        assert abs(float(r["power"][k, 0]) - 1.0) < 1e-13
        assert np.all(r["power"] <= 1 + 1e-15) and np.all(r["power"] >= 0)
        assert int(np.argmax(r["power"][:, 0])) == k


def test_standard_power_is_invariant_under_affine_maps_of_the_signal():
    t, y, f = _record(2)
    W = np.random.default_rng(3).uniform(0.5, 2.0, len(t))
    p0 = lomb_ref(y, t, f, W=W)["power"]
    for center in (True, False):
        p1 = lomb_ref(-3.5 * y + 11.0, t, f, W=W, center_data=center)["power"]
        assert np.max(np.abs(p1 - p0)) < 1e-13
    ym = np.stack([y, -3.5 * y + 11.0], axis=1)                          # two signals in one call
    pm = lomb_ref(ym, t, f, W=W)["power"]
    assert np.max(np.abs(pm[:, 0] - p0[:, 0])) < 1e-16 and np.max(np.abs(pm[:, 1] - p0[:, 0])) < 1e-13   # (numpy's products reorder the sums)


def test_zero_frequency_and_the_nyquist_alias_are_degenerate():
    t = np.arange(64) * 0.25                                             # uniform: the alias of 0 is 1 / (2 dt) = 2
    y = np.random.default_rng(4).standard_normal(64)
    f = np.array([0.0, 0.5, 2.0, 1.0])
    for fit_mean in (True, False):
        r = lomb_ref(y, t, f, fit_mean=fit_mean)
        assert r["degenerate"].tolist() == [True, False, True, False]
        for k in (0, 2):
            assert r["power"][k, 0] == 0 and r["a"][k, 0] == 0 and r["b"][k, 0] == 0 and r["c"][k, 0] == 0
        assert r["power"][1, 0] > 0 and r["D"][1] > 0.01
    const = lomb_ref(np.full(64, 2.5), t, f)                            # YY = 0: the standard power is 0
    assert np.all(const["power"] == 0)


def test_phases_are_those_of_the_exact_product():
    f = np.array([0.1, 1.0 / 3.0, 7.3])
    t = np.array([3.0e9 + 0.123, 1.0e15 + 0.5, 12345.678])
    u = exact_turns(f, t)
    assert u.dtype == LD and np.all(np.abs(u) <= 1.0)              # 1/2 + the product's rounding error, itself at most 1/2
    from fractions import Fraction
    for i in range(3):
        for j in range(3):
            q = Fraction(float(f[i])) * Fraction(float(t[j]))
            d = Fraction(float(u[i, j])) + Fraction(float(u[i, j] - LD(float(u[i, j])))) - q    # a whole number of turns, up to 2^-64
            assert abs(d - round(d)) < Fraction(1, 2 ** 62)


def test_phases_of_inexact_products_at_three_million_turns():
    """The GPU tests' second family of inputs (late_times, wide_freqs): every product f t is inexact and reaches 3e6 turns.  exact_turns
    against rational arithmetic: hi + lo of the long double minus f t is a whole number to 2^-62, for lattice and full-mantissa times."""
    from fractions import Fraction
    from _lomb_ref import late_times, wide_freqs
    rng = np.random.default_rng(11)
    f = wide_freqs(rng, 12)
    for lattice in (True, False):
        t = late_times(rng, 25, lattice)
        t[-1] = 2.0 ** 20 - 2.0 ** -10                                   # the far end of the record
        p = f[:, None] * t[None, :]
        assert np.all(p != np.rint(p)) and p.max() > 2.0e6
        inexact = sum(Fraction(float(a)) * Fraction(float(b)) != Fraction(float(a * b)) for a in f for b in t)
        assert inexact >= 0.95 * f.size * t.size                         # (a product that happens to be exact is no harm)
        u = exact_turns(f, t)
        assert u.dtype == LD and np.all(np.abs(u) <= 0.5 + 2.0 ** -30)
        for i in range(len(f)):
            for j in range(len(t)):
                q = Fraction(float(f[i])) * Fraction(float(t[j]))
                d = Fraction(float(u[i, j])) + Fraction(float(u[i, j] - LD(float(u[i, j])))) - q
                assert abs(d - round(d)) < Fraction(1, 2 ** 62), (i, j)
