"""The reference of wwz (tests/_wwz_ref.py) against Foster's own formulation (AJ 112, 1709, 1996), CPU only.

wwz_cell_ref is lomb_ref -- the floating-mean fit with the phase origin t = 0 -- of a cell's slice under the weights W g, plus Neff, Z and
the amplitude.  wwz_foster is the explicit weighted least squares on Foster's design matrix [1, cos w (t - tau), sin w (t - tau)], his
Vx and Vy, Z = (Neff - 3) Vy / (2 (Vx - Vy)) and WWA = sqrt(y_2^2 + y_3^2).  Both are long double.  They have to agree in everything that
does not depend on the phase origin (Z, WWA, Vy / Vx = power, Neff, the constant), and Foster's (y_2, y_3) have to be (a, b) rotated by
2 pi f tau: that is the proof that sharing the phases of t = 0 among all times changes nothing but (a, b)."""
import numpy as np
import pytest

from _lomb_ref import LD
from _wwz_ref import decay, radius, reach, wwz_cell_ref, wwz_foster

TOL = 1e-13                                   # long double carries 1e-19; the 3 x 3 systems here are conditioned below 1e4


def _record(N=400, span=100.0, seed=3):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, int(span * 1024), N)) / 1024.0
    y = np.where(t < span / 2, np.cos(2 * np.pi * 1.25 * t), np.cos(2 * np.pi * 2.5 * t + 0.3)) + 0.3 * rng.standard_normal(N) + 2.0
    W = rng.uniform(0.5, 2.0, N)
    return t, y, W


def test_decay_and_radius_are_the_stated_doubles():
    f = np.array([0.25, 1.0, 3.0])
    c = 1.0 / (8.0 * np.pi ** 2)
    w = 6.283185307179586 * f
    assert np.array_equal(decay(c, f), c * (w * w))
    assert np.allclose(decay(c, f), f * f / 2, rtol=1e-15)                     # Foster's default: exp(-f^2 d^2 / 2)
    r = radius(f, c, 1e-9)
    assert np.allclose(np.exp(-decay(c, f) * r * r), 1e-9, rtol=1e-12)         # the weight at the edge of the reach is wmin
    assert np.allclose(r * f, np.sqrt(2 * np.log(1e9)), rtol=1e-15)            # 6.44 periods, whatever the frequency
    assert np.all(np.isinf(radius(f, c, 0)))


def test_reach_is_searchsorted_on_the_stated_edges():
    t = np.array([0.0, 1.0, 1.0, 2.0, 3.0, 5.0])
    assert reach(t, 2.0, 1.0) == (1, 4)                                        # [1, 3]: both ties at 1 and the 3 are inside
    assert reach(t, 10.0, 1.0) == (6, 0) and reach(t, -4.0, 1.0) == (0, 0)
    assert reach(t, 2.0, np.inf) == (0, 6)


@pytest.mark.parametrize("with_W", [True, False])
@pytest.mark.parametrize("c", [1.0 / (8.0 * np.pi ** 2), 1.0 / (128.0 * np.pi ** 2)])
def test_the_cell_reference_is_fosters_projection(c, with_W):
    t, y, W = _record()
    W = W if with_W else None
    worst = 0.0
    for f in (0.5, 1.25, 2.5, 2.984375):
        a, r = decay(c, f), radius(f, c, 1e-9)
        for tau in (-1.0, 10.0, 37.5, 50.0, 77.25, 101.0):
            ref = wwz_cell_ref(y, t, W, f, tau, a, r)
            if ref is None or ref["count"] < 6:
                continue
            F = wwz_foster(y, t, W, f, tau, a, r)
            assert not ref["degenerate"]
            th = 2 * np.arccos(LD(-1)) * (LD(f) * LD(tau))
            a2, b2 = ref["a"][0] * np.cos(th) + ref["b"][0] * np.sin(th), ref["b"][0] * np.cos(th) - ref["a"][0] * np.sin(th)
            z = F["Z"] if ref["neff"] > 3 else LD(0)                              # (the rule of g8: no degrees of freedom left)
            pairs = [(ref["wwz"][0], z), (ref["amplitude"][0], F["WWA"]), (ref["power"][0], F["Vy"] / F["Vx"]), (ref["neff"], F["neff"]),
                     (ref["c"][0], F["coef"][0]), (a2, F["coef"][1]), (b2, F["coef"][2]), (ref["YYf"][0], F["Vx"]), (ref["p"][0], F["Vy"])]
            for got, want in pairs:
                err = float(abs(got - want) / max(abs(want), LD(1e-3)))
                worst = max(worst, err)
                assert err <= TOL, (f, tau, got, want)
    assert worst > 0                                                          # (cells were compared)
    print("worst relative difference:", worst)


def test_empty_cells_and_the_rules():
    t, y, W = _record()
    c = 1.0 / (8.0 * np.pi ** 2)
    assert wwz_cell_ref(y, t, W, 3.0, 200.0, decay(c, 3.0), radius(3.0, c, 1e-9)) is None      # out of reach of every sample
    # Neff <= 3: a cell that holds few samples, all the weight on one or two of them
    ref = wwz_cell_ref(y, t, W, 3.0, t[0] - 1.5, decay(c, 3.0), radius(3.0, c, 1e-9))
    assert ref is not None and ref["neff"] <= 3 and np.all(ref["wwz"] == 0)
    # a constant signal: standard power 0, Z = 0
    ref = wwz_cell_ref(np.full(len(t), 7.0), t, W, 1.25, 50.0, decay(c, 1.25), radius(1.25, c, 1e-9))
    assert np.all(ref["power"] == 0) and np.all(ref["wwz"] == 0)
    # an exact fit: Z = inf
    ref = wwz_cell_ref(3.0 + np.cos(2 * np.pi * 1.25 * t), t, None, 1.25, 50.0, decay(c, 1.25), radius(1.25, c, 1e-9))
    assert abs(ref["power"][0] - 1) < 1e-15 and (np.isinf(ref["wwz"][0]) or ref["wwz"][0] > 1e15)
