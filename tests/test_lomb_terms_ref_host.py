"""The long-double reference of lombscargle(..., nterms=K) (tests/_lomb_terms_ref.py) checked on its own, CPU only:
  K = 1 is the single-term reference of tests/_lomb_ref.py;
  the fit (c, theta) it returns satisfies the weighted normal equations of the EXPLICIT N x (2K + 1) design matrix -- which knows nothing
  of the product identities behind A -- and 1 - chi^2 / chi_0^2 of that residual is the power;
  a planted record with harmonics 1, 2 and 3 has power 1 from three terms on and clearly less below."""
import functools

import numpy as np
import pytest

from _lomb_ref import LD, TWO_PI, exact_turns, lomb_ref
from _lomb_terms_ref import lomb_terms_ref

EPS_LD = float(np.finfo(LD).eps)


@functools.lru_cache(maxsize=None)
def _record(N, ns, seed=0):
    """The record of tests/test_gpu_lomb.py."""
    rng = np.random.default_rng(1000 * N + 10 * ns + seed)
    t = rng.integers(0, 40 * 1024, N) / 1024.0
    if N != 1000:
        t = np.sort(t)
    y = np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(ns)[None, :]) * (1.0 + np.arange(ns))[None, :] + 0.5 * rng.standard_normal((N, ns)) + 0.75
    W = rng.uniform(0.5, 2.0, N)
    return t, y, W


def planted(t, f0=1.25):
    """y = 0.75 + cos phi + 0.5 sin(2 phi + 0.3) - 0.25 cos 3 phi, phi = 2 pi f0 t from the exact turns, rounded once to double."""
    phi = TWO_PI * exact_turns([f0], t)[0]
    return (LD(0.75) + np.cos(phi) + LD(0.5) * np.sin(2 * phi + LD(0.3)) - LD(0.25) * np.cos(3 * phi)).astype(np.float64)


F = np.array([4, 9, 33, 80, 81, 150, 192]) / 64.0


@pytest.mark.parametrize("fit_mean,center", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("normalization", ["standard", "psd"])
def test_one_term_is_the_single_term_reference(fit_mean, center, normalization):
    t, y, W = _record(255, 3)
    f = np.concatenate([[0.0], F])                                            # f = 0: degenerate in both
    one = lomb_ref(y, t, f, W=W, fit_mean=fit_mean, center_data=center, normalization=normalization)
    r = lomb_terms_ref(y, t, f, 1, W=W, fit_mean=fit_mean, center_data=center, normalization=normalization)
    assert np.array_equal(r["degenerate"], one["degenerate"]) and r["degenerate"][0] and not r["degenerate"][1:].any()
    for got, want in ((r["power"], one["power"]), (r["a"][0], one["a"]), (r["b_h"][0], one["b"]), (r["c"], one["c"])):
        scale = np.abs(want)
        assert np.all(np.abs(got - want) <= 64 * EPS_LD * scale), float(np.max(np.abs(got - want) / scale)) / EPS_LD
    for k, k1 in (("C", "C"), ("S", "S")):
        assert np.array_equal(r[k][0], one[k1]) and np.array_equal(r[k][1], one[k1 + "2"])
    assert np.array_equal(r["YC"][:, 0], one["YC"]) and np.array_equal(r["Y"], one["Y"]) and np.array_equal(r["YY"], one["YY"])


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("center", [True, False])
def test_the_fit_solves_the_normal_equations_of_the_explicit_design_matrix(K, center):
    t, y, W = _record(255, 3)
    r = lomb_terms_ref(y, t, F, K, W=W, fit_mean=True, center_data=center)
    assert not r["degenerate"].any()
    w = (W / LD(1)).astype(LD)
    w = w / w.sum()
    yl = y.astype(LD)
    turns = exact_turns(F, t)
    tol = 1e-15 * (w[:, None] * np.abs(yl)).sum(axis=0)
    for k in range(len(F)):
        X = np.ones((len(t), 2 * K + 1), dtype=LD)
        for h in range(1, K + 1):
            X[:, 2 * h - 1], X[:, 2 * h] = np.cos(TWO_PI * (h * turns[k])), np.sin(TWO_PI * (h * turns[k]))
        coef = np.concatenate([r["c"][k][None, :], r["theta"][k].T], axis=0)  # (2K + 1, ns)
        res = yl - X @ coef
        grad = X.T @ (w[:, None] * res)
        assert np.all(np.abs(grad) <= tol[None, :]), (k, float(np.max(np.abs(grad) / tol[None, :])))
        # 1 - chi^2 / chi_0^2, chi_0^2 about the weighted mean
        chi2 = (w[:, None] * res * res).sum(axis=0)
        mean = (w[:, None] * yl).sum(axis=0)
        chi0 = (w[:, None] * (yl - mean[None, :]) ** 2).sum(axis=0)
        assert np.all(np.abs((1 - chi2 / chi0) - r["power"][k]) <= 1e-15), k


def test_without_fit_mean_the_fit_is_that_of_the_design_matrix_without_a_constant():
    t, y, W = _record(255, 3)
    K = 3
    r = lomb_terms_ref(y, t, F, K, W=W, fit_mean=False, center_data=True)
    w = W.astype(LD) / W.astype(LD).sum()
    yc = y.astype(LD) - r["removed"][None, :]
    turns = exact_turns(F, t)
    tol = 1e-15 * (w[:, None] * np.abs(yc)).sum(axis=0)
    for k in range(len(F)):
        X = np.zeros((len(t), 2 * K), dtype=LD)
        for h in range(1, K + 1):
            X[:, 2 * h - 2], X[:, 2 * h - 1] = np.cos(TWO_PI * (h * turns[k])), np.sin(TWO_PI * (h * turns[k]))
        grad = X.T @ (w[:, None] * (yc - X @ r["theta"][k].T))
        assert np.all(np.abs(grad) <= tol[None, :]), k
        assert np.array_equal(r["c"][k], r["removed"])


def test_a_planted_record_of_three_harmonics_needs_three_terms():
    t, _, W = _record(1000, 1)
    y = planted(t)
    got = [float(lomb_terms_ref(y, t, [1.25], K, W=W)["power"][0, 0]) for K in (1, 2, 3, 4)]
    print("power at f0 for 1 .. 4 terms:", got)
    assert got[0] < 0.96 and got[1] < 0.96 and got[0] < got[1]
    assert abs(got[2] - 1) <= 1e-15 and abs(got[3] - 1) <= 1e-15
    r = lomb_terms_ref(y, t, [1.25], 3, W=W)
    want = [1.0, 0.0, 0.5 * np.sin(0.3), 0.5 * np.cos(0.3), -0.25, 0.0]      # (a_1, b_1, a_2, b_2, a_3, b_3)
    assert np.all(np.abs(r["theta"][0, 0] - np.array(want)) <= 1e-15) and abs(float(r["c"][0, 0]) - 0.75) <= 1e-15
