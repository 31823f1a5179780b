"""oracle.gram_ld (oracle/lpvs_oracle_ld.c: lpvo_gram_ld) on its own, no GPU: the long-double Gram that tests/test_gpu_gram_dense.py holds
every dense Gram kernel instance to must itself be right -- against exact rational arithmetic, against int64 products, and, at every shape the
GPU test uses, a plain f64 product of the same regressor must sit inside the GPU test's bound (tests/_gram_ref.py) with a wide margin: the
bound prices a summation order, so a reference that another f64 summation misses would be the wrong reference."""
from fractions import Fraction

import numpy as np
import pytest

import _gram_ref as R


def test_gram_ld_equals_exact_rational_arithmetic(oracle):
    rng = np.random.default_rng(5)
    N, n = 7, 5
    Phi, y, W = rng.standard_normal((N, n)) * 10.0 ** rng.integers(-3, 4, (N, n)), rng.standard_normal(N), rng.random(N) + 0.1
    for Wc in (None, W):
        G, S, b, s = oracle.gram_ld(Phi, y, Wc)
        fw = [Fraction(1) if Wc is None else Fraction(float(v)) for v in W]
        for a in range(n):
            for c in range(n):
                terms = [fw[k] * Fraction(float(Phi[k, a])) * Fraction(float(Phi[k, c])) for k in range(N)]
                assert G[a, c] == float(sum(terms)) and S[a, c] == float(sum(abs(t) for t in terms)), (a, c)
            terms = [fw[k] * Fraction(float(Phi[k, a])) * Fraction(float(y[k])) for k in range(N)]
            assert b[a] == float(sum(terms)) and s[a] == float(sum(abs(t) for t in terms)), a
        assert np.all(S >= np.abs(G)) and np.all(s >= np.abs(b)) and np.array_equal(G, G.T) and np.array_equal(S, S.T)


@pytest.mark.parametrize("N", [333, 1500])
def test_gram_ld_is_exact_on_the_integer_family(oracle, N):
    A, y = R.integer_family(N)
    Y2 = np.stack([y, -2 * y + 1], axis=1)
    Wi = np.arange(N) % 3 + 1.0
    Ai, Yi = A.astype(np.int64), Y2.astype(np.int64)
    G, S, b, s = oracle.gram_ld(A, Y2)
    assert np.array_equal(G, Ai.T @ Ai) and np.array_equal(S, np.abs(Ai).T @ np.abs(Ai))
    assert np.array_equal(b, Ai.T @ Yi) and np.array_equal(s, np.abs(Ai).T @ np.abs(Yi)) and b.shape == (300, 2)
    Gw, Sw, bw, sw = oracle.gram_ld(A, y, Wi)
    Wl = Wi.astype(np.int64)
    assert np.array_equal(Gw, Ai.T @ (Wl[:, None] * Ai)) and np.array_equal(bw, Ai.T @ (Wl * Yi[:, 0])) and bw.shape == (300,)
    assert np.all(Sw >= np.abs(Gw)) and np.all(sw >= np.abs(bw))


def _check_numpy_inside_bound(oracle, Phi, y, W, N, name):
    G, S, b, s = oracle.gram_ld(Phi, y, W)
    assert np.all(S >= np.abs(G)) and np.all(s >= np.abs(b))
    assert S.min() > 1e-200 and s.min() > 1e-200, (name, S.min(), s.min())
    WP = Phi if W is None else W[:, None] * Phi
    rg = R.worst_ratio(Phi.T @ WP, G, N, S)
    rb = R.worst_ratio(WP.T @ y, b, N, s)
    print(f"{name}: f64 numpy product vs long double, worst |diff| / bound: G {rg:.4f}, b {rb:.4f}; min S {S.min():.2e}")
    assert rg <= 1.0 and rb <= 1.0, (name, rg, rb)
    return rg, rb


_SHAPES = {(c[1], c[2], c[3], c[7]): c for c in reversed(R.LPV_CASES) if c[2] > 1}      # one case per distinct input (forms of one shape share it)


def test_a_single_basis_function_has_no_finite_regressor(oracle):
    """Nv = 1 (nb = 1, the only way to gram_kernel<0,16> below nb = 312): the reference's gamma = Nv / |vc[1] - vc[end]| is 1 / 0
    (src/utilities.jl:23-36), the activation at the sample V = min V is exp(-inf * 0) = NaN and normalising spreads it over every row.
    So the two Nv = 1 cases of the GPU test can assert which instance ran and that the NaN arrives, but no entry: the entrywise check of
    gram_kernel<0,16> is the nb = 320 case."""
    case = next(c for c in R.LPV_CASES if c[2] == 1)
    y, X, V, w = R.lpv_inputs(case)
    assert np.isnan(oracle.lpv_regressor(X, V, w, 1, True, False, permuted=True)).all()
    Phi = oracle.lpv_regressor(X, V, w, 1, False, False, permuted=True)
    assert np.isnan(Phi[np.argmin(V)]).all() and np.isnan(Phi.T @ Phi).all()


@pytest.mark.parametrize("case", list(_SHAPES.values()), ids=[c[0] for c in _SHAPES.values()])
def test_numpy_product_of_the_lpv_regressor_is_inside_the_bound(oracle, case):
    cid, Nf, Nv, N, _, _, _, normalize, _ = case
    y, X, V, w = R.lpv_inputs(case)
    Phi = oracle.lpv_regressor(X, V, w, Nv, normalize, False, permuted=True)
    _check_numpy_inside_bound(oracle, Phi, y, None, N, cid)


@pytest.mark.parametrize("case", R.FOURIER_CASES, ids=R.FOURIER_IDS)
def test_numpy_product_of_the_fourier_regressor_is_inside_the_bound(oracle, case):
    y, t, f, W = R.fourier_inputs(case)
    A, zf = oracle.get_fourier_regressor(t, f)
    assert A.shape[1] == 2 * case[1] - int(case[2])
    _check_numpy_inside_bound(oracle, A, y, W, case[4], case[0])


def test_plan_mirror_matches_the_shapes_the_gpu_test_states():
    """The tile / chunk arithmetic the GPU test asserts, on the shapes the cases were chosen for."""
    p = R.plan("krs", 280, 1500, 70, 2)
    assert (p["tile_rows"], p["tile_cols"], p["ksplit"], p["rows_per_chunk"]) == (2, 2, 3, 512)
    p = R.plan("krs", 320, 1500, 8, 20)
    assert (p["tile_rows"], p["tile_cols"]) == (1, 14)
    assert R.plan("krs", 2470, 1500, 65, 19)["tile_rows"] == 2
    assert R.plan("kr", 300, 333)["ksplit"] == 1 and R.plan("kr", 300, 333)["rows_per_chunk"] == 384
    for case in R.LPV_CASES:
        p = R.plan(case[5], 2 * case[1] * case[2], case[3], case[1], case[2])
        assert p["tile_cols"] >= 2, case[0]


@pytest.mark.parametrize("case", R.STRUCT_LPV_CASES, ids=[c[0] for c in R.STRUCT_LPV_CASES])
def test_phase_exact_lpv_gram_against_the_rounded_phase_product(oracle, case):
    """oracle.gram_phase_ld differs from the f64 product of the oracle's regressor by the half-ulp of phase the latter rounds away and a
    summation order: far inside the pair-scale bound the structured forms are held to."""
    _, Nf, Nv, N = case
    y, X, V, w = R.struct_lpv_inputs(case)
    K = oracle.basis_activation(V, Nv)
    G = oracle.gram_phase_ld(X, w, K)
    Phi = oracle.lpv_regressor(X, V, w, Nv)
    C = np.abs(K).T @ np.abs(K)
    j = np.arange(2 * Nf * Nv) % Nv
    r = np.abs(G - Phi.T @ Phi) / (R.struct_tol(w.max(), np.abs(X).max()) * C[np.ix_(j, j)])
    print(f"{case[0]}: f64 product vs phase-exact long double, worst ratio to the pair-scale bound {r.max():.4f}")
    assert np.array_equal(G, G.T) and r.max() <= 0.1


@pytest.mark.parametrize("case", R.STRUCT_FOURIER_CASES, ids=[c[0] for c in R.STRUCT_FOURIER_CASES])
def test_phase_exact_fourier_gram_against_the_rounded_phase_product(oracle, case):
    _, Nf, zero, weighted, N = case
    y, t, f, W = R.struct_fourier_inputs(case)
    A, zf = oracle.get_fourier_regressor(t, f)
    G = oracle.gram_phase_ld(t, 6.283185307179586 * f, None, zero, W)
    Wv = np.ones(N) if W is None else W
    scale = np.abs(Wv).sum() / (2 * Nf) * R.struct_tol(2 * np.pi * f.max(), t.max())
    r = np.abs(G - A.T @ (Wv[:, None] * A)).max() / scale
    print(f"{case[0]}: f64 product vs phase-exact long double, worst ratio to the weight-sum bound {r:.4f}")
    assert G.shape == (A.shape[1],) * 2 and r <= 0.1
