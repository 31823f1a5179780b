"""tests/_refine_ref.py without a GPU: the family is exact, the exact residual is exact, the exact-arithmetic models of the three refined solves of
csrc/admm_refine.hip sit inside their bounds -- and the SAME recurrences with a residual that is only as good as plain doubles, or as x87 long
doubles, or with no refinement at all, do not: the evidence that tests/test_gpu_refine.py fails on a kernel that lost its compensation term.
numpy's LAPACK inverse stands in for the device's."""
from fractions import Fraction

import numpy as np
import pytest

import _refine_ref as R


@pytest.fixture(scope="module")
def host():
    """(family, numpy inverse and what the bounds need of it) per n, built once."""
    cache = {}

    def get(n):
        if n not in cache:
            F = R.family(n)
            cache[n] = (F, R.Inverse(F, np.linalg.inv(F.H)))
        return cache[n]
    return get


@pytest.mark.parametrize("n", [200, 513, 2100])
def test_family_is_exact_and_has_the_chosen_spectrum(n):
    F = R.family(n)
    assert sum(F.orders) == n and F.d.min() == 1 and F.d.max() == 2 ** R.LOG2_COND
    Hint = (F.H * F.m).astype(np.int64)
    assert np.array_equal(Hint.astype(np.float64) / F.m, F.H) and np.abs(Hint).max() < 2 ** 53             # m H: integers, H: no rounding
    if n <= 513:          # the dense definition, block by block, by integer matrix products (n = 2100: half a minute of them)
        B = np.zeros((n, n), dtype=np.int64)
        for o, mk in zip(F.offsets, F.orders):
            W = R.hadamard(mk)
            assert np.array_equal(W @ W.T, mk * np.eye(mk, dtype=np.int64))
            B[o:o + mk, o:o + mk] = (W * F.d[o:o + mk]) @ W.T * (F.m // mk)
        P = np.zeros((n, n), dtype=np.int64)
        P[F.perm, np.arange(n)] = 1
        assert np.array_equal(P @ B @ P.T, Hint)
    X = np.random.default_rng(n).integers(-2 ** 13, 2 ** 13 + 1, (n, 3))
    assert np.array_equal(F.apply_int(X), Hint @ X)
    assert np.array_equal(F.b * F.m, Hint @ F.xstar.astype(np.int64)) and np.abs(F.xstar).max() == 8
    assert np.array_equal(F.G, F.G.T) and np.array_equal(F.G + np.eye(n), F.H) and np.array_equal(F.absH, np.abs(F.H))
    # dense within a block, every block scattered over the matrix
    assert np.count_nonzero(F.H) == sum(mk * mk for mk in F.orders)
    ev = np.linalg.eigvalsh(F.H)
    assert np.max(np.abs(ev - np.sort(F.d))) <= 1e-9 * 2 ** R.LOG2_COND
    assert abs(ev[-1] / ev[0] / 2 ** R.LOG2_COND - 1) <= 1e-9
    assert abs(np.linalg.eigvalsh(F.G)[0]) <= 1e-9                                 # G = H - I is singular: the shift holds it up


def test_exact_residual_is_exact_on_rows_done_in_rationals(host):
    F, inv = host(200)
    rng = np.random.default_rng(1)
    x = (inv.A @ F.b[:, 0]) * np.where(rng.random(200) < 0.1, 2.0 ** -40, 1.0)       # 53-bit entries, some forty binades down
    x[3], x[7] = 0.0, 2.0 ** -300
    b = F.b[:, 0] + rng.standard_normal(200)                                      # any doubles, not only the family's
    hi, lo = R.exact_residual(F, b, x)
    for i in range(0, 200, 7):
        r = Fraction(float(b[i])) - sum(Fraction(float(F.H[i, j])) * Fraction(float(x[j])) for j in range(200))
        assert hi[i] == float(r) and lo[i] == float(r - Fraction(float(hi[i]))), i


@pytest.mark.parametrize("n", [2048, 2100])
def test_exact_residual_agrees_with_long_double(host, n):
    F, inv = host(n)
    b = F.b[:, 0]
    for x in (inv.A @ b, F.xstar[:, 0] + 1e-9 * np.random.default_rng(2).standard_normal(n)):
        hi, lo = R.exact_residual(F, b, x)
        xl = x.astype(np.longdouble)
        rl = b.astype(np.longdouble) - (F.G.astype(np.longdouble) @ xl + xl)
        S = np.abs(b) + F.absH @ np.abs(x)
        worst = float(np.max(np.abs(rl - (hi.astype(np.longdouble) + lo.astype(np.longdouble))) / S))
        print(f"[refine-ref] n = {n}: exact residual vs long double {worst:.2e} of the term sum (2^-60 = {2.0 ** -60:.2e})")
        assert worst <= 2.0 ** -60
        assert np.all(np.abs(lo) <= 0.5 * np.spacing(np.abs(hi)))
    assert np.array_equal(R.exact_residual(F, b, F.xstar[:, 0])[0], np.zeros(n))   # b = H x*, exactly


def _offset_with(F, inv, b, xb0, residual):
    """The device's recurrence xb1 = fl(xb0 + fl(A r^)) in host doubles with the residual formed three ways."""
    if residual == "exact":
        r = R.exact_residual(F, b, xb0)[0]
    elif residual == "double":
        r = b - (F.G @ xb0 + xb0)
    else:
        xl = xb0.astype(np.longdouble)
        r = (b.astype(np.longdouble) - (F.G.astype(np.longdouble) @ xl + xl)).astype(np.float64)
    return xb0 + inv.A @ r


@pytest.mark.parametrize("n", [2048, 2100])
def test_offset_vector_model_meets_its_bounds_and_lesser_residuals_do_not(host, n):
    F, inv = host(n)
    b, xs = F.b[:, 0], F.xstar[:, 0]
    xb0 = inv.A @ b
    assert R.worst_ratio(xb0.astype(np.longdouble) - inv.Ald @ b.astype(np.longdouble), R.product_bound(F, inv, b)) <= 1
    m = R.offset_model(F, inv, b, xb0)
    fwd = R.offset_forward_bound(F, inv, xb0, xs, m["bound"])
    ratios = {}
    for kind in ("exact", "double", "longdouble"):
        xb1 = _offset_with(F, inv, b, xb0, kind)
        ratios[kind] = (R.worst_ratio(xb1.astype(np.longdouble) - m["xb1"], m["bound"]), R.worst_ratio(xb1 - xs, fwd))
    print(f"[refine-ref] n = {n}: cond 2^20, |E|_inf {inv.normE:.2e}, offset-vector bound {m['bound'].max() / (R.U * 8):.2f} u max|x*|; error / bound "
          f"(vs model, vs x*) with the residual rounded once {ratios['exact'][0]:.2e}, {ratios['exact'][1]:.2e}; formed in doubles "
          f"{ratios['double'][0]:.2e}, {ratios['double'][1]:.2e}; in 64-bit-mantissa long doubles {ratios['longdouble'][0]:.2e}, {ratios['longdouble'][1]:.2e}")
    assert inv.normE < 2.0 ** -16
    assert max(ratios["exact"]) <= 1
    assert min(ratios["double"]) > 100 and min(ratios["longdouble"]) > 100


@pytest.mark.parametrize("n", [200, 513, 2100])
def test_ridge_model_meets_its_residual_bound(host, n):
    F, inv = host(n)
    b = F.b[:, 0]
    xs = R.ridge_recurrence(F, inv, b, 2)
    r1 = R.exact_residual(F, b, xs[1])[0]
    r2 = R.exact_residual(F, b, xs[2])[0]
    ratio = R.worst_ratio(r2, R.ridge_residual_bound(F, inv, b, xs[2], r1))
    r0 = R.exact_residual(F, b, xs[0])[0]
    none = R.worst_ratio(r0, R.ridge_residual_bound(F, inv, b, xs[0], r1))
    print(f"[refine-ref] n = {n}: ridge residual / bound after two plain-double steps {ratio:.2e}, with no refinement (A b alone) {none:.3g}")
    assert ratio <= 1
    assert float(np.max(np.abs(xs[2] - F.xstar[:, 0]))) <= float(np.max(inv.absA @ np.abs(r2)))
    if n == 200:
        # gamma_n grows with n, the rounding of A b that the steps remove like sqrt(n): the factor shrinks from 193 (n = 200) over 87 (513)
        # to 18 (2100) with this inverse; asserted where it holds
        assert none > 100
    else:
        assert none > 10                                # a floor at the other sizes: the bound must not drift until a plain A b passes it


def test_correction_model_meets_its_bounds(host):
    F, inv = host(2100)
    n = F.n
    v = np.random.default_rng(4).integers(-8, 9, n).astype(np.float64)
    xb0 = inv.A @ F.b[:, 0]
    m = R.correction_model(F, inv, v, xb0)
    w = inv.A @ v                                                                  # the device's recurrence in host doubles
    ld = lambda d: (xb0 + d).astype(np.longdouble) - xb0.astype(np.longdouble)     # what the test can observe: fl(xb0 + d) - xb0
    got = ld(inv.A @ R.exact_residual(F, v, w)[0])
    plain = ld(inv.A @ (v - (F.G @ w + w)))                                        # ... with the residual in plain doubles
    ratio, tight = R.worst_ratio(got - m["d"], m["bound"]), R.worst_ratio(got - m["d"], m["bound_tight"])
    lost, none = R.worst_ratio(plain - m["d"], m["bound_tight"]), R.worst_ratio(m["d"], m["bound_tight"])
    print(f"[refine-ref] n = {n}: correction max|d| {float(np.abs(m['d']).max()):.2e}, bound {m['bound'].max():.2e} (error / bound {ratio:.2e}), tight bound "
          f"{m['bound_tight'].max():.2e} (error / bound {tight:.2e}; with a plain-double residual {lost:.3g}, with d = 0 {none:.3g}; against the wide bound "
          f"{R.worst_ratio(plain - m['d'], m['bound']):.2e}, {R.worst_ratio(m['d'], m['bound']):.2e})")
    assert ratio <= 1 and tight <= 1
    assert np.all(m["bound_tight"] <= m["bound"])
    assert lost > 4 and none > 4                        # the tight bound sees a lost compensation term and a correction that was not applied


def test_eigenvector_right_hand_side_is_refused_for_its_residual_alone():
    """The case of the residual refusal: exact, positive pivots guaranteed, and two plain-double steps stall four decades above 1e-9."""
    H, b = R.eigenvector_rhs()
    n = len(b)
    assert np.array_equal(H, H.T) and np.array_equal(H @ b, b) and set(np.unique(b)) == {-1.0, 0.0, 1.0}
    ev = np.linalg.eigvalsh(H)
    assert abs(ev[0] - 1) < 1e-5 and ev[-1] == pytest.approx(2.0 ** 36, rel=1e-9)
    assert ev[0] > 100 * R.gamma(n) * ev[-1]
    np.linalg.cholesky(H)
    A = np.linalg.inv(H)
    G = H - np.eye(n)
    assert np.array_equal(G + np.eye(n), H)
    x = A @ b
    for _ in range(2):
        x = x + A @ (b - (G @ x + x))
    rel = float(np.linalg.norm(b - (G @ x + x)) / np.linalg.norm(b))
    print(f"[refine-ref] eigenvector right-hand side: relative residual after two steps {rel:.2e}")
    assert 1e-7 < rel < 1e-3
