"""The host side of the regularisation path: lambda_grid against literals, lambda_max's two formulas against the CPU oracle, the refusals.
No GPU: lambda_max reads a handle's right-hand side through get_rhs(), which a stand-in supplies here.

Bounds.  lambda_grid's end points are exact by construction (ratio ** 0.0 == 1 and ratio ** 1.0 == ratio in IEEE pow, one rounding in
the product with lmax, which the literals below do not need); an interior point is lmax * pow(ratio, k / (count - 1)): the quotient, pow
and the product round once each, pow's argument error is amplified by |ln ratio| <= 7 for ratio >= 1e-3 -- 16 ulp covers it.  The oracle
runs to ||x - z|| < 1e-9: at 1.01 lambda_max the KKT conditions at x = 0 hold strictly (|b_i| <= lambda / 1.01), so near the fixed point
v = x + u lies strictly inside the threshold and the soft threshold returns EXACTLY zero; at 0.9 lambda_max x = 0 violates them and the
solution is non-zero."""
import numpy as np
import pytest


class _Rhs:
    """What lambda_max reads of a Problem."""
    def __init__(self, b, weighted=False):
        self._b = np.asarray(b, dtype=np.float64)
        self.n, self.ns, self.weighted = self._b.shape[0], (1 if self._b.ndim == 1 else self._b.shape[1]), weighted

    def get_rhs(self):
        return self._b


def test_lambda_grid_literals(L):
    assert L.lambda_grid(8.0, 1).tolist() == [8.0]
    assert L.lambda_grid(8.0, 2, ratio=0.125).tolist() == [8.0, 1.0]
    assert L.lambda_grid(8.0, 3, ratio=0.25).tolist() == [8.0, 4.0, 2.0]              # pow(0.25, 0.5) = 0.5 exactly
    assert L.lambda_grid(3.0, 5, ratio=1.0).tolist() == [3.0] * 5
    g = L.lambda_grid(0.7, 8)
    assert g.shape == (8,) and g[0] == 0.7 and g[-1] == 0.7 * 1e-3                    # the default ratio, end points exact
    assert np.all(np.diff(g) < 0)
    r = g[1:] / g[:-1]
    assert np.all(np.abs(r - 1e-3 ** (1 / 7)) <= 16 * 2.0 ** -53 * r)                 # geometric
    for bad in (dict(lmax=1.0, count=0), dict(lmax=0.0, count=3), dict(lmax=1.0, count=3, ratio=0.0), dict(lmax=1.0, count=3, ratio=2.0)):
        with pytest.raises(ValueError):
            L.lambda_grid(**bad)


def test_lambda_max_formulas_on_literals(L):
    b = np.array([1.0, -7.0, 3.0, 4.0, 0.0, -6.0])
    assert L.lambda_max(_Rhs(b), L.NormL1) == 7.0
    assert L.lambda_max(_Rhs(b), L.NormL1(2.0)) == 7.0                                # a prox object or the PROX_* id name the kind too
    assert L.lambda_max(_Rhs(b), L.SlicedSeparableSum, group_len=2) == np.sqrt(50.0)  # groups (1, -7), (3, 4), (0, -6)
    assert L.lambda_max(_Rhs(b), L.SlicedSeparableSum, group_len=4) == np.sqrt(75.0)  # one whole group; the tail (0, -6) is in no slice
    assert L.lambda_max(_Rhs(b), L.SlicedSeparableSum.frequency_groups(1.0, 2, 3)) == np.sqrt(59.0)
    B = np.stack([b, 2 * b], axis=1)
    assert L.lambda_max(_Rhs(B), L.NormL1).tolist() == [7.0, 14.0]                    # one value per signal


def test_lambda_max_refusals(L):
    b = np.ones(6)
    for g in (L.NormL0, L.IndBallL0, L.NormL0(1.0), L.IndBallL0(3)):
        with pytest.raises(ValueError):
            L.lambda_max(_Rhs(b), g)
    with pytest.raises(ValueError):
        L.lambda_max(_Rhs(b, weighted=True), L.NormL1)                                # the as-written weighted Quadratic
    with pytest.raises(ValueError):
        L.lambda_max(_Rhs(b), L.SlicedSeparableSum)                                   # no group length


@pytest.fixture(scope="module")
def gram60():
    rng = np.random.default_rng(60)
    A = rng.standard_normal((200, 60))
    y = A[:, [3, 17, 40]] @ np.array([2.0, -1.5, 1.0]) + 0.1 * rng.standard_normal(200)
    return A.T @ A, A.T @ y


@pytest.mark.parametrize("form", ["l1", "group"])
def test_lambda_max_against_the_oracle(L, oracle, gram60, form):
    G, b = gram60
    if form == "l1":
        lmax, make = L.lambda_max(_Rhs(b), L.NormL1), oracle.NormL1
    else:
        lmax, make = L.lambda_max(_Rhs(b), L.SlicedSeparableSum, group_len=4), (lambda lam: oracle.GroupL2(lam, 4))
    above = oracle.admm_gram(G, b, make(1.01 * lmax), iters=20000, tol=1e-9, mu=0.05)
    below = oracle.admm_gram(G, b, make(0.9 * lmax), iters=20000, tol=1e-9, mu=0.05)
    assert not np.any(above["z"]), "1.01 lambda_max must give z = 0 exactly"
    assert np.any(below["z"]), "0.9 lambda_max must leave a non-zero z"
