"""tests/_eval_ref.py on its own, no GPU: the long-double reference that tests/test_gpu_predict.py holds predict / residual / fva to must
itself be the regressor times the coefficients, and the tolerance the type-2 path is held to must be reachable -- a numpy model of its
three steps (coefficients / phihat, grid synthesis, 16-point interpolation, with the rotation and the first-order twin) is held to the
reference within struct_tol * S_m at every fine grid it can take, two of them filled to the 3.9x limit."""
import numpy as np
import pytest

import _eval_ref as E

LD = np.longdouble


def _coefs(rng, n, nc=1):
    return (rng.standard_normal((n, nc)) + 1j * rng.standard_normal((n, nc))) * 10.0 ** rng.integers(-2, 2, (n, 1))


@pytest.mark.parametrize("normalize,coulomb", [(True, False), (False, False), (True, True)])
def test_reference_is_the_lpv_regressor_times_the_coefficients(oracle, normalize, coulomb):
    rng = np.random.default_rng(11)
    Nf, Nv, M = 24, 3, 700
    nb = 2 * Nv if coulomb else Nv
    X, V = rng.uniform(-3.0, 5.0, M), rng.uniform(-1.0, 1.0, M)
    w = np.sort(rng.uniform(0.4, 6.0, Nf))
    P = _coefs(rng, Nf * nb, 2)
    vc, gamma = oracle.basis_centers(V, Nv, coulomb)
    yh, S = E.evaluate_ld(P, w, X, E.activations_ld(V, vc, gamma, normalize, coulomb))
    Phi = oracle.lpv_regressor(X, V, w, Nv, normalize, coulomb, permuted=False)
    ref = Phi.astype(LD) @ E.stack_re_im(P).astype(LD)
    assert S.min() > 0
    ratio = float(np.max(np.abs(yh - ref) / E.direct_bound(Nf, nb, S)))
    print(f"normalize={normalize} coulomb={coulomb}: worst |reference - regressor product| / bound = {ratio:.4f}")
    assert ratio <= 1.0                                              # the regressor's own roundings: a few ulps per entry


@pytest.mark.parametrize("zero", [False, True])
def test_reference_is_the_fourier_regressor_times_the_coefficients(oracle, zero):
    rng = np.random.default_rng(12 + zero)
    Nf, M = 40, 600
    t = np.cumsum(0.5 + rng.random(M))
    f = np.sort(rng.uniform(0.01, 0.45, Nf))
    if zero:
        f[0] = 0.0
    p = _coefs(rng, Nf)[:, 0]
    if zero:
        p[0] = p[0].real                                             # the sine column of the zero frequency does not exist
    yh, S = E.evaluate_ld(p, E.fourier_w(f), t, None, E.fourier_scale_ld(Nf))
    A, zf = oracle.get_fourier_regressor(t, f)
    assert bool(zf) == zero
    ref = A.astype(LD) @ E.fourier_real_vector(p, zf).astype(LD)
    ratio = float(np.max(np.abs(yh[:, 0] - ref) / E.direct_bound(Nf, 1, S[:, 0])))
    print(f"zero={zero}: worst |reference - regressor product| / bound = {ratio:.4f}")
    assert ratio <= 1.0


def _planted(rng, D, M, xmax):
    """Samples whose reduced phase D x sits at 0, at 1e-9, at 2 pi - 1e-9 and at pi (the 16 taps wrap round the grid's ends), then random."""
    x = rng.uniform(-xmax, xmax, M)
    x[:4] = np.array([0.0, 1e-9, 2 * np.pi - 1e-9, np.pi]) / D + 2 * np.pi / D * np.array([0.0, 3.0, -2.0, 5.0])
    return x


@pytest.mark.parametrize("Nf,start", [(24, 0), (24, 1), (65, 1), (512, 0), (2100, 1)])
def test_type2_model_is_inside_the_structured_tolerance(Nf, start):
    rng = np.random.default_rng(100 + Nf + start)
    D = 2 * np.pi / 7.0
    w = D * np.arange(start, start + Nf)                             # start = 0: a = 0 and a zero frequency; 1: a = D, the rotation
    x = _planted(rng, D, 300, 50.0)
    p = _coefs(rng, Nf)[:, 0]
    yh, S = E.evaluate_ld(p, w, x)
    got = E.type2_model(p, w, x).real
    tol = E.struct_tol(np.abs(w).max(), np.abs(x).max())
    ratio = float(np.max(np.abs(got - yh[:, 0]) / (tol * S[:, 0])))
    print(f"Nf={Nf} nf={E.grid_size(Nf)} start={start}: worst |model - reference| / (struct_tol S_m) = {ratio:.4f}")
    assert E.grid_size(Nf) == {24: 256, 65: 256, 512: 2048, 2100: 8192}[Nf]
    assert ratio <= 1.0


def test_first_order_twin_carries_the_residuals():
    """Residuals with emax * max|x| = 5e-8 (admitted: below 1e-7): with the twin the model holds the tolerance, without it it is off by
    the residual phase itself, four orders of magnitude above the tolerance."""
    rng = np.random.default_rng(7)
    Nf, D = 24, 2 * np.pi / 7.0
    x = _planted(rng, D, 300, 50.0)
    xam = np.abs(x).max()
    eps = rng.uniform(-1.0, 1.0, Nf)
    eps[0] = eps[-1] = 0.0                                            # the end points define a and D
    eps *= 5e-8 / (np.abs(eps).max() * xam)
    w = D * np.arange(1, Nf + 1) + eps
    p = _coefs(rng, Nf)[:, 0]
    yh, S = E.evaluate_ld(p, w, x)
    tol = E.struct_tol(np.abs(w).max(), xam)
    with_twin = float(np.max(np.abs(E.type2_model(p, w, x).real - yh[:, 0]) / (tol * S[:, 0])))
    without = float(np.max(np.abs(E.type2_model(p, w, x, twin=False).real - yh[:, 0]) / (tol * S[:, 0])))
    print(f"worst |model - reference| / (struct_tol S_m): with the twin {with_twin:.4f}, without {without:.1f}")
    assert with_twin <= 1.0 and without > 1e3
