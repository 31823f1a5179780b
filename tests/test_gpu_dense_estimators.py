"""Every dense estimator's solve against a componentwise backward error (tests/_dense_ref.py): ls_spectral tall, fat and weighted and
its _f32 entry, ls_spectral_lpv with its Sigma, the dense estimator of the window engine with the sums on top of it, and lpvs_windowpsd_lpv_f64.
GPU only; tests/test_dense_ref_host.py shows without one that a correct solver passes every case with room and that the planted mutations miss.

Metric: omega(x^) = max_i |Phi'(W .* (y - Phi x^)) - rho x^|_i / ((E |x^|)_i + f_i) <= 1 on the regressor the library itself materialises, in long
double, E and f from the Gram bound of the form that ran plus c_s = 2 rounds of gamma_(np+2) (derived in tests/_dense_ref.py).  Nothing grows with
cond(H).  Every test prints its figures; DESIGN 6.6 tabulates them next to LAPACK's on the same inputs.

Measured on an MI355X (DESIGN.md 6.6 has the table): omega of the primal cases 1e-4 .. 7e-3, of the dual cases 1e-3 .. 9e-3 (cond <= 10) and
0.02 .. 0.10 (cond 4e5 .. 6e6), of the window engine 2e-4 .. 8e-3 including the default lam at cond(H) = 7e9, of ls_spectral_lpv 7e-5 .. 5e-3.  On a
library built from the fat branch as it was before its refinement the mid-conditioned dual cases sit at omega = 59 .. 4240, and the first refusal
case came back 5 % wrong without an error.

Sigma takes the inverse itself, and the inverse of the blocked sweep loses sqrt(cond) where it eliminates more than one 128-block: 341 u |M||H||M|
at n = 144 (cond(H) = 1.1e5) where numpy's is at 4.9 and the one-block cases at 0.5 .. 7.2 (Demmel, Higham, Schreiber 1995: block elimination on
a positive definite matrix).  Sigma of that case sat at 2.18 of its tolerance; ls_spectral_lpv now takes the inverse refined once on the device
(lpvs_problem_get_inverse_refined_f64), and the test prints the raw and the refined ratio next to numpy's."""
import ctypes as C

import numpy as np
import pytest

import _dense_ref as D
from _guards import precondition_not_met

pytestmark = pytest.mark.gpu


def _held(name, om, idx):
    print(f"{name}: omega {om:.3g} (entry {idx})")
    assert om <= 1.0, (name, om, idx)


# ---------------------------------------------------------------------------------------------------------------- ls_spectral, primal
@pytest.mark.parametrize("cid", [c[0] for c in D.PRIMAL_CASES])
def test_ls_spectral_primal(L, cid):
    case = D.PRIMAL[cid]
    _, nreg, zero, N, weighted, lam, fj, _ = case
    y, t, f, W, rho = D.primal_inputs(case)
    A, zf = L.get_fourier_regressor(t, f)
    assert A.shape == (N, nreg) and bool(zf) == zero
    with L.Problem.fourier(y, t, f, W) as p:                        # the handle the estimator builds from the same inputs
        form = p.timing()["gram_form"]
    assert form == ("panel" if fj else "ap"), form
    x, _ = L.ls_spectral(y, t, f, W, λ=lam)
    om, idx, _ = D.omega(A, W, y, rho, D.complex2fourier(x, zero), form, sys=D.fourier_system(A, t, f, y, W, rho, form))
    _held(f"{cid} ({form})", om, idx)


@pytest.mark.parametrize("cid,dual", [("n127-N333", False), ("n129-N129", False), ("N=nreg-1", True), ("N=257", True)])
def test_ls_spectral_f32_entry_is_the_f64_call_on_the_widened_inputs(L, cid, dual):
    """lpvs_ls_spectral_f32 widens exactly, calls the f64 entry and rounds once: bit for bit the f64 call on the widened inputs, as complex64."""
    if dual:
        y, t, f = D.dual_inputs(next(c for c in D.DUAL_CASES if c[0] == cid and c[4] == "well"))
    else:
        y, t, f = D.primal_inputs(D.PRIMAL[cid])[:3]
    y32, t32, f32 = (np.asarray(a, dtype=np.float32) for a in (y, t, f))
    x32, _ = L.ls_spectral(y32, t32, f32)
    x64, _ = L.ls_spectral(y32.astype(np.float64), t32.astype(np.float64), f32.astype(np.float64))
    assert x32.dtype == np.complex64 and x64.dtype == np.complex128 and np.all(np.isfinite(x32))
    assert np.array_equal(x32, x64.astype(np.complex64))


# ---------------------------------------------------------------------------------------------------------------- ls_spectral, dual
@pytest.mark.parametrize("case", D.DUAL_CASES, ids=[D.dual_id(c) for c in D.DUAL_CASES])
def test_ls_spectral_dual(L, case):
    """x^ = A' alpha^ held to the primal-form omega with rho = lam^2 (np: the padded order of the dual system, ldn = round_up(N, 256) its panel)."""
    cid, nreg, zero, N, grade, _ = case
    y, t, f = D.dual_inputs(case)
    A, zf = L.get_fourier_regressor(t, f)
    assert A.shape == (N, nreg) and N < nreg and bool(zf) == zero
    lam = D.DUAL_LAM
    x, _ = L.ls_spectral(y, t, f, λ=lam)
    om, idx, _ = D.omega(A, None, y, lam * lam, D.complex2fourier(x, zero), "panel", sys=D.fourier_system(A, t, f, y, None, lam * lam, "panel", nsolve=N))
    _held(D.dual_id(case), om, idx)


# ---------------------------------------------------------------------------------------------------------------- the refusal group
def _ls_spectral_entry(y, t, f, lam):
    """lpvs_ls_spectral_f64 itself -> (return code, message, re + i im)."""
    from lpvspectral_jl_amd._lib import lib
    y, t, f = (np.ascontiguousarray(a, dtype=np.float64) for a in (y, t, f))
    re, im = np.zeros(len(f)), np.zeros(len(f))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib().lpvs_ls_spectral_f64(ptr(y), ptr(t), len(y), ptr(f), len(f), float(lam), 0, ptr(re), ptr(im))
    return rc, lib().lpvs_last_error().decode(), re + 1j * im


@pytest.mark.parametrize("case", D.REFUSAL_CASES, ids=[c[0] for c in D.REFUSAL_CASES])
def test_fat_system_beyond_normal_equations_is_refused_or_right(L, case):
    """cond(A A' + lam^2 I) u >= 1.  The C entry must refuse (LPVS_ENUMERIC, the message naming the dual system) or be within 1e-6 of the
    extended-precision minimiser; ls_spectral, which takes the host route on a refusal, must be within 1e-6.  A silently wrong answer fails."""
    y, t, f = D.refusal_inputs(case)
    A, _ = L.get_fourier_regressor(t, f)
    lam = D.DUAL_LAM
    xs = D.fat_solution_ld(A, y, lam)
    e_np = D.rel_l2(D.numpy_route(np.asarray(A), y, lam), xs)
    if not e_np <= 1e-7:
        precondition_not_met(f"{case[0]}: numpy's route on the device's regressor at {e_np:.3g} > 1e-7 of the extended-precision solution")
    rc, msg, xc = _ls_spectral_entry(y, t, f, lam)
    if rc == 0:
        e = D.rel_l2(D.complex2fourier(xc, False), xs)
        print(f"{case[0]}: the device solve returned, rel-L2 {e:.3g}")
        assert e <= 1e-6, (case[0], "silently wrong", e)
    else:
        print(f"{case[0]}: refused ({rc}): {msg}")
        assert rc == -7, (rc, msg)                                   # LPVS_ENUMERIC
        assert "dual" in msg or "positive definite" in msg, msg
    x, _ = L.ls_spectral(y, t, f, λ=lam)
    e = D.rel_l2(D.complex2fourier(x, False), xs)
    print(f"{case[0]}: ls_spectral rel-L2 {e:.3g} (numpy's route {e_np:.3g})")
    assert e <= 1e-6, (case[0], e)


def test_lpv_more_unknowns_than_samples_host_route_coefficients(L):
    """ls_spectral_lpv at n = 80 > N = 60 with the default lam = 1e-8 (tests/test_gpu_regressions.py holds the fit): the coefficients, too."""
    Y, X, V, w, Nv = D.refusal_lpv_inputs()
    Phi = L.lpv_regressor(X, V, w, Nv, permuted=True)
    xs = D.ridge_solution_ld(Phi, Y, 1e-8)
    e_np = D.rel_l2(D.numpy_route(np.asarray(Phi), Y, 1e-8), xs)
    if not e_np <= 1e-7:
        precondition_not_met(f"numpy's route on the device's regressor at {e_np:.3g} > 1e-7")
    for cov in (False, True):
        try:
            se = L.ls_spectral_lpv(Y, X, V, w, Nv, covariance=cov)
        except L.NumericError as e:
            print(f"covariance={cov}: refused: {e}")
            continue
        e = D.rel_l2(D.lpv_complex2permuted(se.x, len(w), Nv), xs)
        print(f"covariance={cov}: rel-L2 {e:.3g} (numpy's route {e_np:.3g})")
        assert e <= 1e-6, (cov, e)


# ---------------------------------------------------------------------------------------------------------------- ls_spectral_lpv and Sigma
@pytest.mark.parametrize("cid", [c[0] for c in D.LPV_CASES])
def test_ls_spectral_lpv_coefficients_and_sigma(L, cid):
    """Coefficients to omega <= 1 with and without Sigma; Sigma entry by entry against var_e_ld P M_ld P' on the device's own Gram, tolerance
    8 r u var_e |M||H||M| + |d var_e| |M| with r numpy's own worst |inv(H) - M_ld| / (u |M||H||M|) on the same H."""
    case = D.LPV[cid]
    _, Nf, Nv, N, coulomb, normalize, prog, lam = case
    nb = 2 * Nv if coulomb else Nv
    Y, X, V, w = D.lpv_inputs(case)
    Phi = L.lpv_regressor(X, V, w, Nv, normalize, coulomb, permuted=True)
    with L.Problem.lpv_multi(np.stack([Y, np.ones(N)], axis=1), X, V, w, Nv, normalize, coulomb) as p:     # the handle of covariance = True
        form = p.timing()["gram_form"]
        G, _ = p.get_gram()
        B = p.get_rhs()
        M_dev = p.get_inverse(lam)
        M_ref = p.get_inverse_refined(lam)
    with L.Problem.lpv(Y, X, V, w, Nv, normalize, coulomb) as p:
        assert p.timing()["gram_form"] == form
    assert form == ("ap" if prog else "krs"), form
    kw = {}
    if prog:
        kw = dict(wmax=float(w.max()), xmax=float(np.abs(X).max()), pair=D.lpv_pair_scale(L.basis_activation_func(V, Nv, normalize, coulomb), Nf, Y))
    sys = D.system(Phi, None, Y, lam * lam, form, **kw)
    x = None
    for cov in (False, True):
        se = L.ls_spectral_lpv(Y, X, V, w, Nv, λ=lam, coulomb=coulomb, normalize=normalize, covariance=cov)
        x = D.lpv_complex2permuted(se.x, Nf, nb)
        om, idx, _ = D.omega(Phi, None, Y, lam * lam, x, form, sys=sys)
        _held(f"{cid} ({form}, covariance={cov})", om, idx)
    # Sigma = var(e) P inv(G + lam I) P' entry by entry on the device's own G
    var_e, _, _ = D.lpv_stats_ld(Phi, Y, x)
    dvar = D.var_e_bound(sys, x, Y, B[:, 1])
    M, T = D.inverse_scale(G, lam)
    r_np = D.inverse_ratio(np.linalg.inv(G + lam * np.eye(G.shape[0])), M, T)
    r_dev, r_ref = D.inverse_ratio(M_dev, M, T), D.inverse_ratio(M_ref, M, T)
    assert np.array_equal(M_ref, M_ref.T)
    perm = D.lpv_unpermutation(Nf, nb)
    tol = (8 * r_np * D.U * float(var_e) * T + dvar * np.abs(M))[np.ix_(perm, perm)]
    ratio = D.ratio_where(np.asarray(se.Σ) - D.sigma_ld(var_e, M, Nf, nb), tol)
    print(f"{cid}: inverse error / (u |M||H||M|): the sweep's {r_dev:.3g}, refined once {r_ref:.3g}, numpy {r_np:.3g}; Sigma at {ratio:.3g} of the tolerance (8 x numpy's ratio)")
    assert ratio <= 1.0, (cid, ratio, r_dev, r_ref, r_np)


# ---------------------------------------------------------------------------------------------------------------- the window engine
def _engine(lam):
    from lpvspectral_jl_amd import _lib
    return dict(estimator=_lib.EST_DENSE, lam=lam, prox=(_lib.PROX_L1, 0.0, 0), μ=0.05, tol=0.0, iters=0, sign=_lib.LINEAR_LEAST_SQUARES)


@pytest.mark.parametrize("cid", [c[0] for c in D.WINDOW_CASES])
def test_window_engine_dense_estimator(L, monkeypatch, cid):
    from lpvspectral_jl_amd import api
    case = D.WINDOWS[cid]
    _, n, nwin, ns, grid, window, lam, tj, sub, env, form = case
    Y, t, f, W = D.window_inputs(case)
    Wd = np.ones(n) if W is None else W                               # the drivers always pass the window vector (rect: ones)
    zero = f[0] == 0
    if env:
        monkeypatch.setenv("LPVS_NUDFT", env)
    else:
        monkeypatch.delenv("LPVS_NUDFT", raising=False)
    lo, hi = sub if sub else (0, None)
    x, _ = L.windows_estimate(Y, t, f, n, 0, Wd, _engine(lam), win_lo=lo, win_hi=hi)
    tm = api.windowpsd_last_timing()
    ranges = D.window_ranges(case)
    assert x.shape == (ns, len(ranges), len(f))
    assert tm["gram_form"] == form and tm["passes"] == 1 and tm["windows"] == len(ranges), tm
    worst = (0.0, None)
    for k, (i, sl) in enumerate(ranges):
        A, _ = L.get_fourier_regressor(t[sl], f)
        for q in range(ns):
            y = Y[q][sl]
            om, idx, _ = D.omega(A, Wd, y, lam, D.complex2fourier(x[q, k], zero), form, sys=D.fourier_system(A, t[sl], f, y, Wd, lam, form))
            if om > worst[0]:
                worst = (om, (i, q, idx))
    _held(f"{cid} ({form})", worst[0], worst[1])
    if sub is None:
        wf = dict(rect=L.rect, hann=lambda m: L.hanning(m) + 0.1, hann0=L.hanning)[window]
        assert np.array_equal(np.asarray(wf(n), dtype=np.float64), Wd), "the case's window is the library's"
        # S of ls_windowpsd: the in-order host sum of the device's own per-window coefficients
        S, _ = L.ls_windowpsd(Y[0], t, f, nw=nwin, noverlap=0, window_func=wf, λ=lam)
        acc = np.zeros(len(f))
        for k in range(nwin):
            acc += x[0, k].real * x[0, k].real + x[0, k].imag * x[0, k].imag
        assert np.array_equal(S, acc / nwin ** 2)
    if ns >= 2:
        Syu, Syy, Suu, xy, xu = L.windowcsd_batched(Y[0], Y[1], t, f, n, 0, Wd, _engine(lam), win_lo=lo, win_hi=hi)
        assert np.array_equal(xy, x[0]) and np.array_equal(xu, x[1])
        sre, sim, syy, suu = (np.zeros(len(f)) for _ in range(4))
        for k in range(len(ranges)):
            ar, ai, br, bi = xy[k].real, xy[k].imag, xu[k].real, xu[k].imag
            sre += ar * br + ai * bi
            sim += ai * br - ar * bi
            syy += ar * ar + ai * ai
            suu += br * br + bi * bi
        assert np.array_equal(Syu.real, sre) and np.array_equal(Syu.imag, sim) and np.array_equal(Syy, syy) and np.array_equal(Suu, suu)
        if sub is None and window == "hann0":                         # ls_cohere takes Hann windows itself
            c, _ = L.ls_cohere(Y[0], Y[1], t, f, nw=nwin, noverlap=0, λ=lam)
            assert np.all(np.isfinite(c)) and 0 <= c.min() and c.max() <= 1 + 1e-12, (c.min(), c.max())
            assert np.array_equal(c, (sre * sre + sim * sim) / (suu * syy))


# ---------------------------------------------------------------------------------------------------------------- lpvs_windowpsd_lpv_f64
def _windowpsd_lpv(Y, X, V, w, nwin, in_flight):
    from lpvspectral_jl_amd._lib import lib
    Y, X, V, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (Y, X, V, w))
    S, fva = np.zeros(len(w)), np.ones(nwin)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib().lpvs_windowpsd_lpv_f64(ptr(Y), ptr(X), ptr(V), len(Y), ptr(w), len(w), D.WPL_NV, D.WPL_N, 0, D.WPL_LAM, 1, 0, 0, in_flight, ptr(S), ptr(fva))
    return rc, lib().lpvs_last_error().decode(), S, fva


@pytest.fixture(scope="module")
def wpl_reference(L):
    """Per window count: (S_ref, its bound, fva per window) from the extended-precision solutions; computed once."""
    cache = {}

    def get(nwin):
        if nwin not in cache:
            Y, X, V, w = D.wpl_inputs(nwin)
            S, bound, fva = np.zeros(D.WPL_NF, dtype=D.LD), np.zeros(D.WPL_NF), []
            for k in range(nwin):
                sl = slice(k * D.WPL_N, (k + 1) * D.WPL_N)
                with L.Problem.lpv(Y[sl], X[sl], V[sl], w, D.WPL_NV) as p:
                    assert p.timing()["gram_form"] == "krs"
                Phi = L.lpv_regressor(X[sl], V[sl], w, D.WPL_NV, permuted=True)
                s, b, fv = D.wpl_window_reference(Phi, Y[sl], D.WPL_LAM)
                S, bound = S + s, bound + b
                fva.append(float(fv))
            cache[nwin] = (S, bound + (nwin + 1) * D.U * S.astype(np.float64), np.array(fva))
        return cache[nwin]
    yield get
    cache.clear()


@pytest.mark.parametrize("nwin,in_flight", D.WPL_CASES)
def test_windowpsd_lpv_sum_and_fva(L, wpl_reference, nwin, in_flight):
    Y, X, V, w = D.wpl_inputs(nwin)
    S_ref, bound, fva_ref = wpl_reference(nwin)
    rc, msg, S, fva = _windowpsd_lpv(Y, X, V, w, nwin, in_flight)
    assert rc == 0, msg
    rS = float(np.max(np.abs(S - S_ref).astype(np.float64) / bound))
    dfva = float(np.max(np.abs(fva - fva_ref)))
    print(f"{nwin} windows, in_flight {in_flight}: S at {rS:.3g} of its forward bound, fva within {dfva:.3g} (1e-8 promised)")
    assert rS <= 1.0 and dfva <= 1e-8
    if in_flight > 1:                                                 # the sum is taken in window order: in_flight changes no bit
        assert np.array_equal(S, _windowpsd_lpv(Y, X, V, w, nwin, 1)[2])


def test_windowpsd_lpv_constant_window_and_nan():
    Y, X, V, w = D.wpl_inputs(2)
    Yc = Y.copy()
    Yc[D.WPL_N:] = 0.75                                               # a constant second window: var(y) = 0
    rc, msg, S, fva = _windowpsd_lpv(Yc, X, V, w, 2, 2)
    assert rc == 0, msg
    assert fva[1] == -np.inf and np.isfinite(fva[0]) and np.all(np.isfinite(S))
    Vn = V.copy()
    Vn[D.WPL_N + 7] = np.nan
    rc, msg, _, _ = _windowpsd_lpv(Y, X, Vn, w, 2, 1)
    assert rc == -1, (rc, msg)                                       # LPVS_EARGUMENT
    assert "window 1" in msg and f"samples {D.WPL_N} .. {2 * D.WPL_N - 1}" in msg, msg
