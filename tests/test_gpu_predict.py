"""predict / residual / fva on the GPU (csrc/eval.hip) against the long-double reference of tests/_eval_ref.py, whose docstring derives
the direct path's per-sample bound (Nf nb + 16) 2^-53 S_m and names the type-2 path's tolerance struct_tol * S_m (tests/test_eval_ref_host.py
proves both on the CPU).  No sample is exempt and no maximum over the record is taken: every |got - ref| is divided by ITS bound.

    1  direct path on grids off any progression: Fourier (with / without the zero frequency), LPV (normalize on / off, coulomb)
    2  type-2 path: the structured cases' shapes, the 256 grid at its limit with default_freqs (a = 0, zero frequency), a != 0 (the rotation),
       samples planted where the taps wrap, planted residuals (the twin); and at |w x| = 3e6 and 2^30 rad against the phases of the real
       products, where the low words of nu_phase_turns decide (the direct path at 2^30 rad against its own reference)
    3  the path argument
    4  columns: a multi-column call equals the single-column calls bit for bit
    5  residual, sums, fva
    6  predicting off the record: the fitted basis, not a basis of the new V
    7  device tensors
    8  end to end: fva of a sparse and of a ridge estimate"""
import functools

import numpy as np
import pytest

import _eval_ref as E
import _gram_ref as R
import _phase_ref as PR

pytestmark = pytest.mark.gpu
LD = np.longdouble
U = 2.0 ** -53


def _coefs(rng, n, nc=1):
    return (rng.standard_normal((n, nc)) + 1j * rng.standard_normal((n, nc))) * 10.0 ** rng.integers(-2, 2, (n, 1))


def _plant(x, period):
    """Reduced phases 0, 1e-9, 2 pi - 1e-9 and pi (a few periods in): the 16 taps wrap round both ends of the fine grid."""
    x[:4] = [0.0, period * (1e-9 / (2 * np.pi)) + 3 * period, period * (1 - 1e-9 / (2 * np.pi)) + period, 0.5 * period + 2 * period]
    return x


def _se(L, Y, X, V, w, Nv, normalize, coulomb, x):
    return L.SpectralExt(Y, X, V, w, Nv, 1.0, coulomb, normalize, x, None)


def _worst(got, ref, bound):
    assert np.all(bound > 0)
    return float(np.max(np.abs(got.astype(LD) - ref) / bound))


# ---- the cases (inputs and references are computed once) ---------------------------------------------------------------------------------
M_DIRECT_LPV, M_NUFFT = 4099, 4096 + 3


@functools.lru_cache(maxsize=None)
def _lpv_direct(normalize, coulomb):
    """Nf = 24, Nv = 3 on a sorted random grid (no progression), M = 4099 (17 workgroups, the last one 3 samples), 2 coefficient columns."""
    from oracle import oracle
    rng = np.random.default_rng(31 + 2 * normalize + coulomb)
    Nf, Nv, M = 24, 3, M_DIRECT_LPV
    nb = 2 * Nv if coulomb else Nv
    X, V = rng.uniform(-3.0, 5.0, M), rng.uniform(-1.0, 1.0, M)
    w = np.sort(rng.uniform(0.4, 6.0, Nf))
    P = _coefs(rng, Nf * nb, 2)
    vc, gamma = oracle.basis_centers(V, Nv, coulomb)
    yh, S = E.evaluate_ld(P, w, X, E.activations_ld(V, vc, gamma, normalize, coulomb))
    return dict(Nf=Nf, Nv=Nv, nb=nb, M=M, X=X, V=V, w=w, P=P, yh=yh, S=S, Y=rng.standard_normal(M))


@functools.lru_cache(maxsize=None)
def _fourier_direct(zero):
    rng = np.random.default_rng(41 + zero)
    Nf, M = 40, 1000
    t = np.cumsum(0.5 + rng.random(M))
    f = np.sort(rng.uniform(0.01, 0.45, Nf))
    if zero:
        f[0] = 0.0
    p = _coefs(rng, Nf)[:, 0]
    if zero:
        p[0] = p[0].real
    yh, S = E.evaluate_ld(p, E.fourier_w(f), t, None, E.fourier_scale_ld(Nf))
    return dict(Nf=Nf, M=M, t=t, f=f, p=p, yh=yh[:, 0], S=S[:, 0], y=rng.standard_normal(M))


NUFFT_LPV = {                       # id: (Nf, Nv, first multiple of the step, planted residual phase emax * max|x|)
    "ap-24x3": (24, 3, 1, 0.0),     # tests/_gram_ref.py: STRUCT_LPV_CASES' shapes and grid w = D (1 .. Nf): a != 0, the rotation
    "ap-20x8": (20, 8, 1, 0.0),
    "ap-65x2-limit": (65, 2, 1, 0.0),        # 3.9 * 65 = 253.5: the 256 grid filled to its limit
    "ap-24x3-from-0": (24, 3, 0, 0.0),       # a = 0 and a zero frequency
    "ap-24x3-residuals": (24, 3, 1, 5e-8),   # admitted (< 1e-7); without the first-order twin this misses by four orders of magnitude
}


@functools.lru_cache(maxsize=None)
def _lpv_nufft(cid):
    from oracle import oracle
    Nf, Nv, start, resid = NUFFT_LPV[cid]
    rng = np.random.default_rng(900 + Nf + Nv + start)
    M, D = M_NUFFT, 2 * np.pi / 7.0
    X = _plant(rng.permutation(np.sort(rng.random(M)) * 50.0), 7.0)
    V = rng.uniform(-1.0, 1.0, M)
    w = D * np.arange(start, start + Nf)
    if resid:
        eps = rng.uniform(-1.0, 1.0, Nf)
        eps[0] = eps[-1] = 0.0
        w = w + eps * (resid / (np.abs(eps).max() * np.abs(X).max()))
    P = _coefs(rng, Nf * Nv, 2)
    vc, gamma = oracle.basis_centers(V, Nv, False)
    yh, S = E.evaluate_ld(P, w, X, E.activations_ld(V, vc, gamma, True, False))
    return dict(Nf=Nf, Nv=Nv, M=M, X=X, V=V, w=w, P=P, yh=yh, S=S, tol=E.struct_tol(np.abs(w).max(), np.abs(X).max()), Y=rng.standard_normal(M))


@functools.lru_cache(maxsize=None)
def _fourier_nufft(kind):
    """'ap-fourier' / 'ap-fourier-zero': STRUCT_FOURIER_CASES' grids k / 97 (Nf = 40); 'default-freqs': default_freqs of the first 128
    stamps -- (0 .. 64) fs / 128, a = 0, a zero frequency, 65 modes on the 256 grid."""
    import lpvspectral_jl_amd as L
    rng = np.random.default_rng(17 + len(kind))
    M = M_NUFFT
    t = np.sort(rng.random(M) * 300.0)
    if kind == "default-freqs":
        f = L.default_freqs(t, n=128)
        assert len(f) == 65 and f[0] == 0.0
    else:
        f = (np.arange(40) if kind == "ap-fourier-zero" else np.arange(1, 41)) / 97.0
    step = f[1] - f[0]
    t = np.sort(_plant(t, 1.0 / step))
    Nf = len(f)
    p = _coefs(rng, Nf)[:, 0]
    yh, S = E.evaluate_ld(p, E.fourier_w(f), t, None, E.fourier_scale_ld(Nf))
    return dict(Nf=Nf, M=M, t=t, f=f, p=p, yh=yh[:, 0], S=S[:, 0], tol=E.struct_tol(np.abs(E.fourier_w(f)).max(), np.abs(t).max()))


# ---- 1  direct path ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero", [False, True])
def test_direct_fourier(L, zero):
    c = _fourier_direct(zero)
    got = L.predict(c["p"], c["f"], c["t"])
    tm = L.eval_last_timing()
    assert tm["path"] == "direct" and tm["nf"] == 0 and got.shape == (c["M"],)
    bound = E.direct_bound(c["Nf"], 1, c["S"])
    r_ref = _worst(got, c["yh"], bound)
    A, zf = L.get_fourier_regressor(c["t"], c["f"])
    r_reg = _worst(got, A.astype(LD) @ E.fourier_real_vector(c["p"], zf).astype(LD), bound)
    print(f"fourier zero={zero}: worst |got - ref| / bound = {r_ref:.4f}; against the device regressor's product {r_reg:.4f}")
    assert r_ref <= 1.0 and r_reg <= 1.0
    x_real = E.fourier_real_vector(c["p"], zf)                       # the real vector the regressor multiplies is accepted too
    assert np.array_equal(L.predict(x_real, c["f"], c["t"]), got)


@pytest.mark.parametrize("normalize,coulomb", [(True, False), (False, False), (True, True)])
def test_direct_lpv(L, normalize, coulomb):
    c = _lpv_direct(normalize, coulomb)
    se = _se(L, c["Y"], c["X"], c["V"], c["w"], c["Nv"], normalize, coulomb, c["P"])
    got = L.predict(se)                                               # auto: M >= the threshold, but the grid is no progression
    tm = L.eval_last_timing()
    assert tm["path"] == "direct" and tm["slabs"] == 17 and got.shape == (c["M"], 2)
    bound = E.direct_bound(c["Nf"], c["nb"], c["S"])
    r_ref = _worst(got, c["yh"], bound)
    Phi = L.lpv_regressor(c["X"], c["V"], c["w"], c["Nv"], normalize, coulomb, permuted=False)
    r_reg = _worst(got, Phi.astype(LD) @ E.stack_re_im(c["P"]).astype(LD), bound)
    print(f"lpv normalize={normalize} coulomb={coulomb}: worst |got - ref| / bound = {r_ref:.4f}; against the device regressor's product {r_reg:.4f}")
    assert r_ref <= 1.0 and r_reg <= 1.0


# ---- 2  type-2 path ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(NUFFT_LPV))
def test_nufft_lpv(L, cid):
    c = _lpv_nufft(cid)
    se = _se(L, c["Y"], c["X"], c["V"], c["w"], c["Nv"], True, False, c["P"])
    got = L.predict(se)                                               # auto: a progression and M >= the plan's threshold
    tm = L.eval_last_timing()
    assert tm["path"] == "nufft" and tm["nf"] == 256
    if NUFFT_LPV[cid][3]:
        assert tm["twin"]
    r = _worst(got, c["yh"], c["tol"] * c["S"])
    rd = _worst(L.predict(se, path="direct"), c["yh"], E.direct_bound(c["Nf"], c["Nv"], c["S"]))
    print(f"{cid}: twin={tm['twin']} worst |got - ref| / (struct_tol S_m) = {r:.4f}; the direct path against its own bound {rd:.4f}")
    assert r <= 1.0 and rd <= 1.0


@pytest.mark.parametrize("kind", ["ap-fourier", "ap-fourier-zero", "default-freqs"])
def test_nufft_fourier(L, kind):
    c = _fourier_nufft(kind)
    got = L.predict(c["p"], c["f"], c["t"])
    tm = L.eval_last_timing()
    assert tm["path"] == "nufft" and tm["nf"] == 256
    r = _worst(got, c["yh"], c["tol"] * c["S"])
    print(f"{kind}: twin={tm['twin']} worst |got - ref| / (struct_tol S_m) = {r:.4f}")
    assert r <= 1.0


# ---- 2b  type-2 path where the low words of its phases decide -------------------------------------------------------------------------------
# The cases above keep |w x| <= 1.1e3 rad and carry struct_tol's term 4.5e-16 max|w| max|x|.  Here |w x| reaches 3e6 rad (natural rounding
# residuals of the grid; planted ones at the admission limit) and 2^30 rad (a dyadic grid), the reference forms the phases of the real products
# (tests/_phase_ref.py: evaluate_exact) and the bound is (1e-12 + q) S_m per sample: 1e-12 the stated tolerance of the transform, q <= 1e-13
# the squares the kernel headers drop (_phase_ref.second_order).  Nothing grows with |w||x|.  The inputs are built like the structured Gram's
# (tests/_gram_ref.py: PHASE_PREDICT_CASES, which says why the grids start at a = 2.5 D).
@functools.lru_cache(maxsize=None)
def _lpv_large_phase(cid):
    from oracle import oracle
    case = R.PHASE_LPV[cid]
    Nf, Nv = case[1], case[2]
    Y, X, V, w = R.phase_lpv_inputs(case)
    P = _coefs(np.random.default_rng(len(cid)), Nf * Nv, 2)
    vc, gamma = oracle.basis_centers(V, Nv, False)
    K = E.activations_ld(V, vc, gamma, True, False)
    q = PR.second_order(w, X)
    assert q <= 1e-13
    yh, S = PR.evaluate_exact(P, w, X, K)
    return dict(Nf=Nf, Nv=Nv, M=len(X), X=X, V=V, w=w, P=P, K=K, Y=Y, yh=yh, S=S, tol=1e-12 + q)


@pytest.mark.parametrize("cid", [c[0] for c in R.PHASE_PREDICT_CASES])
def test_nufft_lpv_against_exact_phases(L, cid):
    """eval_grid_kernel, eval_interp_kernel (nu_phase_turns of D x) and the rotation e^{i a x} (nu_phase_turns of a x) at |w x| = 3e6 rad
    and 2^30 rad."""
    c = _lpv_large_phase(cid)
    se = _se(L, c["Y"], c["X"], c["V"], c["w"], c["Nv"], True, False, c["P"])
    got = L.predict(se)
    tm = L.eval_last_timing()
    assert tm["path"] == "nufft" and tm["nf"] == 256 and tm["twin"] == (cid != "predict-24x3-beyond")
    r = _worst(got, c["yh"], c["tol"] * c["S"])
    print(f"{cid}: max|w x| = {np.abs(c['w']).max() * np.abs(c['X']).max():.3g} rad, twin={tm['twin']}, worst |got - ref| / ((1e-12 + q) S_m) = {r:.4f}")
    assert r <= 1.0


def test_direct_lpv_at_two_to_the_thirty_radians(L):
    """The direct path rounds the phase as the reference implementation does and keeps its rounded-phase reference and its bound: the
    device's sincos at arguments up to 2^30."""
    c = _lpv_large_phase("predict-24x3-beyond")
    se = _se(L, c["Y"], c["X"], c["V"], c["w"], c["Nv"], True, False, c["P"])
    got = L.predict(se, path="direct")
    assert L.eval_last_timing()["path"] == "direct"
    yh, S = E.evaluate_ld(c["P"], c["w"], c["X"], c["K"])
    r = _worst(got, yh, E.direct_bound(c["Nf"], c["Nv"], S))
    print(f"direct at 2^30 rad: worst |got - ref| / bound = {r:.4f}")
    assert r <= 1.0


# ---- 3  the path argument ----------------------------------------------------------------------------------------------------------------
def test_path_argument(L):
    c = _lpv_direct(True, False)
    se = _se(L, c["Y"], c["X"], c["V"], c["w"], c["Nv"], True, False, c["P"][:, 0])
    with pytest.raises(ValueError, match="arithmetic progression"):
        L.predict(se, path="nufft")
    with pytest.raises(ValueError):
        L.predict(se, path="fft")
    L.predict(se, path="auto")
    assert L.eval_last_timing()["path"] == "direct"
    c = _lpv_nufft("ap-24x3")
    se = _se(L, c["Y"], c["X"], c["V"], c["w"], c["Nv"], True, False, c["P"][:, 0])
    L.predict(se)
    assert L.eval_last_timing()["path"] == "nufft"
    L.predict(se, X=c["X"][:4095], V=c["V"][:4095])                   # one sample below the plan's threshold
    assert L.eval_last_timing()["path"] == "direct"
    L.predict(se, X=c["X"][:100], V=c["V"][:100], path="nufft")       # asked for: no threshold
    assert L.eval_last_timing()["path"] == "nufft"
    from lpvspectral_jl_amd._lib import lib, out_ptr, LPVS_EARGUMENT
    one = np.ones(8)
    assert lib().lpvs_fourier_eval_f64(out_ptr(one), out_ptr(one), 1, out_ptr(one), 8, out_ptr(one), None, 8, 3, 0, out_ptr(one), None) == LPVS_EARGUMENT


# ---- 4  columns --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["direct", "nufft"])
def test_a_column_of_a_path_equals_its_own_call_bit_for_bit(L, path):
    c = _lpv_nufft("ap-24x3")
    rng = np.random.default_rng(5)
    P3 = _coefs(rng, c["Nf"] * c["Nv"], 3)
    mk = lambda x: _se(L, c["Y"], c["X"], c["V"], c["w"], c["Nv"], True, False, x)   # noqa: E731
    all3 = L.predict(mk(P3), path=path)
    assert all3.shape == (c["M"], 3) and L.eval_last_timing()["path"] == path
    for q in range(3):
        one = L.predict(mk(P3[:, q]), path=path)
        assert one.shape == (c["M"],) and np.array_equal(one, all3[:, q]), q
    nine = L.predict(mk(np.concatenate([P3, P3, P3], axis=1)), path=path)             # 9 columns: two column blocks of the direct path
    assert np.array_equal(nine[:, :3], all3) and np.array_equal(nine[:, 6:], all3)


# ---- 5  residual, sums, fva --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["direct", "nufft"])
def test_residual_sums_and_fva(L, path):
    c = _lpv_nufft("ap-24x3")
    M = c["M"]
    y = (c["yh"][:, 0] + 0.3 * c["Y"].astype(LD)).astype(np.float64)                  # a signal the first column explains well
    se = _se(L, y, c["X"], c["V"], c["w"], c["Nv"], True, False, c["P"])
    yhat = L.predict(se, path=path)
    e, sums = L.residual(se, path=path, return_sums=True)
    assert np.array_equal(e, y[:, None] - yhat)                                       # bit for bit
    e2, sums2 = L.residual(se, path=path, return_sums=True)
    assert np.array_equal(e, e2) and np.array_equal(sums, sums2)                      # no atomics: the same bits
    el = e.astype(LD)
    for q in range(2):
        s1, s2 = el[:, q].sum(), (el[:, q] * el[:, q]).sum()
        assert abs(LD(sums[q, 0]) - s1) <= (M + 16) * U * np.abs(el[:, q]).sum(), q
        assert abs(LD(sums[q, 1]) - s2) <= (M + 16) * U * s2, q
    # fva: the per-sample bound delta moves var(e) by at most (2 mean|e| delta + delta^2) M / (M - 1); the sums' own rounding
    # ((M + 16) u of sum|e| resp. sum e^2: 3 (M + 16) u sum e^2 in var(e), since (sum|e|)^2 <= M sum e^2) and four roundings of the final
    # arithmetic are added; nothing else
    per_sample = E.direct_bound(c["Nf"], c["Nv"], c["S"]) if path == "direct" else c["tol"] * c["S"]
    got = L.fva(se, path=path)
    assert got.shape == (2,)
    var_y = np.var(y.astype(LD), ddof=1)
    for q in range(2):
        eref = y.astype(LD) - c["yh"][:, q]
        delta = per_sample[:, q].max() + U * np.abs(eref).max()                       # + the rounding of y - yhat
        dvar = (2 * np.abs(eref).mean() * delta + delta * delta) * M / (M - 1)
        dsum = ((M + 16) * U * (eref * eref).sum() * (1 + 2) + 4 * U * (eref * eref).sum()) / (M - 1)   # sum e^2, (sum e)^2 / M <= sum e^2
        ref = 1 - np.var(eref, ddof=1) / var_y
        bound = (dvar + dsum) / var_y + (M + 16) * U * abs(1 - ref)                   # + var(y)'s own float64 summation and the quotient
        print(f"{path} column {q}: fva = {got[q]:.6f}, |got - ref| = {float(abs(got[q] - ref)):.3e}, bound = {float(bound):.3e}")
        assert abs(LD(got[q]) - ref) <= bound, q
    assert got[0] > 0.5                                                               # the first column does explain the signal
    assert L.fva(_se(L, y, c["X"], c["V"], c["w"], c["Nv"], True, False, c["P"][:, 0]), path=path) == got[0]


def test_fourier_residual_and_fva(L):
    c = _fourier_direct(True)
    e, sums = L.residual(c["p"], c["f"], c["t"], c["y"], return_sums=True)
    assert np.array_equal(e, c["y"] - L.predict(c["p"], c["f"], c["t"]))
    M = c["M"]
    want = 1 - ((sums[0, 1] - sums[0, 0] ** 2 / M) / (M - 1)) / np.var(c["y"], ddof=1)
    assert L.fva(c["p"], c["f"], c["t"], c["y"]) == want


# ---- 6  off the record -------------------------------------------------------------------------------------------------------------------
def test_new_samples_meet_the_fitted_basis(L, oracle):
    c = _lpv_direct(True, False)
    rng = np.random.default_rng(77)
    Mn = 777
    Xn = rng.uniform(-2.0, 4.0, Mn)
    Vn = rng.uniform(-0.5, 0.6, Mn)                                                   # strictly inside the training range
    se = _se(L, c["Y"], c["X"], c["V"], c["w"], c["Nv"], True, False, c["P"])
    got = L.predict(se, X=Xn, V=Vn)
    assert got.shape == (Mn, 2)
    vc, gamma = oracle.basis_centers(c["V"], c["Nv"], False)                          # the TRAINING record's centres
    yh, S = E.evaluate_ld(c["P"], c["w"], Xn, E.activations_ld(Vn, vc, gamma, True, False))
    r = _worst(got, yh, E.direct_bound(c["Nf"], c["nb"], S))
    vc2, gamma2 = oracle.basis_centers(Vn, c["Nv"], False)                            # a basis rebuilt on the new V is another model
    yh2, _ = E.evaluate_ld(c["P"], c["w"], Xn, E.activations_ld(Vn, vc2, gamma2, True, False))
    r2 = _worst(got, yh2, E.direct_bound(c["Nf"], c["nb"], S))
    print(f"worst |got - ref| / bound: fitted basis {r:.4f}, basis of the new V {r2:.3e}")
    assert r <= 1.0 and r2 > 1e6


# ---- 7  device tensors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["direct", "nufft"])
def test_device_tensors_give_the_same_bits(L, path):
    import torch
    c = _lpv_nufft("ap-24x3")
    se = _se(L, c["Y"], c["X"], c["V"], c["w"], c["Nv"], True, False, c["P"])
    e_host, s_host = L.residual(se, path=path, return_sums=True)
    dev = lambda a: torch.tensor(a, dtype=torch.float64, device="cuda")               # noqa: E731
    sed = _se(L, dev(c["Y"]), dev(c["X"]), dev(c["V"]), c["w"], c["Nv"], True, False, c["P"])
    out = torch.zeros(2 * c["M"], dtype=torch.float64, device="cuda")
    e_dev, s_dev = L.residual(sed, path=path, out=out, return_sums=True)
    assert e_dev is out
    assert np.array_equal(out.cpu().numpy().reshape(2, c["M"]).T, e_host) and np.array_equal(s_dev, s_host)
    x32 = c["X"].astype(np.float32)                                                   # float32 inputs are widened
    assert np.array_equal(L.predict(se, X=x32, V=c["V"], path=path), L.predict(se, X=x32.astype(np.float64), V=c["V"], path=path))


# ---- 8  end to end -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_problem():
    rng = np.random.default_rng(3)
    N, Nf, Nv = 600, 10, 3
    X = np.sort(rng.random(N)) * 20.0
    V = np.linspace(-1.0, 1.0, N)
    w = 2 * np.pi * np.arange(1, Nf + 1) / 10.0
    Y = (1 + V) * np.sin(w[2] * X) + (1 - V) * np.cos(w[5] * X) + 0.05 * rng.standard_normal(N)
    return Y, X, V, w, Nv


def test_fva_of_a_sparse_estimate(L):
    Y, X, V, w, Nv = _small_problem()
    import warnings
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        se = L.ls_sparse_spectral_lpv(Y, X, V, w, Nv, λ=0.02, iters=40, printerval=10 ** 6)
    assert se.Σ is None and not [m for m in seen if "variance" in str(m.message)]    # it returns what it returned and warns of nothing new
    v = L.fva(se)
    print(f"sparse estimate after 40 iterations: fva = {v:.4f}")
    assert np.isfinite(v) and v <= 1.0


def test_fva_of_a_ridge_estimate_is_the_regressors(L):
    Y, X, V, w, Nv = _small_problem()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        se = L.ls_spectral_lpv(Y, X, V, w, Nv, λ=1e-4)
    got = L.fva(se, path="direct")
    assert L.eval_last_timing()["path"] == "direct"
    Phi = L.lpv_regressor(X, V, w, Nv, True, False, permuted=False).astype(LD)
    coef = E.stack_re_im(np.asarray(se.x)).astype(LD)
    K = L.basis_activation_func(V, Nv, True, False).astype(LD)
    S = K @ np.abs(np.asarray(se.x)).reshape(Nv, len(w)).sum(axis=1).astype(LD)      # S_m = sum_j K_j sum_f |p_fj|
    eref = Y.astype(LD) - Phi @ coef
    N = len(Y)
    delta = E.direct_bound(len(w), Nv, S).max() + U * np.abs(eref).max()
    dvar = (2 * np.abs(eref).mean() * delta + delta * delta) * N / (N - 1)
    dsum = ((N + 16) * U * (eref * eref).sum() * 3 + 4 * U * (eref * eref).sum()) / (N - 1)
    var_y = np.var(Y.astype(LD), ddof=1)
    ref = 1 - np.var(eref, ddof=1) / var_y
    bound = (dvar + dsum) / var_y + (N + 16) * U * abs(1 - ref)                       # + var(Y)'s own float64 summation and the quotient
    print(f"ridge estimate: fva = {got:.6f}, |got - ref| = {float(abs(got - ref)):.3e}, bound = {float(bound):.3e}")
    assert abs(LD(got) - ref) <= bound
    assert got > 0.9
