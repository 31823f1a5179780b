"""ComplexNormal on the device (csrc/cnormal.hip): the blocked Cholesky against its backward-error bound, the sampler against a
long-double product, the counter-based normals against the pure-Python restatement, the reference's statistical test
(test/runtests.jl:154-162), and the Monte-Carlo bands of the SpectralExt recipe against the numpy restatement (tests/_cnormal_ref.py)
on the reference's LPV test problem (test/runtests.jl:89-104)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cnormal_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

u = 2.0 ** -53
# largest |device normal - long-double restatement| over 10^7 elements, in units of u * r (r = sqrt(-2 ln u1), the draw's radius), as
# measured on an MI355X by tools/cnormal_time.py --normals; the tolerance is twice that (one more bit)
NORMALS_MEASURED_MAX = 2.788
NORMALS_TOL = 2 * NORMALS_MEASURED_MAX


def _bits(z):
    return np.ascontiguousarray(z).view(np.float64)


def gamma(k):
    return k * u / (1 - k * u)


def _spd(rng, n):
    A = rng.standard_normal((n, n))
    return A.T @ A / n + np.eye(n)


W_TEST = 2 * np.pi * np.arange(2, 25, 2.0)          # test/runtests.jl:95  2π*collect(2:2:25)
W_TRUE = 2 * np.pi * np.array([2.0, 10.0, 20.0])    # :94


@functools.lru_cache(maxsize=None)
def _problem(Nv, coulomb=False, Nf100=False):
    """The LPV test problem (test/runtests.jl:89-104) and its ridge estimate with covariance."""
    import lpvspectral_jl_amd as L
    Y, V, X, _, _ = R.generate_signal(R.F_TRUE, W_TRUE, 500, True, seed=0)
    if coulomb:
        V = V - 0.5                                 # a scheduling variable that changes sign
    w = 2 * np.pi * np.linspace(1, 25, 100) if Nf100 else W_TEST
    se = L.ls_spectral_lpv(Y, X, V, w, Nv, λ=0.02, normalize=True, coulomb=coulomb)
    return se


def _check_factor(V, U):
    n2 = V.shape[0]
    assert np.array_equal(np.tril(U, -1), np.zeros_like(U)), "lower triangle is not exactly zero"
    assert (np.diag(U) > 0).all()
    g = gamma(n2 + 1)
    Vs = np.triu(V) + np.triu(V, 1).T
    if n2 <= 200:
        Ul = U.astype(np.longdouble)
        res = np.abs(Ul.T @ Ul - Vs)
        bound = g * (np.abs(Ul).T @ np.abs(Ul))
    else:                                           # a long-double product of the whole matrix takes minutes: the diagonal and 20000 random entries
        rng = np.random.default_rng(n2)
        I = np.concatenate([np.arange(n2), rng.integers(0, n2, 20000)])
        J = np.concatenate([np.arange(n2), rng.integers(0, n2, 20000)])
        res, bound = np.empty(len(I), np.longdouble), np.empty(len(I), np.longdouble)
        for a in range(0, len(I), 2000):
            ui, uj = U[:, I[a:a + 2000]].astype(np.longdouble), U[:, J[a:a + 2000]].astype(np.longdouble)
            res[a:a + 2000] = np.abs((ui * uj).sum(axis=0) - Vs[I[a:a + 2000], J[a:a + 2000]])
            bound[a:a + 2000] = g * (np.abs(ui) * np.abs(uj)).sum(axis=0)
    ratio = float((res / bound).max())
    print(f"cholesky n2={n2}: max |U'U - V| / (gamma |U'||U|) = {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("n2", [6, 130, 1200, 2048])
def test_cholesky_random_spd(L, n2):
    V = _spd(np.random.default_rng(n2), n2)
    V = np.triu(V) + np.tril(np.full((n2, n2), np.nan), -1)      # only the upper triangle may be read
    _check_factor(V, L.cholesky_upper(V))


def test_cholesky_of_an_lpv_covariance(L):
    se = _problem(8)
    _check_factor(np.asarray(se.Σ), L.cholesky_upper(se.Σ))
    import torch
    Ud = L.cholesky_upper(torch.from_numpy(np.ascontiguousarray(np.asarray(se.Σ).T)).cuda())   # a device matrix: row-major Σ' is column-major Σ
    assert np.array_equal(Ud, L.cholesky_upper(se.Σ))


def test_cholesky_indefinite_input(L):
    from lpvspectral_jl_amd._lib import lib, LPVS_ENUMERIC, last_error
    rng = np.random.default_rng(5)
    for n2, bad in ((6, 3), (300, 217)):
        V = np.asfortranarray(_spd(rng, n2))
        V[bad, bad] = -1.0
        out = np.full((n2, n2), 7.0, order="F")
        rc = lib().lpvs_cholesky_upper_f64(C.c_void_p(V.ctypes.data), n2, 0, C.c_void_p(out.ctypes.data))
        assert rc == LPVS_ENUMERIC and f"pivot {bad} " in last_error(), last_error()
        assert (out == 7.0).all(), "outputs were written"
        with pytest.raises(L.NumericError):
            L.cholesky_upper(V)
    cn = L.ComplexNormal(np.zeros(3) + 0j, np.diag([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]))
    with pytest.raises(L.NumericError):
        L.rand(cn, 10)


@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("Nv", [8, 50])
def test_sampling_with_injected_normals(L, Nv, with_mean):
    """Z against m + R U_dev in long double.  The bound on the product is gamma_2n (|R||U|), componentwise, and it is asserted as it
    stands for the distribution with zero mean.  With the mean of the LPV estimate the result m + (R U) is rounded once more to a
    double, an error of up to u |Z| that NO double-precision output can avoid and that the product's bound does not contain: where
    |m| exceeds 2 (2n) |R||U| -- coefficients whose standard deviation is below 1/400 of their value -- the plain bound is out of
    reach of any implementation (measured on an MI355X: 1.62 of it at 2n = 192 and 0.52 at 2n = 1200; with u |Z| added to the bound
    0.43 and 0.15; the zero-mean cases sit at 0.026 and 0.007 of the plain bound).  That case asserts gamma_2n (|R||U|) + u |Z|."""
    import torch
    se = _problem(Nv)
    n2 = se.Σ.shape[0]
    s = 333
    Rn = np.random.default_rng(Nv).standard_normal((s, n2))
    mean = np.asarray(se.x) if with_mean else np.zeros(n2 // 2, dtype=np.complex128)
    cn = L.ComplexNormal(mean, se.Σ)
    Z = L.rand(cn, s, normals=Rn)
    assert Z.shape == (s, n2 // 2) and Z.dtype == np.complex128
    U = L.cholesky_upper(se.Σ)
    zr, zi = R.rand_given(mean, U, Rn, dtype=np.longdouble)
    ref = np.concatenate([zr, zi], axis=1)
    got = np.concatenate([Z.real, Z.imag], axis=1)
    bound = gamma(n2) * (np.abs(Rn).astype(np.longdouble) @ np.abs(U).astype(np.longdouble))
    err = np.abs(got - ref)
    print(f"sampling 2n={n2} mean={with_mean}: max |dZ| / (gamma_2n |R||U|) = {float((err / bound).max()):.4f}, "
          f"with the output's rounding u|Z| added to the bound {float((err / (bound + u * np.abs(ref))).max()):.4f}")
    if with_mean:
        bound = bound + u * np.abs(ref)
    assert float((err / bound).max()) <= 1.0
    assert np.array_equal(_bits(L.rand(cn, s, normals=Rn)), _bits(Z))
    Zd = L.rand(cn, s, normals=torch.from_numpy(Rn).cuda())
    assert np.array_equal(_bits(Zd), _bits(Z))


def test_device_normals_against_the_restatement(L):
    seed = 20240229
    rows, cols = 4000, 63
    got = L.randn(rows, cols, seed=seed)
    ref, rad = R.randn(seed, 0, rows, cols, dtype=np.longdouble)
    err = np.abs(got - ref) / (u * rad)
    print(f"normals: max error {float(err.max()):.3f} u*r over {rows * cols} elements (tolerance {NORMALS_TOL})")
    assert float(err.max()) <= NORMALS_TOL
    assert abs(got.mean()) < 0.01 and abs(got.std() - 1) < 0.01
    a, b = 1234, 1777
    assert np.array_equal(L.randn(b - a, cols, seed=seed, row0=a), got[a:b])
    assert not np.array_equal(L.randn(8, cols, seed=seed + 1), got[:8])
    big = 2 ** 33 + 5                                             # the high counter word
    gb = L.randn(3, 4, seed=seed, row0=big)
    rb, radb = R.randn(seed, big, 3, 4, dtype=np.longdouble)
    assert float((np.abs(gb - rb) / (u * radb)).max()) <= NORMALS_TOL
    cn = L.ComplexNormal(np.arange(3) + 1j, _spd(np.random.default_rng(0), 6))
    z2 = L.rand(cn, 700, seed=9)
    assert np.array_equal(_bits(L.rand(cn, 130, seed=9)), _bits(z2[:130]))
    assert np.array_equal(_bits(L.rand(cn, 700, normals=L.randn(700, 6, seed=9))), _bits(z2))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_reference_statistical_test(L, seed):
    """test/runtests.jl:154-162, its sizes and its tolerance."""
    rng = np.random.default_rng(100)
    x, y = rng.standard_normal((1000, 3)), rng.standard_normal((1000, 3))
    cn = L.ComplexNormal(x, y)
    z = L.rand(cn, 1_000_000, seed=seed)
    cn2 = L.ComplexNormal(z)
    dG, dC = np.linalg.norm(cn.Γ - cn2.Γ), np.linalg.norm(cn.C - cn2.C)
    print(f"seed {seed}: |Γ - Γ2| = {dG:.5f}, |C - C2| = {dC:.5f}")
    assert dG < 0.01 and dC < 0.01
    m, G, Cc, _ = R.from_samples(z.real[:50000], z.imag[:50000])         # the device covariance against numpy's on a slice
    c3 = L.ComplexNormal(z[:50000])
    assert np.allclose(c3.m, m, rtol=0, atol=1e-13) and np.allclose(c3.Γ, G, rtol=0, atol=1e-12) and np.allclose(c3.C, Cc, rtol=0, atol=1e-12)


def test_grid_basis_is_the_references_K(L):
    """The activation kernel evaluated ON THE GRID places the centres of K = basis_activation_func(se.V, ...): the grid has V's extremes."""
    for coulomb, V in ((False, np.linspace(0, 1, 500)), (True, np.linspace(-0.5, 0.5, 500)), (True, np.linspace(-0.2, 0.7, 321))):
        for normalize in (True, False):
            vg = R.linrange(V.min(), V.max(), 100)
            assert vg.min() == V.min() and vg.max() == V.max()
            got = L.basis_activation_func(vg, 8, normalize, coulomb)
            want = R.basis_activation(V, 8, normalize, coulomb)(vg)
            assert np.allclose(got, want, rtol=1e-11, atol=1e-300), (coulomb, normalize, np.abs(got - want).max())


BAND_CASES = [
    dict(Nv=8, nMC=5000), dict(Nv=50, nMC=5000), dict(Nv=8, nMC=5000, coulomb=True), dict(Nv=2, nMC=1000, Nf100=True),
    dict(Nv=8, nMC=10), dict(Nv=8, nMC=16384),
]


@pytest.mark.parametrize("case", BAND_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_bands_with_injected_normals(L, case):
    se = _problem(case["Nv"], case.get("coulomb", False), case.get("Nf100", False))
    nMC = case["nMC"]
    Nf = len(se.w)
    n2 = se.Σ.shape[0]
    nb = n2 // 2 // Nf
    Rn = np.random.default_rng(nMC + n2).standard_normal((nMC, n2))
    sf = L.schedfunc(se, nMC=nMC, phase=True, normals=Rn)
    U = L.cholesky_upper(se.Σ)
    ref = R.schedfunc(se.x, se.Σ, se.V, se.w, se.Nv, se.normalize, se.coulomb, R=Rn, U=U, nMC=nMC, phase=True)
    G = 101 if Nf == 100 else 100
    assert sf.F.shape == (Nf, G) and sf.FBl.shape == (Nf, G) and sf.PBm.shape == (Nf, G) and len(sf.v) == G
    assert np.array_equal(sf.v, ref["vg"])
    tau = 4 * (nb + 2) * u * ref["absdot"]
    xa = np.abs(np.reshape(se.x, (Nf, -1), order="F")) @ np.abs(ref["K"]).T
    tauF = 4 * (nb + 2) * u * xa
    for name, got, want, tol in (("F", sf.F, ref["F"], tauF), ("FBl", sf.FBl, ref["FBl"], tau), ("FBu", sf.FBu, ref["FBu"], tau),
                                 ("FBm", sf.FBm, ref["FBm"], tau + nMC * u * ref["FBm"])):
        ratio = float((np.abs(got - want) / tol).max())
        print(f"{name}: max error / tolerance = {ratio:.4f}")
        assert ratio <= 1.0, name
    skip = (ref["dmin"] < 1e-9 * np.abs(se.x).max()) | ref["near_cut"]
    print(f"phase: {int(skip.sum())} of {skip.size} cells left out")
    assert skip.mean() <= 0.01
    keep = ~skip
    tolP = tau / ref["dmin"]
    tolP0 = tauF / np.abs(np.conj(np.reshape(se.x, (Nf, -1), order="F")) @ ref["K"].T)
    for name, got, want, tol in (("P", sf.P, ref["P"], tolP0), ("PBl", sf.PBl, ref["PBl"], tolP), ("PBu", sf.PBu, ref["PBu"], tolP),
                                 ("PBm", sf.PBm, ref["PBm"], tolP)):
        ratio = float((np.abs(got - want)[keep] / tol[keep]).max())
        print(f"{name}: max error / tolerance = {ratio:.4f}")
        assert ratio <= 1.0, name


def test_bands_from_the_device_generator(L):
    se = _problem(8)
    Nf, n2, nMC = len(se.w), se.Σ.shape[0], 5000
    a = L.schedfunc(se, seed=11)
    b = L.schedfunc(se, seed=11)
    Rn = L.randn(nMC, n2, seed=11)
    c = L.schedfunc(se, normals=Rn)
    for name in ("F", "FBl", "FBu", "FBm"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
        assert np.array_equal(getattr(a, name), getattr(c, name)), name
    assert not np.array_equal(a.FBl, L.schedfunc(se, seed=12).FBl)
    assert (a.PBl == 0).all() and (a.PBu == 0).all() and (a.PBm == 0).all()     # phase=False: left zero, as in the reference
    wide = a.FBl < a.FBu
    assert wide.any() and (a.FBl[wide] <= a.FBm[wide]).all() and (a.FBm[wide] <= a.FBu[wide]).all()
    # coverage of the noise-free dependence at the three true frequencies, against the restatement on the same normals
    ref = R.schedfunc(se.x, se.Σ, se.V, se.w, se.Nv, se.normalize, se.coulomb, R=Rn, U=L.cholesky_upper(se.Σ), nMC=nMC)
    for k, j in enumerate((0, 4, 9)):                                           # 2π·[2, 10, 20] within 2π·(2:2:24)
        truth = np.abs(R.F_TRUE[k](a.v))
        mine = int(((a.FBl[j] <= truth) & (truth <= a.FBu[j])).sum())
        theirs = int(((ref["FBl"][j] <= truth) & (truth <= ref["FBu"][j])).sum())
        print(f"true frequency {k}: {mine} of {len(truth)} grid points covered, restatement {theirs}")
        assert abs(mine - theirs) <= 1


def test_schedfunc_plumbing(L):
    se = _problem(8)
    Nf = len(se.w)
    nb_ = L.schedfunc(se, bounds=False)
    assert nb_.FBl is None and nb_.FBu is None and nb_.FBm is None and nb_.PBl is None and nb_.F.shape == (Nf, 100)
    se0 = L.SpectralExt(se.Y, se.X, se.V, se.w, se.Nv, se.λ, se.coulomb, se.normalize, se.x, None)
    assert L.schedfunc(se0).FBl is None
    for normalization in ("sum", "max"):
        for normdim in ("freq", "v"):
            got = L.schedfunc(se, normalization=normalization, normdim=normdim, bounds=False)
            want = R.schedfunc(se.x, se.Σ, se.V, se.w, se.Nv, se.normalize, se.coulomb, normalization=normalization, normdim=normdim)
            assert np.allclose(got.F, want["F"], rtol=1e-11, atol=0), (normalization, normdim)
    plain = L.schedfunc(se, nMC=200, seed=3)
    scaled = L.schedfunc(se, nMC=200, seed=3, normalization="max")
    assert np.array_equal(plain.FBl, scaled.FBl) and np.array_equal(plain.FBu, scaled.FBu)   # the bands are not normalised (as written)
    mm = L.schedfunc(se, nMC=200, seed=3, mcmean=True)
    assert np.array_equal(mm.line, mm.FBm) and np.array_equal(plain.line, plain.F) and np.array_equal(nb_.line, nb_.F)
    Y, V, X = se.Y, se.V, se.X
    sp = L.ls_sparse_spectral_lpv(Y, X, V, W_TEST, 8, λ=5, iters=200, tol=0, printerval=1000)
    assert sp.Σ is None
    s2 = L.schedfunc(sp)
    assert s2.F.shape == (Nf, 100) and s2.FBl is None and np.isfinite(s2.F).all()
    t = L.cn_last_timing()
    assert t["draws"] == 200 and t["cells"] == Nf * 100 and t["bands_ms"] > 0


def test_errors(L):
    from lpvspectral_jl_amd import api
    from lpvspectral_jl_amd._lib import lib, LPVS_EARGUMENT, LPVS_EUNSUPPORTED
    se = _problem(8)
    with pytest.raises(ValueError):
        L.schedfunc(se, nMC=9)
    with pytest.raises(NotImplementedError):
        L.schedfunc(se, nMC=16385)
    Nf, nb = len(se.w), 8
    Φ = np.asfortranarray(np.ones((100, nb)) / nb)
    o = [np.full((Nf, 100), 7.0, order="F") for _ in range(3)]
    with api._CnHandle(se.x, se.Σ, 0) as h:
        args = lambda nMC: (h.h, Nf, nb, C.c_void_p(Φ.ctypes.data), 100, nMC, 0, None, 0, *[C.c_void_p(a.ctypes.data) for a in o], None, None, None)
        assert lib().lpvs_cn_bands_f64(*args(9)) == LPVS_EARGUMENT
        assert lib().lpvs_cn_bands_f64(*args(16385)) == LPVS_EUNSUPPORTED
        assert all((a == 7.0).all() for a in o)
    assert lib().lpvs_cn_rand_f64(123456789, 4, 0, None, C.c_void_p(o[0].ctypes.data), C.c_void_p(o[1].ctypes.data)) == LPVS_EARGUMENT   # unknown handle


def test_detrend_on_a_device_tensor(L):
    import torch
    rng = np.random.default_rng(8)
    x, t = rng.standard_normal(1000), np.sort(rng.random(1000))
    xd = torch.from_numpy(x).cuda()
    got = L.detrend(xd, 1, t)
    assert got.is_cuda and torch.equal(xd, torch.from_numpy(x).cuda())          # a copy on the tensor's own device; the input is unchanged
    assert np.allclose(got.cpu().numpy(), R.detrend(x, 1, t), rtol=0, atol=1e-12)
    L.detrend_(xd)
    assert np.allclose(xd.cpu().numpy(), R.detrend(x), rtol=0, atol=1e-14)
