"""ComplexNormal's n x n host algebra, detrend and the argument checks that return before any device call, against the numpy
restatement of the reference (tests/_cnormal_ref.py); the restatement's own generator checks.  test/runtests.jl:115-152."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cnormal_ref as R  # noqa: E402


def _spd(rng, n):
    A = rng.standard_normal((n, n))
    return A.T @ A + np.eye(n)


def test_reference_testset_shapes_and_constructors(L):
    """test/runtests.jl:126-152"""
    rng = np.random.default_rng(0)
    n, n2 = 10, 5
    a, A = rng.standard_normal(n), _spd(rng, n)
    b = rng.standard_normal(n2)
    X, Y = rng.standard_normal((n, n2)), rng.standard_normal((n, n2))
    cn = L.ComplexNormal(X, Y)
    assert cn.m.shape == (n2,) and cn.Γ.shape == (n2, n2) and cn.C.shape == (n2, n2)
    m, G, C, V = R.from_samples(X, Y)
    assert np.allclose(cn.m, m, rtol=0, atol=1e-15) and np.allclose(cn.Γ, G, rtol=1e-13) and np.allclose(cn.C, C, rtol=1e-13)
    for z in (b, 1j * b):
        got, want = L.pdf(cn, z), R.pdf(m, G, C, z)
        assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    U = L.cn_Vxx(A, A)
    assert np.array_equal(U, np.triu(U)) and (np.diag(U) > 0).all()
    assert np.allclose(U.T @ U, L.cn_fVxx(A, A), rtol=1e-13, atol=1e-13)
    S = L.cn_fVxx(A, A)
    assert isinstance(S, np.ndarray) and np.array_equal(S, S.T)
    L.cn_V(A, 0.1 * A)
    c1 = L.ComplexNormal(a, A)                      # real mean of length 2n
    assert c1.m.shape == (n // 2,) and np.array_equal(c1.m, a[:5] + 1j * a[5:])
    c2 = L.ComplexNormal(1j * b, A)                 # complex mean of length n
    assert np.array_equal(c2.m, 1j * b)
    m2, G2, C2 = R.from_mean_cov(a, A)
    assert np.array_equal(c1.Γ, G2) and np.array_equal(c1.C, C2)
    c3 = L.ComplexNormal(X + 1j * Y)                # complex sample matrix
    assert np.array_equal(c3.m, cn.m) and np.array_equal(c3.Γ, cn.Γ) and np.array_equal(c3.C, cn.C)
    assert np.array_equal(L.Σ(cn), cn.Γ)           # as written: Matrix(Γ)


def test_accessors_match_the_restatement(L):
    rng = np.random.default_rng(1)
    V = _spd(rng, 12)
    cn = L.ComplexNormal(rng.standard_normal(6) + 1j * rng.standard_normal(6), V)
    G, C = R.cn_V2GC(V)
    for name in ("cn_fVxx", "cn_fVyy", "cn_fVxy", "cn_fVyx", "cn_fV"):
        assert np.array_equal(getattr(L, name)(cn), getattr(R, name)(G, C)), name
        assert np.array_equal(getattr(L, name)(cn.Γ, cn.C), getattr(R, name)(G, C)), name
    assert np.allclose(L.cn_V(cn), R.cn_V(G, C), rtol=1e-13, atol=1e-14)
    Uyy = L.cn_Vyy(V[:6, :6] + 0j, 0.1 * V[:6, :6] + 0j)
    assert np.allclose(Uyy.T @ Uyy, 0.45 * V[:6, :6], rtol=1e-13)
    with pytest.raises(ArithmeticError):
        L.cn_Vs(V[:6, :6] + 0j, 0.1 * V[:6, :6] + 0j)   # the cross blocks of a real pair are zero: PosDefException, as in the reference
    A, b = rng.standard_normal((3, 6)), rng.standard_normal(3)
    t = L.affine_transform(cn, A, b)
    tm, tG, tC = R.affine_transform(cn.m, G, C, A, b)
    assert np.allclose(t.m, tm) and np.allclose(t.Γ, tG) and np.allclose(t.C, tC)


def test_fV_of_V2GC_is_V(L):
    """The identity the device path relies on when it factors V directly: within 4 ulp of max|V|."""
    rng = np.random.default_rng(2)
    V = _spd(rng, 40)
    V = np.triu(V) + np.triu(V, 1).T
    back = L.cn_fV(*L.cn_V2ΓC(V))
    assert np.abs(back - V).max() <= 4 * np.spacing(np.abs(V).max())


def test_detrend(L):
    """test/runtests.jl:115-122"""
    tre = np.array([1, 2, 3])
    assert np.array_equal(L.detrend(tre), [-1, 0, 1])
    assert np.array_equal(tre, [1, 2, 3])
    assert np.array_equal(L.detrend([1, 2, 3]), [-1, 0, 1])
    L.detrend_(tre)
    assert np.array_equal(tre, [-1, 0, 1])
    rng = np.random.default_rng(3)
    x, t = rng.standard_normal(257), np.sort(rng.random(257))
    got = L.detrend(x, 1, t)
    assert np.array_equal(got.view(np.uint64), R.detrend(x, 1, t).view(np.uint64))
    assert np.array_equal(L.detrend(x, 1).view(np.uint64), R.detrend(x, 1).view(np.uint64))
    assert np.array_equal(L.detrend(x).view(np.uint64), R.detrend(x).view(np.uint64))


def test_argument_checks_before_any_device_call(L):
    rng = np.random.default_rng(4)
    with pytest.raises(TypeError):
        L.ComplexNormal(rng.standard_normal((4, 2)))                 # one real matrix: not a constructor
    with pytest.raises(ValueError):
        L.ComplexNormal(rng.standard_normal(5), np.eye(5))            # odd real mean
    with pytest.raises(ValueError):
        L.ComplexNormal(rng.standard_normal(4) + 0j, np.eye(6))       # V does not match the mean
    cn = L.ComplexNormal(np.zeros(2) + 0j, np.eye(4))
    with pytest.raises(ValueError):
        L.rand(cn, 0)
    with pytest.raises(ValueError):
        L.rand(cn, 8, normals=np.zeros((8, 3)))
    se = L.SpectralExt(None, None, np.linspace(0, 1, 9), np.arange(1.0, 3.0), 2, 0.0, False, True, np.ones(4) + 0j, np.eye(8))
    assert L.SchedFunc.__dataclass_fields__.keys() >= {"w", "v", "F", "P", "FBl", "FBu", "FBm", "PBl", "PBu", "PBm"}
    assert callable(L.schedfunc) and se.Σ is not None
    from lpvspectral_jl_amd._lib import SIGNATURES
    for sym in ("lpvs_cholesky_upper_f64", "lpvs_randn_f64", "lpvs_cn_create_f64", "lpvs_cn_destroy", "lpvs_cn_rand_f64", "lpvs_cn_bands_f64",
                "lpvs_cn_last_timing", "lpvs_cov_f64"):
        assert sym in SIGNATURES


def test_philox_restatement_is_a_pure_function_of_seed_row_column():
    seed = 0x123456789ABCDEF
    full = R.uniform_words(seed, np.arange(40, dtype=np.uint64)[:, None], np.arange(12, dtype=np.uint64)[None, :])
    part = R.uniform_words(seed, np.arange(7, 19, dtype=np.uint64)[:, None], np.arange(12, dtype=np.uint64)[None, :])
    tr = R.uniform_words(seed, np.arange(40, dtype=np.uint64)[None, :], np.arange(12, dtype=np.uint64)[:, None])
    for k in range(4):
        assert full[k].max() <= 0xFFFFFFFF
        assert np.array_equal(full[k][7:19], part[k])
        assert np.array_equal(full[k], tr[k].T)
    other = R.uniform_words(seed + 1, np.arange(40, dtype=np.uint64)[:, None], np.arange(12, dtype=np.uint64)[None, :])
    assert not np.array_equal(full[0], other[0])


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10: all-zero and all-ones counter / key, and the digits-of-pi vector."""
    def run(ctr, key):
        return [int(v) for v in R.philox4x32_10([np.uint64(c) for c in ctr], key)]
    assert run([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert run([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert run([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


def test_restatement_normals_are_standard():
    z, r = R.randn(7, 0, 20000, 6)
    assert np.isfinite(z).all() and (r >= 0).all()
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02
    assert np.abs(np.corrcoef(z, rowvar=False) - np.eye(6)).max() < 0.03
    zl, _ = R.randn(7, 0, 200, 6, dtype=np.longdouble)
    assert np.abs(zl.astype(np.float64) - z[:200]).max() < 1e-14
