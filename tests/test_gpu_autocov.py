"""autocov / autocor at arbitrary sample times (src/autocov.jl) on the device: tau bit- and order-exact against the numpy restatement
(tests/_autocov_ref.py), acf within the stated bounds, the degenerate rules, the vector-of-vectors form, the reference's own testset
(test/runtests.jl:236-343), a large case against torch's stable sort, the count protocol at N = 2^17, device tensors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _autocov_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _check(tau, acf, rtau, racf, scale):
    tau, acf = np.asarray(tau), np.asarray(acf)
    assert tau.dtype == rtau.dtype and acf.dtype == racf.dtype, (tau.dtype, rtau.dtype, acf.dtype, racf.dtype)
    assert len(tau) == len(rtau)
    nan = np.isnan(rtau) if rtau.dtype.kind == "f" else np.zeros(len(rtau), bool)
    assert np.array_equal(np.isnan(tau) if tau.dtype.kind == "f" else nan, nan)
    assert np.array_equal(tau[~nan].view(np.uint8), rtau[~nan].view(np.uint8)), "tau differs (bits or order)"
    if len(acf) == 0:
        return
    ulp = np.spacing(np.maximum(np.abs(acf), np.abs(racf)).astype(racf.dtype)).astype(np.float64)
    err = np.abs(acf.astype(np.float64) - racf.astype(np.float64))
    eq = scale > 0
    # equidistant branch: 1e-13 of the lag sum's magnitude (plus the output's own rounding); elsewhere 2 ulp (bit-exact for autocov)
    bound = np.where(eq, 1e-13 * scale + ulp, 2 * ulp)
    both_nan = np.isnan(acf) & np.isnan(racf)
    bad = ~(err <= bound) & ~both_nan
    assert not bad.any(), f"{bad.sum()} acf values out of bounds, first at {np.argmax(bad)}: {acf[bad][:4]} vs {racf[bad][:4]}"


def _times(kind, N, rng, dtype):
    if kind == "random":
        return (100 * rng.random(N)).astype(dtype)
    if kind == "range":
        return range(1, N + 1)
    if kind == "range2":
        return range(3, 3 + 2 * N, 2)
    if kind == "step033":
        from decimal import Decimal                                  # collect(1:0.33:...): the doubles nearest to 1 + k*33/100
        return np.array([float(1 + k * Decimal("0.33")) for k in range(N)]).astype(dtype)
    if kind == "repeated":
        return np.sort(np.round(10 * rng.random(N))).astype(dtype)[rng.permutation(N)]
    if kind == "quirk":
        return np.array([k % 2 for k in range(N)], dtype=dtype)     # [0,1,0,1,...]: equidistant under the inner abs
    raise KeyError(kind)


def _span(t):
    a = R._as_times(t).astype(np.float64)
    return float(a.max() - a.min())


CASES = []
for N in (2, 3, 10, 100, 1000):
    for tk in ("random", "range", "range2", "step033", "repeated", "quirk"):
        for dt in (np.float64, np.float32):
            if tk.startswith("range") and dt == np.float32:
                continue
            CASES.append((N, tk, dt))
CASES += [(4097, "random", np.float64), (4097, "range", np.float64), (4097, "step033", np.float32), (4097, "repeated", np.float64)]


@pytest.mark.parametrize("N,tk,dt", CASES, ids=[f"N{c[0]}-{c[1]}-{np.dtype(c[2]).name}" for c in CASES])
def test_tau_and_acf_match_the_restatement(L, N, tk, dt):
    rng = np.random.default_rng(N * 7 + len(tk))
    t = _times(tk, N, rng, dt)
    y = rng.standard_normal(N).astype(dt)
    span = _span(t)
    lags = (0.0, 0.5 * span, 2 * span + 1, np.inf) if N <= 1000 else (0.1 * span, np.inf)
    for maxlag in lags:
        for kind in ("cov", "cor"):
            for normalize in ((False, True) if N <= 1000 else (N % 2 == 0,)):
                fn = L.autocov if kind == "cov" else L.autocor
                tau, acf = fn(t, y, maxlag, normalize=normalize)
                rtau, racf, sc = R.autofun(kind, t, y, maxlag, normalize)
                _check(tau, acf, rtau, racf, sc)


def test_nan_times_sort_last_and_nan_maxlag_keeps_every_pair(L):
    rng = np.random.default_rng(3)
    t = 10 * rng.random(50); t[[4, 17]] = np.nan
    y = rng.standard_normal(50)
    for maxlag in (np.nan, 3.0, np.inf):
        tau, acf = L.autocov(t, y, maxlag)
        rtau, racf, sc = R.autofun("cov", t, y, maxlag)
        _check(tau, acf, rtau, racf, sc)
    assert np.isnan(tau[-1]) and len(L.autocor(t, y, np.nan)[0]) == 50 * 51 // 2


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_degenerate_series(L, dt):
    rng = np.random.default_rng(5)
    tr = (10 * rng.random(20)).astype(dt)
    te = np.arange(20).astype(dt)
    for t in (tr, te):
        for y in (np.zeros(20, dt), np.full(20, 3.0, dt), np.full(20, 1e-9, dt)):
            for kind, fn in (("cov", L.autocov), ("cor", L.autocor)):
                tau, acf = fn(t, y, np.inf)
                rtau, racf, sc = R.autofun(kind, t, y, np.inf)
                _check(tau, acf, rtau, racf, sc)
    assert np.all(L.autocov(tr, np.full(20, 3.0, dt), np.inf)[1] == 0)
    assert np.all(L.autocor(te, np.zeros(20, dt), np.inf)[1] == 1)
    assert np.all(L.autocor(tr, np.full(20, 3.0, dt), np.inf)[1] == 1)
    # a constant non-zero series under equidistant autocor is NOT all ones (dot(y,y) >= eps)
    assert not np.all(L.autocor(te, np.full(20, 3.0, dt), np.inf)[1] == 1)


def test_vector_of_vectors_mixes_branches(L):
    rng = np.random.default_rng(11)
    ts = [np.arange(30.0), 100 * rng.random(25), range(0, 40, 2), np.array([0, 1, 0, 1, 0, 1.0]), 5 * rng.random(12)]
    ys = [rng.standard_normal(len(R._as_times(t))) for t in ts]
    ys[4][:] = 2.0
    for kind, fn in (("cov", L.autocov), ("cor", L.autocor)):
        for maxlag in (np.inf, 7.5):
            for normalize in (False, True):
                tau, acf = fn(ts, ys, maxlag, normalize=normalize)
                rtau, racf, sc = R.autofun(kind, ts, ys, maxlag, normalize)
                _check(tau.astype(np.float64), acf, rtau.astype(np.float64), racf, sc)


def _np_autocov(y, cor=False):                      # StatsBase autocov / autocor(y, demean=false), lags 0 .. min(N-1, 10 log10 N)
    N = len(y)
    lags = min(N - 1, int(np.round(10 * np.log10(N))))
    c = np.array([np.dot(y[: N - k], y[k:]) / N for k in range(lags + 1)])
    return c / (np.dot(y, y) / N) if cor else c


def test_reference_testset(L):
    """test/runtests.jl:236-343."""
    from scipy.signal import filtfilt
    rng = np.random.default_rng(1)

    def acfh_of(tau, acf, n):
        return np.array([acf[tau == i].mean() for i in range(n)])

    y = np.tile([1.0, 0.0, -1.0], 100)
    tau, acf = L.autocov(range(1, len(y) + 1), y, np.inf)
    acf0 = _np_autocov(y); acfh = acfh_of(tau, acf, len(acf0))
    assert np.allclose(acfh, acf0, rtol=0.01) and np.linalg.norm(acfh - acf0) < 0.01
    tau, acf = L.autocor(range(1, len(y) + 1), y, np.inf)
    acf0 = _np_autocov(y, True); acfh = acfh_of(tau, acf, len(acf0))
    assert np.allclose(acfh, acf0, rtol=0.01) and np.linalg.norm(acfh - acf0) < 0.1
    y = rng.standard_normal(100)
    tau, acf = L.autocor(range(1, 101), y, np.inf)
    acf0 = _np_autocov(y, True); acfh = acfh_of(tau, acf, len(acf0))
    assert np.allclose(acfh, acf0, rtol=0.01) and np.linalg.norm(acfh - acf0) < 0.1
    y = rng.standard_normal(10)
    tau, acf = L.autocov(range(1, 11), y, np.inf)
    acf0 = _np_autocov(y); acfh = acfh_of(tau, acf, len(acf0))
    assert np.allclose(acfh, acf0, rtol=0.01) and np.linalg.norm(acfh - acf0) < 0.2
    tau, acf = L.autocor(range(1, 11), y, np.inf)
    acf0 = _np_autocov(y, True); acfh = acfh_of(tau, acf, len(acf0))
    assert np.allclose(acfh, acf0, rtol=0.03) and np.linalg.norm(acfh - acf0) < 0.2
    ys = [rng.standard_normal(10) for _ in range(10)]
    T = np.arange(1.0, 101.0).reshape(10, 10, order="F")
    ts = [T[:, i] for i in range(10)]
    for cor, fn in ((False, L.autocov), (True, L.autocor)):
        tau, acf = fn(ts, ys, np.inf)
        acf0 = np.mean([_np_autocov(v, cor) for v in ys], axis=0); acfh = acfh_of(tau, acf, len(acf0))
        assert np.allclose(acfh, acf0, rtol=0.01) and np.linalg.norm(acfh - acf0) < 0.2
    tau, acf = L.autocor(range(1, 11), np.zeros(10), np.inf)
    assert np.all(acf == 1)
    assert L.isequidistant(range(1, 6)) and L.isequidistant(range(1, 10, 2)) and not L.isequidistant(range(9, 0, -2))
    for fn, bound in ((L.autocor, 0.05), (L.autocov, 0.025)):
        res = []
        for _ in range(10):
            t = 100 * rng.random(100)
            assert not L.isequidistant(t)
            t0 = range(0, 100)
            y, y0 = np.sin(0.05 * t), np.sin(0.05 * np.arange(100.0))
            tau0, acf0 = fn(t0, y0, np.inf, normalize=True)
            tau, acf = fn(t, y, np.inf)
            acff = filtfilt(np.ones(200), [200], acf)
            assert np.count_nonzero(tau == 0) == len(y)
            res.append(np.mean((acf0 - acff) ** 2) < bound)
        assert np.mean(res) > 0.7


def test_large_case_against_torch_stable_sort(L):
    """N = 2^14, non-equidistant, maxlag = Inf: 1.3e8 pairs, device in / device out, against torch.sort(stable=True)."""
    import torch
    N = 2 ** 14
    g = torch.Generator(device="cuda").manual_seed(7)
    t = 1000 * torch.rand(N, dtype=torch.float64, device="cuda", generator=g)
    y = torch.randn(N, dtype=torch.float64, device="cuda", generator=g)
    tau, acf = L.autocov(t, y, float("inf"))
    assert tau.is_cuda and acf.is_cuda and tau.numel() == N * (N + 1) // 2
    I, K = torch.triu_indices(N, N, device="cuda")
    rt = (t[K] - t[I]).abs()
    rv = y[I] * y[K]
    del I, K
    rt, o = torch.sort(rt, stable=True)
    rv = rv[o]
    del o
    assert torch.equal(tau.view(torch.int64), rt.view(torch.int64))
    assert torch.equal(acf.view(torch.int64), rv.view(torch.int64))
    del tau, acf, rt, rv
    torch.cuda.empty_cache()


def test_count_only_at_2_17(L):
    from lpvspectral_jl_amd import _lib
    N = 2 ** 17
    rng = np.random.default_rng(2)
    t = np.sort(rng.random(N) * N)
    y = rng.standard_normal(N)
    off = np.array([0, N], dtype=np.int64)
    n = C.c_int64(-1)
    _lib.check(_lib.lib().lpvs_autofun_f64(1, _lib.out_ptr(t), _lib.out_ptr(y), _lib.out_ptr(off), 1, np.inf, 0, 0, None, None, 0, C.byref(n)))
    assert n.value == N * (N + 1) // 2 == 8590000128
    maxlag = 10.0
    right = np.searchsorted(t, t + maxlag, side="right")                # t sorted: pairs (i, k >= i) with t[k] - t[i] <= maxlag
    expect = int(np.sum(right - np.arange(N)))
    _lib.check(_lib.lib().lpvs_autofun_f64(2, _lib.out_ptr(t), _lib.out_ptr(y), _lib.out_ptr(off), 1, maxlag, 0, 0, None, None, 0, C.byref(n)))
    assert n.value == expect


def test_capacity_protocol(L):
    from lpvspectral_jl_amd import _lib
    rng = np.random.default_rng(4)
    t, y = rng.random(40), rng.standard_normal(40)
    off = np.array([0, 40], dtype=np.int64)
    n = C.c_int64(-1)
    tau = np.full(100, -7.0); acf = np.full(100, -7.0)
    rc = _lib.lib().lpvs_autofun_f64(1, _lib.out_ptr(t), _lib.out_ptr(y), _lib.out_ptr(off), 1, np.inf, 0, 0, _lib.out_ptr(tau), _lib.out_ptr(acf),
                                     100, C.byref(n))
    assert rc == _lib.LPVS_EARGUMENT and n.value == 820
    assert np.all(tau == -7.0) and np.all(acf == -7.0)
    tau = np.full(820, -7.0); acf = np.full(820, -7.0)
    _lib.check(_lib.lib().lpvs_autofun_f64(1, _lib.out_ptr(t), _lib.out_ptr(y), _lib.out_ptr(off), 1, np.inf, 0, 0, _lib.out_ptr(tau),
                                           _lib.out_ptr(acf), 820, C.byref(n)))
    rtau, racf, _ = R.autofun("cov", t, y, np.inf)
    assert np.array_equal(tau, rtau) and np.array_equal(acf, racf)


@pytest.mark.parametrize("dt", ["float64", "float32"])
def test_device_tensors_match_host(L, dt):
    import torch
    rng = np.random.default_rng(9)
    t = (50 * rng.random(300)).astype(dt)
    te = np.arange(300).astype(dt)
    y = rng.standard_normal(300).astype(dt)
    for tt in (t, te):
        assert L.isequidistant(torch.from_numpy(tt).cuda()) == L.isequidistant(tt)
        for fn in (L.autocov, L.autocor):
            for maxlag in (np.inf, 12.0):
                h = fn(tt, y, maxlag, normalize=True)
                d = fn(torch.from_numpy(tt).cuda(), torch.from_numpy(y).cuda(), maxlag, normalize=True)
                assert d[0].is_cuda and d[1].is_cuda
                assert np.array_equal(d[0].cpu().numpy(), h[0]) and np.array_equal(d[1].cpu().numpy(), h[1])
