"""welch_pgram / periodogram on the device against the long-double reference of tests/_welch_ref.py (welch_ld: the long-double mean of
power_ld's columns).  Bound per bin, from constants the project already holds (C per path of tests/test_gpu_stft_paths.py, u = 2^-53):

    |Ŝ_k − S_k| <= (1/K) Σ_f power_bound(P_fk, Ptot_f, N, C[path], r_err) + (D + 2)·u·S_k      (+ 1 float ulp for f32)

D is the reported sum_chain: asserted <= 1100 and equal to the formula of DESIGN.md §4.10 (_welch_ref.sum_chain).  Every case asserts
the path and the FFT length it ran.  The exact properties (repeatability, power-of-two scaling, two-sided output, zero and non-finite
frames) are compared bitwise."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _melspec_ref as R  # noqa: E402
import _welch_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu

C = {1: 14.0, 2: 0.07, 3: 11.0, 4: 0.25}       # tests/test_gpu_stft_paths.py: the per-path constants of power_bound
C_NP = R.C_NP
U = R.U


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _noise(seed, size):
    return np.random.default_rng(seed).standard_normal(size)


def _m(nfft):
    return R.nextfastfft(2 * nfft - 1)


def check(L, y, n, nov, nfft, path, flen, window=None, fs=1, f32=False, B=None, pgram=False):
    """welch_pgram (periodogram when pgram) of y against welch_ld within the bound; returns (device output, timing)."""
    y = np.asarray(y, dtype=np.float32 if f32 else np.float64)
    if pgram:
        out = L.periodogram(y, nfft=nfft, fs=fs, window=window)
    else:
        out = L.welch_pgram(y, n, nov, nfft=nfft, fs=fs, window=window)
    tm = L.stft_last_timing()
    o = _np(out.power)
    assert (tm["path"], tm["fft_length"]) == (path, flen), tm
    if B is not None:
        assert tm["pairs_per_workgroup"] == B, tm
    K = R.frames(len(y), n, nov)
    assert tm["frames"] == K and o.shape == (nfft // 2 + 1,) and o.dtype == (np.float32 if f32 else np.float64)
    D, S = WR.sum_chain(K, path, tm["pairs_per_workgroup"], flen)
    print(f"welch n={n} nfft={nfft} K={K} path={path} B={tm['pairs_per_workgroup']}: sum_chain {tm['sum_chain']} (formula {D}), slabs {tm['slabs']} ({S})")
    assert tm["sum_chain"] == D and tm["slabs"] == S and D <= 1100, (tm, D, S)
    wr = None if window is None else np.asarray(window, dtype=np.float32 if f32 else np.float64).astype(np.float64)
    Sr, bound_fft, Kr = WR.welch_ld(y.astype(np.float64), n, nov, nfft, fs=fs, window=wr)
    assert Kr == K
    b = WR.welch_bound(Sr, bound_fft, C[path], flen, D, f32)
    err = np.abs(o.astype(np.float64) - Sr)
    print(f"    max err / bound {np.max(err / b):.3g}, max rel err {np.max(err / Sr):.3g}")
    assert np.isfinite(o).all() and (err <= b).all(), f"max err / bound {np.max(err / b):.3g}"
    assert np.array_equal(L.freq(out), np.arange(nfft // 2 + 1) * fs / nfft)
    return o, tm


# ---- 1. the LDS path ---------------------------------------------------------------------------------------------------------------
def test_lds_65533_frames(L):
    n, nov = 256, 192
    y = _noise(1, 2 ** 22)
    assert R.frames(len(y), n, nov) == 65533
    _, tm = check(L, y, n, nov, 256, 1, 256, window=L.hanning(n), B=32)
    assert tm["slabs"] == 1024 and tm["sum_chain"] == 63 + 10            # one batch of 64 frames per slab


@pytest.mark.parametrize("n,K", [(5000, 37), (8192, 6), (6000, 9)])
def test_lds_one_pair_per_workgroup(L, n, K):
    """One frame pair per workgroup; 8192 and 6000 have more bins than the workgroup's LDS sums hold (they live in its slab)."""
    check(L, _noise(n, n + (K - 1) * (n // 2)), n, n - n // 2, n, 1, n, B=1)


def test_lds_workgroups_stride_over_batches(L):
    """More than 1024 batches: every workgroup adds several batches into its slab; K is odd."""
    n, nov, K = 2048, 2047, 9001                                          # B = 4: 1126 batches, 1024 slabs, up to 2 batches each
    _, tm = check(L, _noise(2, n + K - 1), n, nov, n, 1, n, window=L.hanning(n), B=4)
    assert tm["slabs"] == 1024 and tm["sum_chain"] == 2 * 8 - 1 + 10


def test_lds_longest_chain(L):
    """B = 512 pairs per workgroup: one batch is already the 1024-frame chain, so every batch gets its own slab (the largest D)."""
    n, K = 8, 40 * 1024 + 7
    _, tm = check(L, _noise(3, n * K), n, 0, n, 1, n, B=512)
    assert tm["slabs"] == 41 and tm["sum_chain"] == 1023 + 6


def test_single_frame_and_zero_padding(L):
    check(L, _noise(4, 300), 300, 0, 300, 1, 300, B=1)                    # K = 1
    check(L, _noise(5, 200 * 9 + 13), 200, 50, 256, 1, 256, window=L.hanning(200))   # nfft > n


# ---- 2. Bluestein in LDS, four-step, Bluestein four-step ------------------------------------------------------------------------------
def test_bluestein_lds(L):
    check(L, _noise(6, 1000 * 40 + 3), 1000, 500, 1009, 3, 2025, window=L.hanning(1000))


def test_four_step_across_a_scratch_chunk(L):
    nfft, n, K = 16384, 16, 4100                                          # 2048 pairs per chunk: frames 0 .. 4095, 4096 .. 4099
    _, tm = check(L, _noise(7, n * K), n, 0, nfft, 2, nfft)
    assert tm["slabs"] == 16 + 1 and tm["sum_chain"] == 255 + 5


def test_bluestein_four_step(L):
    check(L, _noise(8, 4099 + 6 * 1000), 4099, 3099, 4099, 4, 8232)


# ---- 3. periodogram ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ls,path,flen", [(5000, 1, 5000), (2 ** 20, 2, 2 ** 20), (2 ** 20 + 1, 4, None), (3 * 2 ** 20, 2, 3 * 2 ** 20)])
@pytest.mark.parametrize("windowed", [False, True])
def test_periodogram(L, Ls, path, flen, windowed):
    flen = _m(Ls) if flen is None else flen
    w = L.hanning(Ls) if windowed else None
    _, tm = check(L, _noise(Ls, Ls), Ls, 0, Ls, path, flen, window=w, fs=3.0, pgram=True)
    assert tm["frames"] == 1 and tm["sum_chain"] == 0 and tm["slabs"] == 1


def test_periodogram_default_nfft(L):
    y = _noise(9, 4099)
    p = L.periodogram(y)
    assert L.stft_last_timing()["fft_length"] == R.nextfastfft(4099) and len(p.power) == R.nextfastfft(4099) // 2 + 1


# ---- 4. f32 twins --------------------------------------------------------------------------------------------------------------------------
def test_f32_twins(L):
    check(L, _noise(10, 2 ** 18), 256, 192, 256, 1, 256, window=L.hanning(256), f32=True)
    check(L, _noise(11, 1000 * 20), 1000, 500, 1009, 3, 2025, f32=True)
    check(L, _noise(12, 2 ** 20), 2 ** 20, 0, 2 ** 20, 2, 2 ** 20, f32=True, pgram=True)


# ---- 5. scipy as a second opinion -----------------------------------------------------------------------------------------------------------
def test_against_scipy(L):
    import scipy.signal
    n, nov, fs = 512, 256, 8000.0
    y = _noise(13, 2 ** 17)
    w = L.hanning(n)
    out = L.welch_pgram(y, n, nov, fs=fs, window=w)
    tm = L.stft_last_timing()
    f, Ps = scipy.signal.welch(y, fs=fs, window=w, nperseg=n, noverlap=nov, nfft=n, detrend=False, scaling="density")
    Sr, bound_fft, K = WR.welch_ld(y, n, nov, n, fs=fs, window=w)
    b = WR.welch_bound(Sr, bound_fft, C[1] + C_NP, n, tm["sum_chain"]) + bound_fft(C_NP, n) + K * U * Sr   # scipy's FFT and its own mean
    assert np.allclose(f, L.freq(out)) and (np.abs(_np(out.power) - Ps) <= b).all()
    yp = _noise(14, 5000)
    f, Pp = scipy.signal.periodogram(yp, fs=fs, detrend=False)
    out = L.periodogram(yp, fs=fs)
    Sr, bound_fft, _ = WR.welch_ld(yp, 5000, 0, 5000, fs=fs)
    assert (np.abs(_np(out.power) - Pp) <= WR.welch_bound(Sr, bound_fft, C[1] + C_NP, 5000, 0) + bound_fft(C_NP, 5000)).all()


# ---- 6. exact properties, bitwise ------------------------------------------------------------------------------------------------------------
EXACT = [(256, 192, 256, 20000), (1000, 500, 1009, 30000), (16384, 8192, 16384, 16384 * 6), (4099, 0, 4099, 4099 * 5)]


@pytest.mark.parametrize("n,nov,nfft,Ls", EXACT)
@pytest.mark.parametrize("f32", [False, True])
def test_repeatable_scaling_and_two_sided(L, n, nov, nfft, Ls, f32):
    dt = np.float32 if f32 else np.float64
    y = _noise(n, Ls).astype(dt)
    w = L.hanning(n).astype(dt)
    a = _np(L.welch_pgram(y, n, nov, nfft=nfft, window=w).power)
    assert np.isfinite(a).all() and np.array_equal(a, _np(L.welch_pgram(y, n, nov, nfft=nfft, window=w).power))   # two calls, same bits
    for s in (-30, 9):
        assert np.array_equal(_np(L.welch_pgram(np.ldexp(y, s).astype(dt), n, nov, nfft=nfft, window=w).power), np.ldexp(a, 2 * s))
    two = L.welch_pgram(y, n, nov, nfft=nfft, window=w, onesided=False)
    assert np.array_equal(_np(two.power), WR.twosided(a, nfft)) and np.array_equal(L.freq(two), np.fft.fftfreq(nfft, 1.0))


def test_device_tensors_in_and_out(L):
    import torch
    y = _noise(15, 50000)
    for dt in (torch.float64, torch.float32):
        t = torch.as_tensor(y).to(dt).cuda()
        p = L.welch_pgram(t, 500, 100, window=L.hanning(500))
        assert p.power.is_cuda and p.power.dtype == dt
        assert np.array_equal(_np(p.power), _np(L.welch_pgram(t.cpu().numpy(), 500, 100, window=L.hanning(500)).power))
        q = L.periodogram(t, onesided=False)
        assert q.power.is_cuda and q.power.shape == (R.nextfastfft(50000),)


@pytest.mark.parametrize("n,nfft", [(64, 64), (1000, 1009), (16384, 16384)])
def test_zero_frames_change_nothing_but_the_count(L, n, nfft):
    a, b, c, d = (_noise(20 + j, n) for j in range(4))
    z = np.zeros(n)
    four = _np(L.welch_pgram(np.concatenate([a, b, c, d]), n, 0, nfft=nfft).power)
    eight = _np(L.welch_pgram(np.concatenate([a, b, z, z, z, z, c, d]), n, 0, nfft=nfft).power)
    assert L.stft_last_timing()["frames"] == 8 and np.array_equal(eight, four / 2)


@pytest.mark.parametrize("n,nfft,bad", [(256, 256, np.nan), (1000, 1009, np.inf), (16384, 16384, -np.inf), (4099, 4099, np.nan)])
def test_a_non_finite_sample_makes_every_bin_nan(L, n, nfft, bad):
    y = _noise(30, 7 * n)
    y[4 * n + 3] = bad
    assert np.isnan(_np(L.welch_pgram(y, n, 0, nfft=nfft).power)).all()
    assert np.isnan(_np(L.welch_pgram(y, n, 0, nfft=nfft, onesided=False).power)).all()


def test_errors(L):
    y = _noise(31, 1000)
    with pytest.raises(L.DomainError):
        L.welch_pgram(y[:99], 100, 50)                                    # no frame: spectrogram returns zero frames, a mean does not exist
    with pytest.raises(L.DomainError):
        L.welch_pgram(y, 100, 100)
    with pytest.raises(ValueError):
        L.welch_pgram(y, 100, 50, nfft=64)
    with pytest.raises(ValueError):
        L.welch_pgram(y.astype(np.complex128), 100, 50)
    assert L.spectrogram(y[:99], 100, 50).power.shape[1] == 0
    # the library itself answers the same (the Python mirror checks before it calls)
    lib = L._lib.lib()
    out, k = np.zeros(64), ctypes.c_int64(-1)
    args = (ctypes.c_void_p(y.ctypes.data), 99, 100, 50, 100, 1.0, None, 1, 0, ctypes.c_void_p(out.ctypes.data), ctypes.byref(k))
    assert lib.lpvs_welch_f64(*args) == L._lib.LPVS_EDOMAIN and k.value == 0
    assert lib.lpvs_stft_f64(L._lib.STFT_WELCH, ctypes.c_void_p(y.ctypes.data), 1000, 100, 50, 100, 1.0, None, None, 0, None, 0, 0,
                             ctypes.c_void_p(out.ctypes.data), 64, ctypes.byref(k)) == L._lib.LPVS_EARGUMENT


# ---- 7. consistency with the spectrogram's columns (not the tolerance basis) --------------------------------------------------------------
@pytest.mark.parametrize("n,nov,nfft,Ls", EXACT)
def test_consistent_with_the_mean_of_the_spectrogram(L, n, nov, nfft, Ls):
    y = _noise(n + 1, Ls)
    w = L.hanning(n)
    a = _np(L.welch_pgram(y, n, nov, nfft=nfft, window=w).power)
    D = L.stft_last_timing()["sum_chain"]
    P = _np(L.spectrogram(y, n, nov, nfft=nfft, window=w).power)
    K = P.shape[1]
    Sm = P.mean(axis=1)
    assert (np.abs(a - Sm) <= (D + K) * U * Sm).all()
