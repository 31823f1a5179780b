"""welch_pgram / periodogram / compress / heatmap: what is decided on the host -- DSP.jl's signatures and defaults, compress's q
normalisation, Periodogram / freq, the argument errors raised before the library is called, the exported C-ABI, the chain-length
formula and the quantile reference itself.  CPU only."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _welch_ref as WR  # noqa: E402


def _has_device(L):
    return L._lib.lib().lpvs_device_count() > 0


def test_signatures_and_defaults(L):
    w = inspect.signature(L.welch_pgram)
    assert list(w.parameters) == ["s", "n", "noverlap", "onesided", "nfft", "fs", "window", "device"]
    assert [p.default for p in w.parameters.values()][1:] == [None, None, True, None, 1, None, 0]
    p = inspect.signature(L.periodogram)
    assert list(p.parameters) == ["s", "onesided", "nfft", "fs", "window", "device"]
    assert [q.default for q in p.parameters.values()][1:] == [True, None, 1, None, 0]
    assert list(inspect.signature(L.compress).parameters)[:2] == ["x", "q"]
    h = inspect.signature(L.heatmap)
    assert list(h.parameters)[:2] == ["S", "compression"] and h.parameters["compression"].default == (0.005, 1)


def test_periodogram_type_and_freq(L):
    P = L.Periodogram(np.arange(5.0), np.arange(5) / 8)
    assert L.freq(P) is P.freq and P.power[3] == 3
    S = L.Spectrogram(np.zeros((3, 2)), np.arange(3.0), np.arange(2.0))
    assert L.freq(S) is S.freq                                        # the existing types keep their answers


def test_q_normalisation(L):
    from lpvspectral_jl_amd.api import _quantile_pair
    assert _quantile_pair(0.005) == (0.005, 1 - 0.005)
    assert _quantile_pair(0.8) == (1 - 0.8, 1 - (1 - 0.8))            # q >= 0.5 -> 1 - q first (src/plotting.jl:40)
    assert _quantile_pair(0.5) == (0.5, 0.5) and _quantile_pair(1) == (0.0, 1.0) and _quantile_pair(0) == (0.0, 1.0)
    assert _quantile_pair((0.9, 0.1)) == (0.1, 0.9) and _quantile_pair([0.3, 0.3]) == (0.3, 0.3)
    assert _quantile_pair((0.005, 1)) == (0.005, 1.0)
    for q in (0.005, 0.8, 0.5, 1, (0.9, 0.1)):
        assert _quantile_pair(q) == WR.quantile_pair(q)
    for bad in (1.5, -0.1, (0.2, 1.01), (-1e-9, 0.5)):
        with pytest.raises(ValueError):
            _quantile_pair(bad)


def test_argument_errors_before_the_library(L):
    y = np.random.default_rng(0).standard_normal(1000)
    with pytest.raises(L.DomainError):
        L.welch_pgram(y[:99], 100, 50)                                    # L < n: the mean over no frame
    with pytest.raises(L.DomainError):
        L.welch_pgram(y[:7])                                              # default n = 7 >> 3 = 0
    with pytest.raises(L.DomainError):
        L.welch_pgram(y, 100, 100)
    with pytest.raises(L.DomainError):
        L.welch_pgram(y, 100, -1)
    with pytest.raises(ValueError):
        L.welch_pgram(y, 100, 50, nfft=99)
    with pytest.raises(ValueError):
        L.periodogram(y, nfft=999)
    with pytest.raises(ValueError):
        L.welch_pgram(y, 100, 50, window=np.ones(99))
    with pytest.raises(ValueError):
        L.welch_pgram(y.astype(np.complex128), 100, 50)
    with pytest.raises(ValueError):
        L.periodogram(1j * y)
    with pytest.raises(ValueError):
        L.compress(np.zeros((2, 2, 2)), 0.1)
    with pytest.raises(ValueError):
        L.compress(np.zeros((2, 2)), 2)
    with pytest.raises(ValueError):
        L.compress(np.zeros((2, 2), dtype=complex), 0.1)
    with pytest.raises(L.DomainError):
        L.compress(np.zeros((0, 3)), 0.1)
    with pytest.raises(TypeError):
        L.heatmap(L.MFCC(np.zeros((2, 2)), np.arange(1, 3), np.arange(2.0)))


def test_library_argument_checks_need_no_device(L):
    lib = L._lib.lib()
    y = np.random.default_rng(1).standard_normal(256)
    out, th, k = np.zeros(256), np.zeros(2), ctypes.c_int64(-1)
    yp, op = ctypes.c_void_p(y.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    E = L._lib
    assert lib.lpvs_welch_f64(yp, 63, 64, 32, 64, 1.0, None, 1, 0, op, ctypes.byref(k)) == E.LPVS_EDOMAIN and k.value == 0
    assert lib.lpvs_welch_f64(yp, 256, 64, 64, 64, 1.0, None, 1, 0, op, ctypes.byref(k)) == E.LPVS_EDOMAIN
    assert lib.lpvs_welch_f64(yp, 256, 64, 32, 63, 1.0, None, 1, 0, op, ctypes.byref(k)) == E.LPVS_EARGUMENT
    assert lib.lpvs_welch_f64(yp, 256, 64, 32, 64, 1.0, None, 1, 0, None, ctypes.byref(k)) == E.LPVS_EARGUMENT
    assert lib.lpvs_stft_f64(E.STFT_WELCH, yp, 256, 64, 32, 64, 1.0, None, None, 0, None, 0, 0, op, 256, ctypes.byref(k)) == E.LPVS_EARGUMENT
    tp = ctypes.c_void_p(th.ctypes.data)
    assert lib.lpvs_compress_f64(yp, 0, 4, 0, 0, 0.1, 0.9, 0, op, 0, tp) == E.LPVS_EDOMAIN
    assert lib.lpvs_compress_f64(yp, 16, 16, 15, 0, 0.1, 0.9, 0, op, 16, tp) == E.LPVS_EARGUMENT      # ld < rows
    assert lib.lpvs_compress_f64(yp, 16, 16, 16, 0, 0.1, 1.1, 0, op, 16, tp) == E.LPVS_EARGUMENT
    assert lib.lpvs_compress_f64(yp, 16, 16, 16, 0, float("nan"), 0.9, 0, op, 16, tp) == E.LPVS_EARGUMENT
    t = np.zeros(5)
    assert lib.lpvs_compress_last_timing(ctypes.c_void_p(t.ctypes.data), 5) == 0
    assert set(L.stft_last_timing()) >= {"sum_chain", "slabs", "path", "fft_length", "pairs_per_workgroup"}
    assert set(L.compress_last_timing()) == {"passes", "select_ms", "clamp_ms", "total_ms", "digits_skipped"}


def test_no_silent_cpu_fallback(L):
    if _has_device(L):
        pytest.skip("GPU present")
    y = np.random.default_rng(2).standard_normal(512)
    with pytest.raises(L.DeviceError):
        L.welch_pgram(y, 64, 32)
    with pytest.raises(L.DeviceError):
        L.periodogram(y)
    with pytest.raises(L.DeviceError):
        L.compress(y.reshape(16, 32), 0.1)
    with pytest.raises(L.DeviceError):
        L.heatmap(L.Spectrogram(np.abs(y).reshape(16, 32), np.arange(16.0), np.arange(32.0)))


def test_chain_formula():
    """D = F − 1 + ceil(log2 S) of DESIGN.md §4.10 on named cases; D <= 1100 wherever a workgroup chain is capped at 1024."""
    assert WR.sum_chain(65533, 1, 32, 256) == (63 + 10, 1024)            # L = 2^22, n = 256, noverlap = 192
    assert WR.sum_chain(65535, 1, 4, 2048) == (63 + 10, 1024)            # L = 2^26, n = 2048: 8192 batches of 8 frames, 8 per slab
    assert WR.sum_chain(1, 1, 1, 5000) == (0, 1) and WR.sum_chain(1, 2, 0, 2 ** 20) == (0, 1)
    assert WR.sum_chain(2, 1, 1, 8192) == (1, 1) and WR.sum_chain(3, 1, 1, 8192) == (1 + 1, 2)
    assert WR.sum_chain(4100, 2, 0, 16384) == (255 + 5, 17)
    assert WR.sum_chain(40 * 1024 + 7, 1, 512, 8) == (1023 + 6, 41)
    rng = np.random.default_rng(3)
    for _ in range(2000):
        B = int(2 ** rng.integers(0, 10))
        K = int(rng.integers(1, 2 ** 26 // B + 2))
        D, S = WR.sum_chain(K, 1, B, 8192 // B)
        assert 0 <= D <= 1023 + 26 and D <= 1100 and S >= 1
        flen = int(2 ** rng.integers(14, 27))
        D, S = WR.sum_chain(int(rng.integers(1, 100000)), 2, 0, flen)
        assert 0 <= D <= 255 + 17


def test_quantile_reference_is_numpys_default():
    """The formula the device is held to (Julia's default, type 7) against numpy.quantile's default on log-powers."""
    rng = np.random.default_rng(4)
    v = np.sort(np.log(rng.chisquare(2, 4000)))
    for p in (0, 0.005, 0.37, 0.995, 1):
        assert abs(WR.quantile7(v, p) - np.quantile(v, p)) <= 1e-13, p       # same definition; numpy rounds its index and its lerp differently
    assert WR.quantile7(np.array([2.5]), 0.3) == 2.5
    x = rng.standard_normal((7, 9)).astype(np.float32)
    out, th = WR.compress_ref(x, (0.9, 0.1))
    assert out.dtype == np.float32 and th[0] <= th[1] and out.min() >= np.float32(th[0]) - 1e-6 and out.max() <= np.float32(th[1]) + 1e-6
    assert np.array_equal(WR.twosided(np.array([1.0, 4.0, 6.0, 3.0]), 6), [1.0, 2.0, 3.0, 3.0, 3.0, 2.0])
    assert np.array_equal(WR.twosided(np.array([1.0, 4.0, 6.0]), 5), [1.0, 2.0, 3.0, 3.0, 2.0])
