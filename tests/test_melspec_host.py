"""spectrogram / melspectrogram / mfcc (DSP.spectrogram, src/mel.jl): what is decided on the host -- nextfastfft, the Float32
filterbank in both precisions, the reference's mel facts, dct_matrix, the argument errors and the DeviceError without a GPU.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _melspec_ref as R  # noqa: E402


def _has_device(L):
    return L._lib.lib().lpvs_device_count() > 0


def test_nextfastfft_against_brute_force(L):
    for n in range(0, 5001):
        assert L.nextfastfft(n) == R.nextfastfft(n), n


@pytest.mark.parametrize("fs,nfft,kw", [
    (1, 256, {}), (1000, 256, dict(fmin=100)), (16000, 512, dict(nmels=40)), (22050, 2048, dict(nmels=128, fmin=20, fmax=8000)),
    (44100.0, 1024, {}), (8000, 125, dict(nmels=64)), (16000, 400, dict(fmin=np.float32(50.5), fmax=7600.0)),
    (48000.0, 4096, dict(fmin=30.0, nmels=96)),
])
def test_filterbank_matches_the_restatement(L, fs, nfft, kw):
    W = L.mel(fs, nfft, **kw)
    Wr = R.mel(fs, nfft, **kw)
    nm = kw.get("nmels", 128)
    assert W.dtype == np.float32 and W.shape == (nm, (nfft >> 1) + 1)
    np.testing.assert_allclose(W, Wr, rtol=1e-5, atol=1e-7 * float(np.max(np.abs(Wr))))


def test_filterbank_is_sparse_and_contiguous(L):
    W = L.mel(16000, 1024, nmels=80)
    assert (np.count_nonzero(W, axis=0) <= 2).all()                  # every bin lies in at most two filters
    for row in W:
        nz = np.flatnonzero(row)
        assert len(nz) == 0 or nz[-1] - nz[0] + 1 == len(nz)          # each filter's support is contiguous


def test_reference_mel_facts(L):
    M = L.mel(1, 256)
    assert M.shape == (128, 256 // 2 + 1)                            # test/runtests.jl: size(mel(1,256))
    M = L.mel(1000, 256, fmin=100)
    assert M[:, :26].sum() == 0                                      # the reference's unasserted sum(M[:,1:26]) == 0


def test_mel_scale_helpers(L):
    f = np.array([0.0, 500.0, 1000.0, 4000.0])
    assert np.allclose(L.mel_to_hz(L.hz_to_mel(f)), f, rtol=1e-12)
    assert L.hz_to_mel(np.float32(1000)).dtype == np.float32 and L.hz_to_mel(1000.0).dtype == np.float64
    fr = L.fft_frequencies(8000, 16)
    assert fr.dtype == np.float32 and fr[0] == 0 and fr[-1] == 4000 and len(fr) == 9
    mf = L.mel_frequencies(10, 0, 8000.0)
    assert len(mf) == 10 and mf.dtype == np.float64 and abs(mf[-1] - 8000) < 1e-6


def test_dct_matrix(L):
    for nf, ni in ((20, 128), (13, 40), (1, 2)):
        D = L.dct_matrix(nf, ni)
        assert D.dtype == np.float32 and D.shape == (nf, ni)
        np.testing.assert_allclose(D, R.dct_matrix(nf, ni), rtol=0, atol=4e-7)
        i = np.arange(1, nf + 1)[:, None]
        exact = np.cos(i * (2 * np.arange(ni) + 1) * np.pi / (2 * ni)) * np.sqrt(2 / ni)
        np.testing.assert_allclose(D, exact, rtol=0, atol=5e-6)


def test_argument_errors(L):
    y = np.random.default_rng(0).standard_normal(1000)
    with pytest.raises(L.DomainError):
        L.spectrogram(y, 100, 100)                                   # noverlap >= n
    with pytest.raises(L.DomainError):
        L.melspectrogram(y, 100, 120)
    with pytest.raises(ValueError):
        L.spectrogram(y, 100, 50, nfft=64)                           # nfft < n
    with pytest.raises(ValueError):
        L.mfcc(y, nmfcc=128, nmels=128)                              # nmfcc >= nmels
    with pytest.raises(ValueError):
        L.spectrogram(y + 1j * y, 100)                               # complex s
    with pytest.raises(ValueError):
        L.spectrogram(y, 100, 50, window=np.ones(99))                # window length


def test_device_entries_raise_without_a_device(L):
    if _has_device(L):
        pytest.skip("a device is visible: the GPU tests cover the computation")
    y = np.random.default_rng(0).standard_normal(1000)
    with pytest.raises(L.DeviceError):
        L.spectrogram(y, 125)
    with pytest.raises(L.DeviceError):
        L.melspectrogram(y)
    with pytest.raises(L.DeviceError):
        L.mfcc(y)
    S = L.Spectrogram(np.ones((63, 4)), np.arange(63.0), np.arange(4.0))
    with pytest.raises(L.DeviceError):
        L.melspectrogram(S)


@pytest.mark.parametrize("nfft", [7 ** 9, 5 ** 11, 2 ** 25 + 1])
def test_unsupported_lengths_raise_before_any_device(L, nfft):
    """7^9 and 5^11 are 7-smooth with no split into two factors <= 8192; 2^25 + 1 (3·11·251·4051) needs a Bluestein length above 2^26.
    The count-only call decides this before it looks for a device."""
    with pytest.raises(NotImplementedError):
        L.spectrogram(np.zeros(16), 16, 0, nfft=nfft)
    with pytest.raises(NotImplementedError):
        L.spectrogram(np.zeros(16, dtype=np.float32), 16, 0, nfft=nfft)


# ---- the long-double reference and its bound (tests/_melspec_ref.py: power_ld, power_bound) -------------------------------------------
@pytest.mark.parametrize("nfft", [1, 2, 3, 7, 11, 64, 97, 100, 127, 343, 1000, 1009, 4096, 4099, 8191, 8192])
def test_power_ld_matches_numpy(nfft):
    rng = np.random.default_rng(nfft)
    n = max(1, nfft - nfft // 5)
    y = rng.standard_normal(4 * n + 3)
    for window, fs in ((None, 1), (rng.random(n), 3.5)):
        P, Pt, r_err = R.power_ld(y, n, n // 3, nfft, fs=fs, window=window)
        Pn = R.power(y, n, n // 3, nfft, fs=fs, window=window)
        assert P.shape == Pn.shape and np.allclose(Pt, Pn.sum(axis=0), rtol=1e-13, atol=0)
        assert r_err < 1e-13
        np.testing.assert_allclose(P, Pn, rtol=0, atol=1e-13 * Pt.max())
        idx = [0, P.shape[1] - 1]
        Pi, Pti, _ = R.power_ld(y, n, n // 3, nfft, fs=fs, window=window, idx=idx)
        assert np.array_equal(Pi, P[:, idx]) and np.array_equal(Pti, Pt[idx])


@pytest.mark.parametrize("nfft", [2 ** 16, 3 * 2 ** 16, 5 ** 8])
def test_numpy_fft_within_c_np(nfft):
    """The largest lengths check the device against numpy's f64 FFT with C_NP added to c: numpy itself must be within C_NP."""
    y = np.random.default_rng(nfft).standard_normal(2 * nfft)
    P, Pt, r_err = R.power_ld(y, nfft, 0, nfft)
    Pn, _, _ = R.power_ld(y, nfft, 0, nfft, ld=False)
    assert (np.abs(Pn - P) <= R.power_bound(P, Pt, nfft, R.C_NP, r_err)).all()


def test_c_needed_inverts_the_bound():
    rng = np.random.default_rng(1)
    P = rng.random((33, 4)) ** 4
    Pt = P.sum(axis=0)
    for c in (0.01, 1.0, 7.0):
        b = R.power_bound(P, Pt, 64, c)
        np.testing.assert_allclose(R.c_needed(b, P, Pt, 64), c, rtol=1e-9)
    assert (R.c_needed(np.zeros_like(P), P, Pt, 64) == 0).all()


@pytest.mark.parametrize("nfft", [1000, 4099, 8192])
def test_bound_is_sharp(nfft):
    """One bin perturbed by 1e-12 relative fails the bound at the largest c of any path, and the old 1e-12·Ptot check misses it."""
    y = np.random.default_rng(nfft).standard_normal(3 * nfft)
    P, Pt, r_err = R.power_ld(y, nfft, 0, nfft)
    Pn = R.power(y, nfft, 0, nfft)
    cmax = 14.0                                                       # the largest per-path c of tests/test_gpu_stft_paths.py (LDS)
    bound = R.power_bound(P, Pt, nfft, cmax, r_err)
    assert (np.abs(Pn - P) <= bound).all()
    k = int(np.argmax(P[:, 1]))
    Pp = Pn.copy()
    Pp[k, 1] *= 1 + 1e-12
    assert not (np.abs(Pp - P) <= bound).all()
    assert (np.abs(Pp - P) <= 1e-12 * Pt).all()
    for c in (1e-2, 1.0):                                             # a zero frame's bound is exactly 0
        assert (R.power_bound(np.zeros((5, 1)), np.zeros(1), 64, c) == 0).all()


def test_mel_and_mfcc_bounds_cover_their_own_rounding(L):
    """The reference's own mel and MFCC, recomputed from numpy's power, stay inside the bounds carried from the power bound."""
    nfft, nmels, nmfcc = 1024, 40, 13
    y = np.random.default_rng(3).standard_normal(5 * nfft)
    P, Pt, r_err = R.power_ld(y, nfft, 0, nfft)
    Pn = R.power(y, nfft, 0, nfft)
    W = R.mel(1, 2 * (nfft // 2 + 1) - 1, nmels=nmels)
    pb = R.power_bound(P, Pt, nfft, 14.0, r_err)
    M, Mn = R.project(W, P), R.project(W, Pn)
    mb = R.mel_bound(W, P, pb)
    assert (np.abs(Mn - M) <= mb).all()
    D = R.dct_matrix(nmfcc, nmels)
    Cb = R.mfcc_bound(D, M, mb)
    assert (np.abs(R.mfcc_from_mel(D, Mn) - R.mfcc_from_mel(D, M)) <= Cb).all()
    M2 = M.copy()
    M2[3, 2] *= 1 + 1e-9                                              # a 1e-9 relative error in one band is caught
    assert not (np.abs(M2 - M) <= mb).all()
