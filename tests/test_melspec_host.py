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
