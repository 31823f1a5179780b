"""spectrogram / melspectrogram / mfcc on the device (melspec.hip) against the numpy restatement (tests/_melspec_ref.py).

Bounds, with P the frame's total power: power within 1e-12·P per frame; mel band i within 1e-12·(Σ_k W_ik)·P; MFCC within 1e-10
after normalisation; the f32 entry points within the same bounds against the f64 restatement of the float-cast input plus 2 float ulp."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _melspec_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _check_power(P, Pr, ulp32=False):
    P = _np(P).astype(np.float64)
    assert P.shape == Pr.shape
    tot = Pr.sum(axis=0, keepdims=True)
    bound = 1e-12 * tot + (2 * np.spacing(np.abs(Pr).astype(np.float32)).astype(np.float64) if ulp32 else 0)
    err = np.abs(P - Pr)
    assert (err <= bound).all(), f"max err / P = {np.max(err / np.maximum(tot, 1e-300)):.3e}"


def _check_mel(M, W, Pr, ulp32=False):
    M = _np(M).astype(np.float64)
    Mr = R.project(W, Pr)
    assert M.shape == Mr.shape
    bound = 1e-12 * W.astype(np.float64).sum(axis=1, keepdims=True) * Pr.sum(axis=0, keepdims=True)
    if ulp32:
        bound = bound + 2 * np.spacing(np.abs(Mr).astype(np.float32)).astype(np.float64)
    err = np.abs(M - Mr)
    assert (err <= bound).all(), f"max mel err {np.max(err):.3e}"
    return Mr


def _hann(n):
    from lpvspectral_jl_amd import hanning
    return hanning(n)


@pytest.mark.parametrize("nfft", [125, 128, 343, 1000, 2048, 4096, 8192])
def test_power_lds_lengths(L, nfft):
    rng = np.random.default_rng(nfft)
    n = nfft
    y = rng.standard_normal(6 * n + 17)
    for nov in (0, n // 2, n - 1):
        S = L.spectrogram(y, n, nov)
        _check_power(S.power, R.power(y, n, nov, nfft))
        assert np.allclose(S.freq, np.arange(nfft // 2 + 1) / nfft)
        k = R.frames(len(y), n, nov)
        assert np.allclose(S.time, (n / 2 + np.arange(k) * (n - nov)))


@pytest.mark.parametrize("n,nfft", [(100, 128), (125, 343), (1000, 1024), (999, 1000), (300, 315)])
def test_zero_padding_odd_even_fs_and_windows(L, n, nfft):
    rng = np.random.default_rng(n)
    y = rng.standard_normal(10 * n)
    custom = rng.random(n)
    for window, w in ((None, None), (L.rect, np.ones(n)), (_hann, _hann(n)), (custom, custom)):
        S = L.spectrogram(y, n, n // 3, nfft=nfft, fs=3.5, window=window)
        _check_power(S.power, R.power(y, n, n // 3, nfft, fs=3.5, window=w))
        assert np.allclose(S.time, (n / 2 + np.arange(S.power.shape[1]) * (n - n // 3)) / 3.5)


@pytest.mark.parametrize("n,nfft,L_", [(2 ** 14 * 3, 2 ** 14 * 3, 2 ** 14 * 3 * 5), (2 ** 21, 2 ** 21, 2 ** 24)])
def test_power_four_step(L, n, nfft, L_):
    y = np.random.default_rng(7).standard_normal(L_)
    nov = n >> 1
    S = L.spectrogram(y, n, nov, nfft=nfft, window=_hann)
    assert L.stft_last_timing()["path"] == 2
    _check_power(S.power, R.power(y, n, nov, nfft, window=_hann(n)))


def test_reference_default_n_at_2_24_is_four_step_mel(L):
    y = np.random.default_rng(8).standard_normal(2 ** 24)
    n = len(y) >> 3                                                   # 2^21
    M = L.melspectrogram(y, fs=16000)
    assert L.stft_last_timing()["path"] == 2 and M.power.shape == (128, 15)
    W = L.mel(16000, 2 ** 21 + 1)
    _check_mel(M.power, W, R.power(y, n, n >> 1, n, fs=16000, window=_hann(n)))


@pytest.mark.parametrize("n,nfft,L_,path", [(1000, 1009, 7000, 3), (2 ** 20, 2 ** 20 + 1, 3 * 2 ** 20, 4)])
def test_power_bluestein(L, n, nfft, L_, path):
    y = np.random.default_rng(9).standard_normal(L_)
    S = L.spectrogram(y, n, n // 2, nfft=nfft, window=_hann)
    assert L.stft_last_timing()["path"] == path
    _check_power(S.power, R.power(y, n, n // 2, nfft, window=_hann(n)))


def test_fewer_samples_than_n_gives_no_frames(L):
    S = L.spectrogram(np.ones(100), 128)
    assert S.power.shape == (65, 0) and len(S.time) == 0
    assert L.melspectrogram(np.ones(100), 128).power.shape == (128, 0)


def test_large_signal_sampled_frames(L):
    y = np.random.default_rng(10).standard_normal(2 ** 26)
    n, nov = 2048, 1024
    S = L.spectrogram(y, n, nov, window=_hann)
    k = R.frames(len(y), n, nov)
    assert S.power.shape == (1025, k)
    idx = np.sort(np.random.default_rng(11).choice(k, 300, replace=False))
    hop = n - nov
    Pr = np.concatenate([R.power(y[j * hop: j * hop + n], n, 0, n, window=_hann(n)) for j in idx], axis=1)
    _check_power(S.power[:, idx], Pr)
    W = L.mel(1, n)
    M = L.melspectrogram(y, n, nov)
    _check_mel(M.power[:, idx], W, Pr)


@pytest.mark.parametrize("nfft", [128, 343, 1009])
def test_melspectrogram_and_mfcc(L, nfft):
    rng = np.random.default_rng(nfft + 1)
    n = min(nfft, 1000)
    y = rng.standard_normal(20 * n)
    for fs, kw in ((1, {}), (16000, dict(nmels=40, fmin=20, fmax=7000.0)), (22050.0, dict(nmels=64))):
        M = L.melspectrogram(y, n, n // 2, nfft=nfft, fs=fs, **kw)
        nmels = kw.get("nmels", 128)
        fmax = kw.get("fmax", float(fs) / 2 if isinstance(fs, float) else np.float32(fs / 2))
        W = L.mel(fs, 2 * (nfft // 2 + 1) - 1, nmels=nmels, fmin=kw.get("fmin", np.float32(0)), fmax=fmax)
        Pr = R.power(y, n, n // 2, nfft, fs=fs, window=_hann(n))
        Mr = _check_mel(M.power, W, Pr)
        assert len(M.mels) == nmels and np.allclose(M.time, (n / 2 + np.arange(Pr.shape[1]) * (n - n // 2)) / fs)
        C = L.mfcc(y, n, n // 2, nfft=nfft, fs=fs, nmfcc=13, **kw)
        Cr = R.mfcc_from_mel(L.dct_matrix(13, nmels), Mr)
        assert C.mfcc.shape == Cr.shape and np.max(np.abs(C.mfcc - Cr)) <= 1e-10
        assert list(C.number) == list(range(1, 14))


def test_reference_mel_testset(L):
    M = L.mel(1, 256)
    assert M.shape == (128, 129)
    assert L.mel(1000, 256, fmin=100)[:, :26].sum() == 0
    y = np.random.default_rng(12).standard_normal(1000)
    M = L.melspectrogram(y)
    assert len(L.freq(M)) == 128 and M.power.shape == (128, 14) and len(L.time(M)) == 14
    C = L.mfcc(y)
    assert len(L.freq(C)) == 20 and C.mfcc.shape == (20, 14) and len(L.time(C)) == 14


def test_melspectrogram_of_a_spectrogram(L):
    import torch
    y = np.random.default_rng(13).standard_normal(5000)
    n = 250
    S = L.spectrogram(y, n, 100, window=_hann)
    direct = L.melspectrogram(y, n, 100)
    Pr = R.power(y, n, 100, R.nextfastfft(n), window=_hann(n))
    W = L.mel(1, 2 * S.power.shape[0] - 1)
    for src in (S, L.Spectrogram(torch.from_numpy(np.asarray(S.power)).cuda(), S.freq, S.time)):
        M = L.melspectrogram(src)
        _check_mel(M.power, W, Pr)
    _check_mel(direct.power, W, Pr)


def test_nan_rules(L):
    y = np.random.default_rng(14).standard_normal(4000)
    n, nov = 200, 100
    y[1234] = np.nan
    M = _np(L.melspectrogram(y, n, nov).power)
    k = M.shape[1]
    has = np.array([j * (n - nov) <= 1234 < j * (n - nov) + n for j in range(k)])
    assert np.isnan(M[:, has]).all() and not np.isnan(M[:, ~has]).any()
    S = _np(L.spectrogram(y, n, nov).power)                          # the pair partner of a NaN frame keeps its power
    assert np.isnan(S[:, has]).all() and not np.isnan(S[:, ~has]).any()
    C = L.mfcc(np.zeros(4000), n, nov)
    assert np.isnan(C.mfcc).all()
    n = 3 * 2 ** 14                                                  # four-step: the frames are flagged before the FFT
    y = np.random.default_rng(18).standard_normal(5 * n)
    y[n + 5] = np.inf
    M = _np(L.melspectrogram(y, n, n // 2).power)
    has = np.array([j * (n - n // 2) <= n + 5 < j * (n - n // 2) + n for j in range(M.shape[1])])
    assert L.stft_last_timing()["path"] == 2
    assert np.isnan(M[:, has]).all() and not np.isnan(M[:, ~has]).any()


def test_f32_entry_points(L):
    rng = np.random.default_rng(15)
    for nfft, n in ((256, 256), (343, 300), (1009, 1000), (2 ** 14 * 3, 2 ** 14 * 3)):
        y = rng.standard_normal(5 * n).astype(np.float32)
        S = L.spectrogram(y, n, n // 2, nfft=nfft, window=lambda m: _hann(m).astype(np.float32))
        assert S.power.dtype == np.float32
        w = _hann(n).astype(np.float32).astype(np.float64)
        Pr = R.power(y.astype(np.float64), n, n // 2, nfft, window=w)
        _check_power(S.power, Pr, ulp32=True)
        M = L.melspectrogram(y, n, n // 2, nfft=nfft, window=lambda m: _hann(m).astype(np.float32))
        _check_mel(M.power, L.mel(1, 2 * (nfft // 2 + 1) - 1), Pr, ulp32=True)


def test_deterministic(L):
    y = np.random.default_rng(16).standard_normal(2 ** 18)
    for kw in (dict(n=2048), dict(n=1000, nfft=1009), dict(n=2 ** 15, nfft=2 ** 15)):
        a = _np(L.mfcc(y, kw["n"], nfft=kw.get("nfft")).mfcc)
        b = _np(L.mfcc(y, kw["n"], nfft=kw.get("nfft")).mfcc)
        assert np.array_equal(a, b, equal_nan=True)
        a = _np(L.spectrogram(y, kw["n"], nfft=kw.get("nfft")).power)
        b = _np(L.spectrogram(y, kw["n"], nfft=kw.get("nfft")).power)
        assert np.array_equal(a, b)


def test_device_tensors_in_and_out(L):
    import torch
    y = np.random.default_rng(17).standard_normal(20000)
    t = torch.from_numpy(y).cuda()
    S = L.spectrogram(t, 512, 256, window=_hann)
    assert S.power.is_cuda and S.power.dtype == torch.float64 and tuple(S.power.shape) == (257, R.frames(20000, 512, 256))
    _check_power(S.power, R.power(y, 512, 256, 512, window=_hann(512)))
    M = L.melspectrogram(t, 512, 256)
    assert M.power.is_cuda
    C = L.mfcc(t.float(), 512, 256)
    assert C.mfcc.is_cuda and C.mfcc.dtype == torch.float32
    h = L.mfcc(y.astype(np.float32), 512, 256)
    assert np.array_equal(C.mfcc.cpu().numpy(), h.mfcc, equal_nan=True)


@pytest.mark.parametrize("kind", ["power", "mel", "mfcc"])
def test_nan_partner_frame_stays_finite_on_the_bluestein_lds_path(L, kind):
    """nfft = 1009 is Bluestein in LDS: the chirp product mixes the two packed frames, so the flag must come from the samples."""
    n, nov, nfft = 1000, 500, 1009
    y = np.random.default_rng(19).standard_normal(12 * n)
    y[2 * (n - nov) + 10] = np.nan                                   # frames 0, 1 and 2 hold it only if they reach it
    hop = n - nov
    fn = {"power": lambda: L.spectrogram(y, n, nov, nfft=nfft, window=_hann).power,
          "mel": lambda: L.melspectrogram(y, n, nov, nfft=nfft).power,
          "mfcc": lambda: L.mfcc(y, n, nov, nfft=nfft).mfcc}[kind]
    M = _np(fn())
    assert L.stft_last_timing()["path"] == 3
    has = np.array([j * hop <= 2 * hop + 10 < j * hop + n for j in range(M.shape[1])])
    assert has.sum() == 2 and has[1] and has[2]                      # pairs (0, 1), (2, 3): frames 0 and 3 are the clean partners
    assert np.isnan(M[:, has]).all() and np.isfinite(M[:, ~has]).all()
    if kind == "power":
        clean = np.array([j for j in range(M.shape[1]) if not has[j]])
        yc = y.copy(); yc[2 * hop + 10] = 0.0
        _check_power(M[:, clean], R.power(yc, n, nov, nfft, window=_hann(n))[:, clean])


def test_more_frames_than_one_grid_of_workgroups(L):
    """Per-frame kernels stride over the frames: > 65536 frames through the four-step flags and the projection."""
    rng = np.random.default_rng(20)
    n, nov, nfft = 16, 0, 16384                                      # four-step with 2^17 frames of 16 samples
    y = rng.standard_normal(2 ** 21)
    y[70000 * n + 3] = np.nan
    M = _np(L.melspectrogram(y, n, nov, nfft=nfft, nmels=32).power)
    assert L.stft_last_timing()["path"] == 2 and M.shape == (32, 2 ** 17)
    bad = np.zeros(M.shape[1], bool); bad[70000] = True
    assert np.isnan(M[:, bad]).all() and np.isfinite(M[:, ~bad]).all()
    W = L.mel(1, 2 * (nfft // 2 + 1) - 1, nmels=32)
    idx = np.array([0, 1, 65535, 65536, 65537, 69999, 70001, 2 ** 17 - 1])
    Pr = np.concatenate([R.power(y[j * n:(j + 1) * n], n, 0, nfft, window=_hann(n)) for j in idx], axis=1)
    _check_mel(M[:, idx], W, Pr)
    P = np.abs(rng.standard_normal((5, 200000)))                     # melspectrogram(S) of 200000 frames
    S = L.Spectrogram(P, np.arange(5.0), np.arange(200000.0))
    Mp = L.melspectrogram(S, nmels=4)
    _check_mel(Mp.power, L.mel(1, 9, nmels=4), P)
