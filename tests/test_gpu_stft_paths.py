"""Every path of the STFT engine (melspec.hip) against the long-double reference of tests/_melspec_ref.py (power_ld) and its per-bin
bound (power_bound): |P̂_k − P_k| <= e·sqrt(P_k·Ptot) + e²·Ptot with e = c·u·log2 N, N the FFT length run and Ptot the frame's own
total power, plus 1 float ulp for f32 outputs.  Mel bands and normalised MFCC columns get the bound carried through (mel_bound,
mfcc_bound).  Every case asserts the path and the FFT length it ran.

c per path (module constant C) is 4x the largest ratio seen on equal-energy white-noise frames over this file's sweeps (the 7-smooth
lengths <= 8192, the tiny lengths, the Bluestein lengths, the four-step splits up to 2^24); observed maxima on one MI355X:
    LDS 3.48 (on the tiny lengths; 1.80 over the 7-smooth sweep), four-step 0.0171, Bluestein in LDS 2.64, Bluestein four-step 0.0614.
Before the quieter frame of each pair was equalised, a frame packed with a partner 1e6 / 1e24 times louder needed c = 39 / 3.5e10
(LDS), 11 / 1.0e10 (four-step), 59 / 5.8e10 (Bluestein in LDS) and 32 / 2.9e10 (Bluestein four-step).
The two largest lengths (3·2^24, 2^26) take numpy's f64 FFT as the reference, whose own error adds C_NP to c."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _melspec_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

C = {1: 14.0, 2: 0.07, 3: 11.0, 4: 0.25}       # paths: 1 LDS (and its fallback), 2 four-step, 3 Bluestein in LDS, 4 Bluestein four-step
C_NP = R.C_NP
SMOOTH = [m for m in range(1, 8193) if R.nextfastfft(m) == m]
OBSERVED = {}                                 # path -> largest c_needed on the calibration sweeps (read by the calibration run)


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def _m(nfft):
    """The Bluestein length the engine runs for a non-smooth nfft (every 7-smooth m <= 2^26 used here has a split)."""
    return R.nextfastfft(2 * nfft - 1)


def stft(L, kind, y, n, nov, nfft, nmels=40, nmfcc=13, window=None, fs=1):
    if kind == "power":
        r = L.spectrogram(y, n, nov, nfft=nfft, fs=fs, window=window).power
    elif kind == "mel":
        r = L.melspectrogram(y, n, nov, nfft=nfft, fs=fs, nmels=nmels, window=window).power
    else:
        r = L.mfcc(y, n, nov, nfft=nfft, fs=fs, nmels=nmels, nmfcc=nmfcc, window=window).mfcc
    return _np(r), L.stft_last_timing()


def _ulp32(x):
    return np.spacing(np.abs(np.nan_to_num(x)).astype(np.float32)).astype(np.float64)


def check(L, kind, y, n, nov, nfft, path, flen, idx=None, nmels=40, nmfcc=13, window=None, fs=1, f32=False, ld=True, nan=None,
          calib=False, B=None):
    """Run `kind` on y (cast to f32 when f32) and check the frames idx (default all) against the reference; `nan` marks the frames
    that must come back NaN.  Returns the device output and the timing."""
    y = np.asarray(y, dtype=np.float32 if f32 else np.float64)
    out, tm = stft(L, kind, y, n, nov, nfft, nmels, nmfcc, window, fs)
    assert (tm["path"], tm["fft_length"]) == (path, flen), tm
    if B is not None:
        assert tm["pairs_per_workgroup"] == B, tm
    k = R.frames(len(y), n, nov)
    assert out.shape[1] == k and out.dtype == (np.float32 if f32 else np.float64)
    idx = np.arange(k) if idx is None else np.asarray(idx)
    wr = None if window is None else np.asarray(window, dtype=np.float32 if f32 else np.float64).astype(np.float64)
    Pr, Pt, re = R.power_ld(y.astype(np.float64), n, nov, nfft, fs=fs, window=wr, idx=idx, ld=ld)
    o = out[:, idx].astype(np.float64)
    bad = np.zeros(len(idx), bool) if nan is None else np.asarray(nan)[idx]
    assert np.isnan(o[:, bad]).all(), "flagged frames must be NaN"
    ok = ~bad
    o, Pr, Pt = o[:, ok], Pr[:, ok], Pt[ok]
    c = C[path] + (0.0 if ld else C_NP)
    pb = R.power_bound(Pr, Pt, flen, c, re)
    if kind == "power":
        assert np.isfinite(o).all()
        err = np.abs(o - Pr)
        cn = R.c_needed(err, Pr, Pt, flen, re, f32)
        if calib:
            OBSERVED[path] = max(OBSERVED.get(path, 0.0), float(cn.max(initial=0.0)))
        assert (err <= pb + (_ulp32(Pr) if f32 else 0)).all(), f"{kind} nfft {nfft}: c needed {cn.max():.3g} > {c}"
        return out, tm
    W = L.mel(fs, 2 * (nfft // 2 + 1) - 1, nmels=nmels)
    Mr = R.project(W, Pr)
    mb = R.mel_bound(W, Pr, pb)
    if kind == "mel":
        assert np.isfinite(o).all()
        err = np.abs(o - Mr)
        assert (err <= mb + (_ulp32(Mr) if f32 else 0)).all(), f"mel nfft {nfft}: max err / bound {np.max(err / np.maximum(mb, 1e-300)):.3g}"
        return out, tm
    D = L.dct_matrix(nmfcc, nmels)
    Cr = R.mfcc_from_mel(D, Mr)
    cnan = np.isnan(Cr)
    assert (np.isnan(o) == cnan).all(), "MFCC: NaN columns differ from the reference (0/0 of a zero column)"
    cb = np.broadcast_to(R.mfcc_bound(D, Mr, mb), Cr.shape) + (_ulp32(Cr) if f32 else 0)
    err = np.abs(o - Cr)[~cnan]
    assert (err <= cb[~cnan]).all(), f"mfcc nfft {nfft}: max err / bound {np.max(err / cb[~cnan]):.3g}"
    return out, tm


def _noise(seed, size):
    return np.random.default_rng(seed).standard_normal(size)


# ---- 1. every 7-smooth nfft <= 8192 in LDS ---------------------------------------------------------------------------------------------
def test_every_smooth_lds_length(L):
    assert len(SMOOTH) == 317
    for j, nfft in enumerate(SMOOTH):
        y = _noise(nfft, 3 * nfft)                                    # 3 frames: the second pair has no partner
        check(L, "power", y, nfft, 0, nfft, 1, nfft, calib=True, B=min(8192 // nfft, 512, 2))
        if j % 9 == 0:                                                # zero padding, odd n
            n = max(1, (2 * nfft) // 3)
            check(L, "power", _noise(nfft + 1, 3 * n + 5), n, n // 4, nfft, 1, nfft, calib=True)
        if j % 11 == 0:
            check(L, "power", y, nfft, 0, nfft, 1, nfft, f32=True)


# ---- 2. tiny lengths, B = 512 pairs per workgroup --------------------------------------------------------------------------------------
def test_tiny_lengths_and_pairs_per_workgroup(L):
    for nfft in range(1, 17):
        for n in range(1, nfft + 1):
            for k in ((1023, 1024, 1025) if n == nfft else ((1023, 1024, 1025)[(nfft + n) % 3],)):
                nov = n // 3
                y = _noise(100 * nfft + n, n + (k - 1) * (n - nov))
                assert R.frames(len(y), n, nov) == k
                flen = nfft if R.nextfastfft(nfft) == nfft else _m(nfft)   # 11 and 13 run Bluestein in LDS
                check(L, "power", y, n, nov, nfft, 1 if flen == nfft else 3, flen, calib=True,
                      B=min(8192 // flen, 512, (k + 1) // 2))


# ---- 3. Bluestein in LDS ---------------------------------------------------------------------------------------------------------------
def test_bluestein_lds(L):
    lengths = [m for m in range(1, 301) if R.nextfastfft(m) != m] + [4093]
    assert _m(4093) == 8192
    for j, nfft in enumerate(lengths):
        y = _noise(nfft, 5 * nfft)
        m = _m(nfft)
        _, tm = check(L, "power", y, nfft, 0, nfft, 3, m, calib=True)
        assert tm["pairs_per_workgroup"] == min(8192 // m, 3) and (nfft == 4093 or tm["pairs_per_workgroup"] > 1)
        if j % 16 == 0 or nfft == 4093:
            check(L, "mel", y, nfft, 0, nfft, 3, m, nmels=16)
            check(L, "mfcc", y, nfft, 0, nfft, 3, m, nmels=16, nmfcc=7)


# ---- 4. Bluestein on the four-step from small nfft --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft,m", [(4099, 8232), (8191, 16384)])
def test_bluestein_four_step_small_nfft(L, nfft, m):
    y = _noise(nfft, 5 * nfft)
    check(L, "power", y, nfft, 0, nfft, 4, m, calib=True)
    check(L, "mel", y, nfft, 0, nfft, 4, m)
    check(L, "mfcc", y, nfft, 0, nfft, 4, m)


# ---- 5. four-step splits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfft", [16384, 73728, 59049, 33614, 78125, 57344])
def test_four_step_splits_all_kinds(L, nfft):
    y = _noise(nfft, 3 * nfft)
    check(L, "power", y, nfft, 0, nfft, 2, nfft, calib=True)
    w = L.hanning(nfft)
    check(L, "power", y, nfft, nfft // 2, nfft, 2, nfft, window=w, calib=True)
    check(L, "mel", y, nfft, 0, nfft, 2, nfft)
    check(L, "mfcc", y, nfft, 0, nfft, 2, nfft, window=w)


@pytest.mark.parametrize("nfft,ld", [(2 ** 24, True), (3 * 2 ** 24, False), (2 ** 26, False)])
def test_four_step_largest_splits(L, nfft, ld):
    """4096·4096, 6144·8192 (1.6 GB of scratch for its one pair) and 8192·8192: one frame pair each."""
    check(L, "power", _noise(nfft, 2 * nfft), nfft, 0, nfft, 2, nfft, ld=ld, calib=ld)


# ---- 6. the LDS fallback through global power columns ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nfft,nmels,nmfcc,path,flen", [
    ("mel", 8192, 4096, 0, 1, 8192),
    ("mfcc", 8000, 4000, 200, 1, 8000),
    ("mel", 4093, 6200, 0, 3, 8192),
    ("mfcc", 64, 16000, 384, 1, 64),                                  # nmels + nmfcc = 16384: 128 KiB of epilogue LDS
    ("mel", 64, 24000, 0, 1, 64),                                     # more bands than the epilogue's LDS could hold
])
def test_lds_fallback(L, kind, nfft, nmels, nmfcc, path, flen):
    y = _noise(nfft + nmels, 5 * nfft)
    nan = None
    if kind == "mel" and nfft == 8192:                                # a NaN frame: its partner stays clean
        y[2 * nfft + 17] = np.nan
        nan = np.arange(5) == 2
    check(L, kind, y, nfft, 0, nfft, path, flen, nmels=nmels, nmfcc=max(nmfcc, 1), nan=nan, B=0)


# ---- 7. FFT launches cut at 2^20 workgroups ----------------------------------------------------------------------------------------
def test_launch_split_beyond_2_20_workgroups(L):
    nfft = n = 4374                                                   # 2·3^7: radix 2 first, one pair per workgroup
    k = 2 ** 21 + 5                                                   # 2^20 + 3 pairs: two launches
    y = _noise(4374, n + k - 1)
    idx = np.r_[np.arange(2 ** 21 - 4, 2 ** 21 + 5), k - 1]
    check(L, "mel", y, n, n - 1, nfft, 1, nfft, idx=idx, nmels=4, B=1)


# ---- 8. four-step chunk boundaries ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["power", "mfcc"])
def test_four_step_chunk_boundaries(L, kind):
    nfft, n, nov, k = 16384, 16, 0, 4100                              # 2048 pairs per chunk: frames 0 .. 4095, 4096 .. 4099
    y = _noise(21, n * k)
    y[4096 * 16 + 5] = np.nan                                         # only in frame 4096, the first of the second chunk
    nan = np.arange(k) == 4096
    idx = np.r_[0, 1, 4093:4100]
    check(L, kind, y, n, nov, nfft, 2, nfft, idx=idx, nan=nan)


def test_bluestein_four_step_chunk_boundary(L):
    nfft = n = 4099                                                   # m = 8232: 4076 pairs, frames 0 .. 8151 in the first chunk
    k = 8200
    y = _noise(22, n + k - 1)
    idx = np.r_[0, 8149:8156, k - 1]
    check(L, "power", y, n, n - 1, nfft, 4, 8232, idx=idx)


# ---- 9. a frame's error does not depend on its partner ---------------------------------------------------------------------------------
PARTNER_CASES = [("power", 1024, 0, 1, 1024), ("power", 16384, 0, 2, 16384), ("power", 1009, 0, 3, 2025),
                 ("power", 4099, 0, 4, 8232), ("mel", 512, 8000, 1, 512)]


@pytest.mark.parametrize("kind,nfft,nmels,path,flen", PARTNER_CASES)
def test_partner_energy_independence(L, kind, nfft, nmels, path, flen):
    rng = np.random.default_rng(nfft)
    B = 0 if nmels == 8000 else None
    for ratio in (1.0, 1e6, 1e12, 1e24):
        for loud_first in (False, True):
            a, b = rng.standard_normal(nfft), rng.standard_normal(nfft) * np.sqrt(ratio)
            y = np.concatenate([b, a] if loud_first else [a, b])
            check(L, kind, y, nfft, 0, nfft, path, flen, nmels=max(nmels, 40), B=B)
    for zero_first in (False, True):                                  # an all-zero frame: exactly 0 power and mel, NaN MFCC
        a, b = np.zeros(nfft), rng.standard_normal(nfft) * 1e3
        y = np.concatenate([a, b] if zero_first else [b, a])
        z = 0 if zero_first else 1
        out, _ = check(L, kind, y, nfft, 0, nfft, path, flen, nmels=max(nmels, 40), B=B)
        assert (out[:, z] == 0).all()
        C_, tm = stft(L, "mfcc", y, nfft, 0, nfft, nmels=max(nmels, 40))
        assert tm["path"] == path and np.isnan(C_[:, z]).all() and np.isfinite(C_[:, 1 - z]).all()


@pytest.mark.parametrize("kind", ["mel", "mfcc"])
def test_noise_onset_after_silence(L, kind):
    n = 400
    y = np.concatenate([np.zeros(4000), 1e-5 * _noise(23, 4000)])
    w = L.hanning(n)
    out, _ = check(L, kind, y, n, n // 2, n, 1, n, window=w, nmels=128, nmfcc=20)
    silent = np.array([j * (n // 2) + n <= 4000 for j in range(out.shape[1])])
    assert silent.sum() >= 9
    if kind == "mfcc":
        assert np.isnan(out[:, silent]).all() and np.isfinite(out[:, ~silent]).all()
    else:
        assert (out[:, silent] == 0).all() and (out[:, ~silent] > 0).any(axis=0).all()


# ---- 10. power-of-two equivariance, bitwise --------------------------------------------------------------------------------------------
EQUI_CASES = [(1000, 0, 1, False), (16384, 0, 2, False), (1009, 0, 3, False), (4099, 0, 4, False), (512, 8000, 1, True)]


@pytest.mark.parametrize("nfft,nmels,path,fallback", EQUI_CASES)
@pytest.mark.parametrize("f32", [False, True])
def test_power_of_two_equivariance(L, nfft, nmels, path, fallback, f32):
    dt = np.float32 if f32 else np.float64
    y = _noise(nfft + 5, 3 * nfft + 7).astype(dt)
    w = L.hanning(nfft).astype(dt)
    nm = max(nmels, 40)
    P0 = stft(L, "power", y, nfft, nfft // 3, nfft, window=w)[0]
    M0, tm = stft(L, "mel", y, nfft, nfft // 3, nfft, nmels=nm, window=w)
    assert tm["path"] == path and (tm["pairs_per_workgroup"] == 0) == fallback
    C0 = stft(L, "mfcc", y, nfft, nfft // 3, nfft, nmels=nm, window=w)[0]
    assert np.isfinite(P0).all() and np.isfinite(M0).all() and np.isfinite(C0).all()
    for s in (-40, 17):
        ys = np.ldexp(y, s).astype(dt)
        assert np.array_equal(stft(L, "power", ys, nfft, nfft // 3, nfft, window=w)[0], np.ldexp(P0, 2 * s))
        assert np.array_equal(stft(L, "mel", ys, nfft, nfft // 3, nfft, nmels=nm, window=w)[0], np.ldexp(M0, 2 * s))
        assert np.array_equal(stft(L, "mfcc", ys, nfft, nfft // 3, nfft, nmels=nm, window=w)[0], C0)
        ws = np.ldexp(w, s).astype(dt)
        assert np.array_equal(stft(L, "power", y, nfft, nfft // 3, nfft, window=ws)[0], P0)
        assert np.array_equal(stft(L, "power", y, nfft, nfft // 3, nfft, window=w, fs=2.0 ** s)[0], np.ldexp(P0, -s))
