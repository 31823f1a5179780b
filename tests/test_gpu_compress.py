"""compress (src/plotting.jl:38-47) and heatmap (the numbers of plot_spectrogram and of the MelSpectrogram recipe) on the device.

compress without the log: the thresholds must EQUAL those of numpy.sort plus Julia's quantile formula in Python floats (the radix select
is exact and the interpolation is the same handful of f64 operations, contraction off), the output must equal numpy.clip with them.

heatmap: reference = long-double power -> log -> thresholds -> clip.  Order statistics are 1-Lipschitz in the sup norm, so every element
and both thresholds get the one tolerance τ = max over frames and bins k >= 1 of power_bound(P_fk, ...)/P_fk + 4u·|log P_fk|; the tests
assert τ < 1e-8 for the reference alone, so that τ cannot hide anything (mel_bound in place of power_bound for a MelSpectrogram)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _melspec_ref as R  # noqa: E402
import _welch_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu
U = R.U
C_LDS = 14.0                                    # tests/test_gpu_stft_paths.py: power_bound's constant of the LDS path


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def check(L, x, q):
    """compress(x, q) on the device == the sorted reference: thresholds equal, output equal to numpy.clip.  Returns the timing."""
    out, th = L.compress_thresholds(x, q)
    tm = L.compress_last_timing()
    ref, thr = WR.compress_ref(_np(x), q)
    print(f"compress {tuple(_np(x).shape)} q={q}: thresholds {th} (reference {thr}), {tm}")
    assert th[0] == thr[0] and th[1] == thr[1], (th, thr)
    o = _np(out)
    assert o.dtype == ref.dtype and o.shape == ref.shape and np.array_equal(o, ref)
    assert np.array_equal(_np(L.compress(x, q)), ref)
    return tm


def test_normals_2_24(L):
    x = np.random.default_rng(0).standard_normal((4096, 4096))
    tm = check(L, x, (0.005, 1))
    assert tm["passes"] + tm["digits_skipped"] == 8
    check(L, x, 0.37)
    check(L, x.astype(np.float32), (0.005, 0.995))                    # the f32 twin: float order statistics, the low key digits are skipped
    assert L.compress_last_timing()["digits_skipped"] >= 3


def test_ties_across_every_rank(L):
    x = np.round(np.random.default_rng(1).standard_normal((1000, 333)) * 4) / 4
    x = np.clip(x, -1.75, 2.0)                                        # 16 levels
    assert len(np.unique(x)) == 16
    for q in (0.005, 0.25, (0.5, 0.5), (0.1, 0.9), (0, 1)):
        tm = check(L, x, q)
        assert tm["digits_skipped"] > 0
    tm = check(L, np.full((37, 41), 3.25), 0.1)                       # a constant matrix: one pass, the rest is read off
    assert tm["passes"] == 1 and tm["digits_skipped"] == 7


def test_infinities(L):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((80, 50))                                 # m = 4000
    x[rng.random(x.shape) < 0.01] = np.inf
    x[rng.random(x.shape) < 0.01] = -np.inf
    check(L, x, (0.1, 0.9))                                           # both quantiles inside the finite range
    y = rng.standard_normal((80, 50))
    y.ravel()[rng.permutation(4000)[:400]] = -np.inf                  # a tenth is -Inf: p = 0.05 has aleph = 200.95, both neighbours -Inf
    out, th = L.compress_thresholds(y, (0.05, 0.9))
    assert th[0] == -np.inf and np.isfinite(th[1])
    check(L, y, (0.05, 0.9))


def test_signed_zeros(L):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((64, 64))
    x[rng.random(x.shape) < 0.6] = 0.0
    x[rng.random(x.shape) < 0.3] *= -1.0                              # -0.0 and +0.0 mixed
    assert np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any()
    for q in (0.2, 0.45, (0.3, 0.6)):
        check(L, x, q)
    check(L, np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0]), (0.2, 0.7))


@pytest.mark.parametrize("m", [1, 2, 3])
def test_tiny(L, m):
    x = np.array([0.3, -1.2, 7.0])[:m]
    for q in (0, 0.25, 0.5, 1, (0.2, 0.7), (1, 0)):
        check(L, x, q)
        check(L, x.reshape(1, m), q)
        check(L, x.reshape(m, 1).astype(np.float32), q)


def test_strided_submatrix_is_read_in_place(L):
    import torch
    rng = np.random.default_rng(4)
    X = np.asfortranarray(rng.standard_normal((301, 200)))
    X[0, :100] = 1e6                                                  # row 0 holds the extremes: reading it would move both thresholds
    X[0, 100:] = -1e6
    sub = X[1:, :]
    assert sub.strides == (8, 8 * 301)
    check(L, sub, (0, 1))
    check(L, sub, 0.01)
    t = torch.as_tensor(np.ascontiguousarray(X.T)).cuda().T           # device tensor, column-major, ld = 301
    out, th = L.compress_thresholds(t[1:, :], (0, 1))
    assert out.is_cuda and th == (sub.min(), sub.max()) and np.array_equal(_np(out), sub)
    check(L, t[1:, :], 0.01)
    check(L, torch.as_tensor(np.ascontiguousarray(X)).cuda()[1:, :], 0.01)   # row-major device tensor: copied to column-major first
    check(L, np.ascontiguousarray(X)[1:, ::2], 0.2)                   # any host view


def test_number_and_reversed_pair(L):
    x = np.random.default_rng(5).standard_normal((50, 60))
    a, ta = L.compress_thresholds(x, 0.8)                             # 0.8 -> (0.2, 0.8) up to 1 - (1 - 0.8)
    b, tb = L.compress_thresholds(x, (1 - (1 - 0.8), 1 - 0.8))        # reversed pair
    assert ta == tb and np.array_equal(a, b)
    check(L, x, 0.8)
    check(L, x, (0.9, 0.1))
    check(L, x, (0, 1))
    assert np.array_equal(L.compress(x, (0, 1)), x)


def test_nan_and_empty_raise(L):
    x = np.random.default_rng(6).standard_normal((20, 20))
    x[3, 4] = np.nan
    with pytest.raises(L.DomainError):
        L.compress(x, 0.1)
    with pytest.raises(L.DomainError):
        L.compress(np.zeros((0, 4)), 0.1)
    with pytest.raises(ValueError):
        L.compress(np.zeros((3, 4)), 1.5)
    y = np.random.default_rng(7).standard_normal(4000)
    y[2345] = np.nan
    S = L.spectrogram(y, 400, 200)
    with pytest.raises(L.DomainError):
        L.heatmap(S)


# ---- heatmap -----------------------------------------------------------------------------------------------------------------------------
def _signal(seed, L_):
    t = np.arange(L_)
    return np.random.default_rng(seed).standard_normal(L_) + 3 * np.sin(2 * np.pi * 0.1234 * t)


def _heat_ref(logP, compression):
    lo, hi = WR.quantile_pair(compression)
    v = np.sort(logP.ravel())
    t0, t1 = WR.quantile7(v, lo), WR.quantile7(v, hi)
    return np.clip(logP, t0, t1), (t0, t1)


def _check_heat(z, th, logP, tau, compression):
    ref, thr = _heat_ref(logP, compression)
    fin = np.isfinite(ref)
    assert np.array_equal(z[~fin], ref[~fin])                          # -Inf survives (==)
    err = np.abs(z[fin] - ref[fin])
    print(f"heatmap: tau {tau:.3g}, max err {err.max():.3g}, thresholds {th} (reference {thr})")
    assert tau < 1e-8 and (err <= tau).all()
    assert all(a == b or abs(a - b) <= tau for a, b in zip(th, thr))


@pytest.mark.parametrize("dev", [False, True])
def test_heatmap_spectrogram(L, dev):
    n, nov = 1024, 512
    y = _signal(8, 2 ** 20)
    w = L.hanning(n)
    ys = y
    if dev:
        import torch
        ys = torch.as_tensor(y).cuda()
    S = L.spectrogram(ys, n, nov, window=w)
    tm, fr, z = L.heatmap(S)
    assert getattr(z, "is_cuda", False) == dev
    z = _np(z)
    Pr, Pt, re = R.power_ld(y, n, nov, n, window=w)
    P1 = Pr[1:, :]
    tau = float(np.max(R.power_bound(P1, Pt[None, :], n, C_LDS, re) / P1 + 4 * U * np.abs(np.log(P1))))
    assert z.shape == P1.shape and np.array_equal(fr, _np(S.freq)[1:]) and np.array_equal(tm, S.time)
    _, th = L.compress_thresholds(S.power[1:, :], (0.005, 1), take_log=True)
    _check_heat(z, th, np.log(P1), tau, (0.005, 1))
    assert L.compress_last_timing()["passes"] <= 8


def test_heatmap_melspectrogram(L):
    n, nov, nmels = 1024, 512, 40
    y = _signal(9, 2 ** 18)
    w = L.hanning(n)
    M = L.melspectrogram(y, n, nov, nmels=nmels, window=w)
    tm, fr, z = L.heatmap(M, compression=(0.01, 0.99))
    Pr, Pt, re = R.power_ld(y, n, nov, n, window=w)
    W = L.mel(1, 2 * (n // 2 + 1) - 1, nmels=nmels)
    Mr = R.project(W, Pr)
    mb = R.mel_bound(W, Pr, R.power_bound(Pr, Pt[None, :], n, C_LDS, re))
    M1 = Mr[1:, :]
    tau = float(np.max(mb[1:, :] / M1 + 4 * U * np.abs(np.log(M1))))
    assert z.shape == M1.shape and np.array_equal(fr, L.mel_to_hz(M.mels)[1:])
    _, th = L.compress_thresholds(M.power[1:, :], (0.01, 0.99), take_log=True)
    _check_heat(_np(z), th, np.log(M1), tau, (0.01, 0.99))


def test_heatmap_keeps_minus_infinity(L):
    n, nov = 1024, 512
    y = _signal(10, 2 ** 19)
    y[100 * 512: 100 * 512 + 1024] = 0.0                               # frame 100 is all zero: a column of -Inf
    w = L.hanning(n)
    S = L.spectrogram(y, n, nov, window=w)
    _, _, z = L.heatmap(S)
    Pr, Pt, re = R.power_ld(y, n, nov, n, window=w)
    P1 = Pr[1:, :]
    assert (P1[:, 100] == 0).all() and (np.delete(P1, 100, axis=1) > 0).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        logP = np.log(P1)
        t = R.power_bound(P1, Pt[None, :], n, C_LDS, re) / P1 + 4 * U * np.abs(logP)
    tau = float(np.max(t[np.isfinite(logP)]))
    _, th = L.compress_thresholds(S.power[1:, :], (0.005, 1), take_log=True)
    _check_heat(z, th, logP, tau, (0.005, 1))                          # 512 of 523776 values are -Inf: the lower threshold is finite
    assert np.isfinite(th[0]) and (z[:, 100] == th[0]).all()
    _, _, z = L.heatmap(S, compression=(0.0004, 1))                    # aleph = 210.5: both neighbours -Inf, the column survives
    _, th = L.compress_thresholds(S.power[1:, :], (0.0004, 1), take_log=True)
    assert th[0] == -np.inf and (z[:, 100] == -np.inf).all()
    _check_heat(z, th, logP, tau, (0.0004, 1))
