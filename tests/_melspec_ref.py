"""numpy restatement of DSP.spectrogram (one-sided, real input) and src/mel.jl (mel, dct_matrix, melspectrogram, mfcc) -- what the
GPU tests check the device against.  The power comes from np.fft.fft in float64 on the windowed, zero-padded frames; the filterbank and
the DCT are float32 arithmetic unless Julia's promotion widens them (a Float64 fs widens the FFT grid, a Float64 fmin / fmax the mel
grid); the products sum each band over the bins in ascending order.

power_ld is the sharper reference the STFT path tests use: the same power from a long-double FFT, with the per-bin bound power_bound
(module constants below, calibrated on the device by tests/test_gpu_stft_paths.py)."""
import numpy as np


def nextfastfft(n):
    m = max(int(n), 1)
    while True:
        k = m
        for p in (2, 3, 5, 7):
            while k % p == 0:
                k //= p
        if k == 1:
            return m
        m += 1


def frames(L, n, noverlap):
    return (L - n) // (n - noverlap) + 1 if L >= n else 0


def power(s, n, noverlap, nfft, fs=1, window=None):
    """(nfft÷2+1) × k one-sided power, float64."""
    s = np.asarray(s, dtype=np.float64)
    k = frames(len(s), n, noverlap)
    nb = nfft // 2 + 1
    win = np.ones(n) if window is None else np.asarray(window, dtype=np.float64)
    norm2 = float(n) if window is None else float(np.sum(win * win))
    r = fs * norm2
    m1, m2 = 1.0 / r, 2.0 / r
    P = np.empty((nb, k))
    hop = n - noverlap
    for j in range(k):
        x = np.zeros(nfft)
        x[:n] = s[j * hop: j * hop + n] * win
        a = np.abs(np.fft.fft(x)[:nb]) ** 2
        sc = np.full(nb, m2)
        sc[0] = m1
        if nb > 1:
            sc[-1] = m2 if nfft % 2 else m1
        P[:, j] = a * sc
    return P


def _wide(x):
    return isinstance(x, (float, np.floating)) and not isinstance(x, (np.float32, np.float16))


def _consts():
    f_sp = np.float32(200) / np.float32(3)
    min_log_hz = np.float32(1000)
    return f_sp, min_log_hz, min_log_hz / f_sp, np.float32(np.log(np.float64(np.float32(6.4)))) / np.float32(27)


def hz_to_mel(f, dt):
    f_sp, min_log_hz, min_log_mel, logstep = _consts()
    f = dt(f)
    m = (f - dt(0)) / dt(f_sp)
    if f >= min_log_hz:
        m = dt(min_log_mel) + dt(np.log(np.float64(f / dt(min_log_hz)))) / dt(logstep)
    return dt(m)


def mel_to_hz(m, dt):
    f_sp, min_log_hz, min_log_mel, logstep = _consts()
    m = dt(m)
    f = dt(0) + dt(f_sp) * m
    if m >= min_log_mel:
        f = dt(min_log_hz) * dt(np.exp(np.float64(dt(logstep) * (m - dt(min_log_mel)))))
    return dt(f)


def mel(fs, nfft, nmels=128, fmin=np.float32(0), fmax=None):
    if fmax is None:
        fmax = float(fs) / 2 if _wide(fs) else np.float32(np.float32(fs) / np.float32(2))
    F = np.float64 if _wide(fs) else np.float32
    G = np.float64 if (_wide(fmin) or _wide(fmax)) else np.float32
    P = np.float64 if (F is np.float64 or G is np.float64) else np.float32
    nb = (nfft >> 1) + 1
    stop = F(F(fs) / F(2))
    t = np.arange(nb) / max(nb - 1, 1)
    ff = (t * np.float64(stop)).astype(F).astype(P)
    lo, hi = hz_to_mel(fmin, G), hz_to_mel(fmax, G)
    nm = nmels + 2
    tt = np.arange(nm) / max(nm - 1, 1)
    mg = ((1 - tt) * np.float64(lo) + tt * np.float64(hi)).astype(G)
    mf = np.array([mel_to_hz(v, G) for v in mg], dtype=G)
    W = np.zeros((nmels, nb), dtype=np.float32)
    with np.errstate(all="ignore"):
        for i in range(nmels):
            enorm = G(2) / (mf[i + 2] - mf[i])
            lower = (ff - P(mf[i])) / P(mf[i + 1] - mf[i])
            upper = (P(mf[i + 2]) - ff) / P(mf[i + 2] - mf[i + 1])
            W[i] = (np.maximum(P(0), np.minimum(lower, upper)) * P(enorm)).astype(np.float32)
    return W


def dct_matrix(nfilters, ninput):
    j = np.arange(ninput)
    smp = (2 * j + 1).astype(np.float32) * np.float32(np.pi) / np.float32(2 * ninput)
    D = np.empty((nfilters, ninput), dtype=np.float32)
    for i in range(1, nfilters + 1):
        D[i - 1] = np.cos(np.float32(i) * smp)
    return D * np.float32(np.sqrt(np.float32(2) / np.float32(ninput)))


def project(W, P):
    """W (float32) times P (float64), every band summed over its bins in ascending order; a frame with non-finite power is NaN."""
    W64 = W.astype(np.float64)
    out = np.zeros((W.shape[0], P.shape[1]))
    for k in range(W.shape[1]):
        out = out + W64[:, k:k + 1] * np.where(np.isfinite(P[k:k + 1]), P[k:k + 1], 0.0)
    bad = ~np.all(np.isfinite(P), axis=0)
    out[:, bad] = np.nan
    return out


def mfcc_from_mel(D, M):
    c = D.astype(np.float64) @ M
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / np.linalg.norm(c, axis=0, keepdims=True)


# ---- the long-double reference and its per-bin bound --------------------------------------------------------------------------------
U = 2.0 ** -53          # f64 unit roundoff
C_NP = 0.03             # numpy's f64 FFT against power_ld at lengths >= 2^16: 4x its largest ratio (0.0066 at 2^16; host self-test)


def _frame_matrix(s, n, noverlap, nfft, win, idx, dt):
    hop = n - noverlap
    X = np.zeros((len(idx), nfft), dtype=dt)
    for r, j in enumerate(idx):
        X[r, :n] = s[j * hop: j * hop + n].astype(dt) * win
    return X


def power_ld(s, n, noverlap, nfft, fs=1, window=None, idx=None, ld=True):
    """One-sided power of the frames `idx` (default: all) from an FFT in long double: the frames are windowed and zero-padded in
    np.longdouble, transformed by scipy.fft.fft (complex256) and scaled by m1 / m2 in long double.  Returns (P, Ptot, r_err) in float64:
    P is (nfft÷2+1) × len(idx), Ptot each frame's total power (the sum of its column), r_err the relative rounding of the f64 sum
    r = fs·Σ win² taken in sample order, the scale the device documents (it is not an FFT error: power_bound adds r_err·P_k).  With
    ld=False the FFT is numpy's f64 one (for lengths where a long-double FFT is too slow; its own error then counts against the bound)."""
    import scipy.fft
    dt = np.longdouble if ld else np.float64
    s = np.asarray(s, dtype=np.float64)
    k = frames(len(s), n, noverlap)
    idx = np.arange(k) if idx is None else np.asarray(idx, dtype=np.int64)
    nb = nfft // 2 + 1
    w64 = np.ones(n) if window is None else np.asarray(window, dtype=np.float64)
    win = w64.astype(dt)
    r = dt(fs) * (dt(n) if window is None else np.sum(win * win))
    r64 = fs * (float(n) if window is None else float(np.add.accumulate(w64 * w64)[-1]))
    r_err = abs(float((dt(r64) - r) / r)) if r != 0 else 0.0
    sc = np.full(nb, dt(2) / r)
    sc[0] = dt(1) / r
    if nb > 1 and nfft % 2 == 0:
        sc[-1] = dt(1) / r
    P = np.empty((nb, len(idx)))
    per = max(1, (1 << 22) // max(nfft, 1))                     # frames per batch: bounds the long-double working set
    for b0 in range(0, len(idx), per):
        X = scipy.fft.fft(_frame_matrix(s, n, noverlap, nfft, win, idx[b0:b0 + per], dt), axis=1, workers=-1)[:, :nb]
        P[:, b0:b0 + per] = ((X.real * X.real + X.imag * X.imag) * sc).T.astype(np.float64)
    return P, P.sum(axis=0), r_err


def _lg(N):
    return max(float(np.log2(max(int(N), 2))), 1.0)


def power_bound(P, Ptot, N, c, r_err=0.0, f32=False):
    """Per-bin bound |P̂_k − P_k| <= e·sqrt(P_k·Ptot) + e²·Ptot + r_err·P_k, e = c·u·log2 N (the normwise FFT error, |X̂ − X| <= e·‖X‖,
    squared through |X|²), plus 1 float ulp of P_k for the f32 outputs.  Only the frame's own energy enters."""
    e = c * U * _lg(N)
    b = e * np.sqrt(P * Ptot) + e * e * Ptot + r_err * np.abs(P)
    return b + (np.spacing(np.abs(P).astype(np.float32)).astype(np.float64) if f32 else 0.0)


def c_needed(err, P, Ptot, N, r_err=0.0, f32=False):
    """The smallest c with err <= power_bound(P, Ptot, N, c, ...) per bin (0 where err is within the c-free terms)."""
    rest = np.maximum(np.abs(err) - power_bound(P, Ptot, N, 0.0, r_err, f32), 0.0)
    a = U * _lg(N) * np.sqrt(P * Ptot)
    b = (U * _lg(N)) ** 2 * Ptot
    with np.errstate(invalid="ignore", divide="ignore"):
        c = 2 * rest / (a + np.sqrt(a * a + 4 * b * rest))
    return np.where(rest > 0, c, 0.0)


def _gamma(m):
    return m * U / (1 - m * U)


def mel_bound(W, Pr, bound):
    """Mel band i: Σ_k W_ik·bound_k plus the rounding of the band sum on either side (each sums its nnz_i products in bin order)."""
    W64 = W.astype(np.float64)
    nnz = np.count_nonzero(W, axis=1)[:, None]
    return W64 @ bound + 2 * _gamma(nnz + 1) * (W64 @ np.where(np.isfinite(Pr), np.abs(Pr), 0.0))


def mfcc_bound(D, Mr, mbound):
    """Normalised MFCC column c/‖c‖: 2‖δc‖/‖c‖ (‖a/|a| − b/|b|‖ <= 2‖a − b‖/|b|) with δc_j = Σ_i |D_ji|·mbound_i plus the rounding
    of the DCT sums on either side, and 8 u for the norm and the division."""
    D64 = np.abs(D.astype(np.float64))
    dc = D64 @ mbound + 2 * _gamma(D.shape[1] + 1) * (D64 @ np.abs(Mr))
    c = D.astype(np.float64) @ Mr
    with np.errstate(invalid="ignore", divide="ignore"):
        return 2 * np.linalg.norm(dc, axis=0, keepdims=True) / np.linalg.norm(c, axis=0, keepdims=True) + 8 * U
