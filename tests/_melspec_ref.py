"""numpy restatement of DSP.spectrogram (one-sided, real input) and src/mel.jl (mel, dct_matrix, melspectrogram, mfcc) -- what the
GPU tests check the device against.  The power comes from np.fft.fft in float64 on the windowed, zero-padded frames; the filterbank and
the DCT are float32 arithmetic unless Julia's promotion widens them (a Float64 fs widens the FFT grid, a Float64 fmin / fmax the mel
grid); the products sum each band over the bins in ascending order."""
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
