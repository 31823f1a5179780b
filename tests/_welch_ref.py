"""References for welch_pgram / periodogram / compress / heatmap -- what tests/test_gpu_welch.py and tests/test_gpu_compress.py check the
device against.

welch_ld: the mean over the frames of power_ld (tests/_melspec_ref.py: long-double FFT), taken in long double.
welch_bound: (1/K) Σ_f power_bound(P_fk, Ptot_f, N, c, r_err) + (D + 2)·u·S_k -- the FFT's per-bin bound averaged, plus D dependent
additions, the division by K and the rounding of the reference's columns to float64.
sum_chain: D from the frame count and the plan, the formula of DESIGN.md §4.10.
quantile7 / compress_ref: Julia's default quantile on a sorted copy and the clamp, in Python floats."""
import numpy as np

import _melspec_ref as R

U = R.U
SCRATCH_BUDGET = 1 << 30      # bytes of four-step scratch per chunk of frame pairs (32 bytes per pair and FFT point)
CHAIN, SLABS, CHUNK_FRAMES = 1024, 1024, 256


def _cdiv(a, b):
    return -(-a // b)


def sum_chain(K, path, B, flen):
    """(D, S): the longest chain of dependent additions behind one bin and the number of slabs, DESIGN.md §4.10.
    LDS paths (1, 3), B frame pairs per workgroup: nbatch = ceil(ceil(K/2) / B) batches, S = max(min(nbatch, 1024), ceil(nbatch /
    max(1, 1024 ÷ 2B))) slabs, slab g adds the batches g, g + S, ...: F = ceil(nbatch/S)·2B frames, less the 2B·nbatch − K frames the
    last batch lacks when slab 0 holds it.  Four-step paths (2, 4): chunks of cp = max(1, min(pairs, 2^30 ÷ 32·flen)) pairs, each cut in
    slabs of 256 frames.  D = F − 1 + ceil(log2 S)."""
    npair = (K + 1) // 2
    if path in (1, 3):
        nbatch = _cdiv(npair, B)
        bpw = max(1, CHAIN // (2 * B))
        S = max(min(nbatch, SLABS), _cdiv(nbatch, bpw))
        F = _cdiv(nbatch, S) * 2 * B - ((2 * B * nbatch - K) if (nbatch - 1) % S == 0 else 0)
    else:
        cp = max(1, min(npair, SCRATCH_BUDGET // (32 * flen)))
        S = F = 0
        for p0 in range(0, npair, cp):
            nfr = min(2 * min(cp, npair - p0), K - 2 * p0)
            S += _cdiv(nfr, CHUNK_FRAMES)
            F = max(F, min(nfr, CHUNK_FRAMES))
    return F - 1 + (S - 1).bit_length(), S


def welch_ld(s, n, noverlap, nfft, fs=1, window=None):
    """(S, bound_fft(c), K): S the long-double mean of power_ld's columns (float64), bound_fft(c) the averaged per-bin FFT bound for the
    path constant c and FFT length N as a function."""
    P, Pt, re = R.power_ld(s, n, noverlap, nfft, fs=fs, window=window)
    K = P.shape[1]
    S = (P.astype(np.longdouble).sum(axis=1) / np.longdouble(K)).astype(np.float64)

    def bound_fft(c, N):
        return R.power_bound(P, Pt, N, c, re).astype(np.longdouble).sum(axis=1).astype(np.float64) / K
    return S, bound_fft, K


def welch_bound(S, bound_fft, c, N, D, f32=False):
    b = bound_fft(c, N) + (D + 2) * U * np.abs(S)
    return b + (np.spacing(np.abs(S).astype(np.float32)).astype(np.float64) if f32 else 0.0)


def twosided(S1, nfft):
    """The two-sided spectrum of a real signal from the one-sided one: interior bins halved and mirrored."""
    nb = nfft // 2 + 1
    out = np.empty(nfft, dtype=S1.dtype)
    out[:nb] = S1
    hi = nb - 1 if nfft % 2 == 0 else nb                       # interior bins 1 .. hi-1
    out[1:hi] = S1[1:hi] / 2
    out[nfft - np.arange(1, hi)] = out[1:hi]
    return out


# ---- compress --------------------------------------------------------------------------------------------------------------------
def quantile_pair(q):
    if isinstance(q, (int, float)):
        q = float(q)
        q = q if q < 0.5 else 1 - q
        return q, 1 - q
    return float(min(q)), float(max(q))


def quantile7(v, p):
    """Julia's default quantile of the SORTED values v (float64) at level p, in Python floats."""
    m = len(v)
    if m == 1:
        return float(v[0])
    aleph = m * p + (1 - p)
    j = min(max(int(aleph), 1), m - 1)
    g = min(max(aleph - j, 0.0), 1.0)
    a, b = float(v[j - 1]), float(v[j])
    with np.errstate(invalid="ignore"):
        if np.isfinite(a) and np.isfinite(b):
            return a + g * (b - a)
        return float(np.float64(1 - g) * np.float64(a) + np.float64(g) * np.float64(b))


def compress_ref(x, q):
    """(clip(x, t0, t1), (t0, t1)) with the thresholds from numpy.sort; float32 input: float order statistics, double interpolation,
    the clamp compared in double and rounded to float."""
    x = np.asarray(x)
    lo, hi = quantile_pair(q)
    v = np.sort(x.astype(np.float64).ravel())
    t0, t1 = quantile7(v, lo), quantile7(v, hi)
    return np.clip(x.astype(np.float64), t0, t1).astype(x.dtype), (t0, t1)
