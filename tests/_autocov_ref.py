"""A numpy restatement of src/autocov.jl (autocov / autocor at arbitrary sample times), written from its semantics: the checker of
tests/test_gpu_autocov.py and the CPU baseline of tools/autocov_time.py.  Test infrastructure, not product code.

Every function also returns ``scale``: per output element, the magnitude the equidistant branch's lag sum is made of
(sum |y_i y_{i+j}| / divisor), 0 elsewhere -- the yardstick of that branch's tolerance."""
import math

import numpy as np

EPS = np.finfo(np.float64).eps


def isequidistant(t):
    """src/autocov.jl:112-121 (a range: step > 0; a vector: d = t[1]-t[0] > 0 and abs(abs(t[i]-t[i-1]) - d) < 20d*eps())."""
    if isinstance(t, range):
        return t.step > 0
    t = np.asarray(t)
    if len(t) < 2:
        raise ValueError("isequidistant needs at least 2 samples")
    d = t[1] - t[0]
    if not d > 0:
        return False
    dev = np.abs(np.abs(t[2:] - t[1:-1]) - d)
    thr = float(t.dtype.type(20) * d) * EPS if t.dtype.kind == "f" else float(20 * int(d)) * EPS
    return bool(np.all(dev.astype(np.float64) < thr))


def _as_times(t):
    return np.arange(t.start, t.stop, t.step, dtype=np.int64) if isinstance(t, range) else np.asarray(t)


def _one(kind, t, y, maxlag, normalize):
    """One segment: (tau, acf, scale) in enumeration order (i-major, then j) of the kept pairs, NOT yet sorted."""
    eq = isequidistant(t)
    t = _as_times(t)
    y = np.asarray(y)
    n = len(y)
    I, K = np.triu_indices(n)                     # (i, i+j) i-major, j ascending
    tau = np.abs(t[K] - t[I])
    keep = ~(tau.astype(np.float64) > float(maxlag))
    I, K, tau = I[keep], K[keep], tau[keep]
    j = K - I
    yd = y.astype(np.float64)
    mean = math.fsum(yd) / n
    var = math.fsum((yd - mean) ** 2) / (n - 1)                          # corrected variance, correctly rounded but for rare ties
    scale = np.zeros(len(tau))
    if eq:
        prods = [yd[: n - k] * yd[k:] for k in range(n)]
        dots = np.array([p.sum() for p in prods])
        absd = np.array([np.abs(p).sum() for p in prods])
        if kind == "cov":
            div = n - normalize * (np.arange(n) - 1.0)                     # src/autocov.jl:47
        else:
            dd = float(y.dtype.type(math.fsum(yd * yd)))
            div = dd * (n - normalize * np.arange(n, dtype=np.float64)) / n  # src/autocov.jl:90
        with np.errstate(divide="ignore", invalid="ignore"):            # dot(y,y) = 0: replaced by the ones rule below
            acf = (dots / div)[j].astype(y.dtype)
            scale = (absd / np.abs(div))[j]
        if kind == "cov" and (np.all(y == y[0]) or float(y.dtype.type(var)) < EPS):
            acf = np.zeros(len(tau), dtype=y.dtype)
        if kind == "cor" and float(y.dtype.type(math.fsum(yd * yd))) < EPS:
            acf = np.ones(len(tau), dtype=y.dtype)
    else:
        prod = y[I] * y[K]                                                # in the eltype of y
        if kind == "cov":
            acf = prod
            if np.all(y == y[0]) or float(y.dtype.type(var)) < EPS:
                acf = np.zeros(len(tau), dtype=y.dtype)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):        # var = 0: replaced by the ones rule below
                acf = (prod / y.dtype.type(var)).astype(y.dtype)
            if float(y.dtype.type(var)) < EPS:
                acf = np.ones(len(tau), dtype=y.dtype)
            else:
                acf[tau == 0] = 1
    return tau, acf, scale


def _stable_order(tau):
    return np.argsort(tau, kind="stable")         # NaN sorts last, ties keep their order (Julia's sortperm)


def autofun(kind, t, y, maxlag, normalize=False):
    """kind 'cov' | 'cor'; t / y arrays (or a range t), or lists of segments (src/autocov.jl:1-12) -> (tau, acf, scale)."""
    seg = isinstance(y, (list, tuple)) and len(y) and not np.isscalar(y[0])
    ts, ys = (list(t), list(y)) if seg else ([t], [y])
    parts = []
    for a, b in zip(ts, ys):
        tau, acf, sc = _one(kind, a, b, maxlag, normalize)
        o = _stable_order(tau)
        parts.append((tau[o], acf[o], sc[o]))
    tau = np.concatenate([p[0] for p in parts])
    acf = np.concatenate([p[1] for p in parts])
    sc = np.concatenate([p[2] for p in parts])
    o = _stable_order(tau)
    return tau[o], acf[o], sc[o]
