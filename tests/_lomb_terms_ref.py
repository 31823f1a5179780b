"""Reference for lombscargle(..., nterms=K): the definition of include/lpvspectral.h (g7) in numpy ``longdouble``, phases from EXACT
products (``_lomb_ref.exact_turns``: f t minus a whole number, r).  The harmonic m is cos / sin(2 pi m r): m r is the exact multiple of the
exact turns, no rotation and no recurrence.  Everything after the trigonometry is plain long-double arithmetic in the order the definition
is written: the sums, A, g, b from the product identities, the floating-mean terms, A = L D L^T without pivoting, theta, p, power, c."""
import numpy as np

from _lomb_ref import LD, TWO_PI, DEGENERATE, exact_turns, yy_noise


def ldl(A):
    """A (Nf, n, n) -> unit lower L (Nf, n, n), pivots d (Nf, n) as they come out, the degenerate mask (a pivot fails d > 2^-40) and
    ``worst`` (Nf,): the smallest pivot of a frequency that is not degenerate, the first failing pivot of one that is.  A failing pivot is
    replaced by 1 for what follows (nothing of a degenerate frequency is used)."""
    Nf, n, _ = A.shape
    L = np.zeros_like(A)
    d = np.zeros((Nf, n), dtype=LD)
    used = np.zeros((Nf, n), dtype=LD)
    deg = np.zeros(Nf, dtype=bool)
    worst = np.full(Nf, np.inf, dtype=LD)
    for j in range(n):
        dj = A[:, j, j] - (L[:, j, :j] ** 2 * used[:, :j]).sum(axis=1)
        d[:, j] = dj
        fail = ~(dj > DEGENERATE)
        worst = np.where(deg, worst, np.where(fail, dj, np.minimum(worst, dj)))
        deg |= fail
        used[:, j] = np.where(fail, LD(1), dj)
        L[:, j, j] = 1
        for i in range(j + 1, n):
            L[:, i, j] = (A[:, i, j] - (L[:, i, :j] * used[:, :j] * L[:, j, :j]).sum(axis=1)) / used[:, j]
    return L, d, used, deg, worst


def ldl_solve(L, d, B):
    """Solve (L diag(d) L^T) X = B for B (Nf, n, q)."""
    n = L.shape[1]
    X = B.astype(LD).copy()
    for i in range(n):
        X[:, i] = X[:, i] - (L[:, i, :i, None] * X[:, :i]).sum(axis=1)
    X = X / d[:, :, None]
    for i in range(n - 1, -1, -1):
        X[:, i] = X[:, i] - (L[:, i + 1:, i, None] * X[:, i + 1:]).sum(axis=1)
    return X


def normal_matrix(C, S):
    """C, S: (2K + 1, Nf) with C[0] = 1, S[0] = 0 -> A (Nf, 2K, 2K) before the floating-mean terms, unknowns (a_1, b_1, a_2, b_2, ...)."""
    K = (C.shape[0] - 1) // 2
    n = 2 * K
    A = np.zeros((C.shape[1], n, n), dtype=C.dtype)
    for h in range(1, K + 1):
        for j in range(1, K + 1):
            dlt, sgn = abs(h - j), np.sign(j - h)
            A[:, 2 * (h - 1), 2 * (j - 1)] = (C[dlt] + C[h + j]) / 2
            A[:, 2 * (h - 1) + 1, 2 * (j - 1) + 1] = (C[dlt] - C[h + j]) / 2
            A[:, 2 * (h - 1), 2 * (j - 1) + 1] = (S[h + j] + sgn * S[dlt]) / 2
            A[:, 2 * (j - 1) + 1, 2 * (h - 1)] = A[:, 2 * (h - 1), 2 * (j - 1) + 1]
    return A


def lomb_terms_ref(y, t, f, nterms, W=None, fit_mean=True, center_data=True, normalization="standard", removed=None):
    """-> dict.  Sums: C, S (2K, Nf) of the harmonics 1 .. 2K; YC, YS (ns, K, Nf); Y, YY, mean (ns,); ``abs_`` + name: the sums of the
    absolute values of their terms.  Fit: A_pre, A (Nf, n, n), g (Nf, n), b_pre, b (Nf, ns, n), L, pivots, worst_pivot, degenerate (Nf,),
    theta (Nf, ns, n), a, b_h (K, Nf, ns), p, power, c (Nf, ns), YYf (ns,).  ``removed``: centre with these means (doubles; what a device
    formed) instead of the reference's own."""
    K = int(nterms)
    n = 2 * K
    y = np.asarray(y, dtype=np.float64)
    y = y.reshape(y.shape[0], -1)
    N, ns = y.shape
    Wl = np.ones(N, dtype=LD) if W is None else np.asarray(W, dtype=np.float64).astype(LD)
    w = Wl / Wl.sum()
    yl = y.astype(LD)
    mean = (w[:, None] * yl).sum(axis=0)
    R = (w[:, None] * yl * yl).sum(axis=0)
    if center_data:
        removed = mean if removed is None else np.asarray(removed, dtype=np.float64).astype(LD)
        yl = yl - removed[None, :]
    else:
        removed = np.zeros(ns, dtype=LD)
    turns = exact_turns(f, t)                                                 # (Nf, N)
    Nf = turns.shape[0]
    wy = w[:, None] * yl                                                      # (N, ns)
    r = {"removed": removed, "mean": mean, "abs_mean": (w[:, None] * np.abs(y.astype(LD))).sum(axis=0), "K": K}
    C, S, aC, aS = (np.zeros((2 * K + 1, Nf), dtype=LD) for _ in range(4))
    YC, YS, aYC, aYS = (np.zeros((ns, K, Nf), dtype=LD) for _ in range(4))
    C[0] = 1
    for m in range(1, 2 * K + 1):
        phi = TWO_PI * (m * turns)
        cs, sn = np.cos(phi), np.sin(phi)
        C[m], S[m], aC[m], aS[m] = cs @ w, sn @ w, np.abs(cs) @ w, np.abs(sn) @ w
        if m <= K:
            YC[:, m - 1], YS[:, m - 1] = (cs @ wy).T, (sn @ wy).T
            aYC[:, m - 1], aYS[:, m - 1] = (np.abs(cs) @ np.abs(wy)).T, (np.abs(sn) @ np.abs(wy)).T
    r.update(C=C[1:], S=S[1:], abs_C=aC[1:], abs_S=aS[1:], YC=YC, YS=YS, abs_YC=aYC, abs_YS=aYS)
    r["Y"], r["YY"] = wy.sum(axis=0), (wy * yl).sum(axis=0)
    noise = yy_noise(N, center_data, fit_mean, R, r["YY"])
    # normal equations
    A_pre = normal_matrix(C, S)
    g = np.stack([C[1:K + 1], S[1:K + 1]], axis=1).reshape(n, Nf).T          # (Nf, n): C_1, S_1, C_2, ...
    b_pre = np.stack([YC, YS], axis=2).reshape(ns, n, Nf).transpose(2, 0, 1)  # (Nf, ns, n)
    Y, YYf = r["Y"], r["YY"]
    A, b = A_pre, b_pre
    if fit_mean:
        A = A_pre - g[:, :, None] * g[:, None, :]
        b = b_pre - Y[None, :, None] * g[:, None, :]
        YYf = YYf - Y * Y
    L, d, used, deg, worst = ldl(A)
    theta = ldl_solve(L, used, b.transpose(0, 2, 1)).transpose(0, 2, 1)       # (Nf, ns, n)
    p = (b * theta).sum(axis=2)                                               # (Nf, ns)
    c = removed[None, :] + ((Y[None, :] - (g[:, None, :] * theta).sum(axis=2)) if fit_mean else 0 * p)
    if normalization == "standard":
        live = np.broadcast_to(YYf > noise, p.shape)
        power = np.where(live, p / np.where(live, np.broadcast_to(YYf, p.shape), LD(1)), LD(0))
    else:
        power = p * N / 2
    z = deg[:, None]
    theta = np.where(z[:, :, None], LD(0), theta)
    r.update(A_pre=A_pre, A=A, g=g, b_pre=b_pre, b=b, L=L, pivots=d, pivots_used=used, worst_pivot=worst, degenerate=deg, theta=theta,
             a=theta[:, :, 0::2].transpose(2, 0, 1), b_h=theta[:, :, 1::2].transpose(2, 0, 1), p=np.where(z, LD(0), p),
             power=np.where(z, LD(0), power), c=np.where(z, LD(0), c), YYf=YYf)
    return r
