"""Reference for wwz: the definition of include/lpvspectral.h (g8) on top of tests/_lomb_ref.lomb_ref.

Cell (k, j) is ``lomb_ref(y[sl], t[sl], [f_k], W = W[sl] g)`` -- the floating-mean fit of g4 of the samples in reach -- with the Gaussian
weight g = exp(-a_k (t - tau_j)^2) evaluated in long double from the DOUBLES a_k, t and tau_j, and on top of it, in long double, Neff,
Foster's Z and his amplitude.  lomb_ref reads its weights as doubles, so the product W g is rounded to double once (a relative error of
2^-53 per weight on the reference's side; the GPU test accounts for it).  The reach follows the stated edges: lo = tau - radius and
hi = tau + radius formed in double, start = #{t < lo}, count = #{t <= hi} - start (numpy's searchsorted, left and right)."""
import numpy as np

from _lomb_ref import LD, lomb_ref, yy_noise

TWO_PI_DOUBLE = 6.283185307179586


def decay(c, f):
    """a_k = c (2 pi f_k)^2 as the library forms it once per frequency: w = 6.283185307179586 * f, a = c * (w * w), in double."""
    w = np.float64(TWO_PI_DOUBLE) * np.asarray(f, dtype=np.float64)
    return np.float64(c) * (w * w)


def radius(f, c, wmin):
    """What lpvspectral.jl_amd.wwz_radius computes (the host expression is the definition), repeated here so that the host tests need no
    library: sqrt(log(1 / wmin) / c) / (2 pi f) in numpy doubles, inf for wmin = 0."""
    f = np.asarray(f, dtype=np.float64)
    if wmin == 0:
        return np.full(f.shape, np.inf)
    return np.sqrt(np.log(1.0 / np.float64(wmin)) / np.float64(c)) / (2.0 * np.pi * f)


def reach(t, tau, r):
    """(start, count) of one cell."""
    lo, hi = np.float64(tau) - np.float64(r), np.float64(tau) + np.float64(r)
    start = int(np.searchsorted(t, lo, side="left"))
    return start, max(int(np.searchsorted(t, hi, side="right")) - start, 0)


def weights(t, W, tau, a):
    """Long-double W g of the samples t (a slice), and the exponents x = a d^2 (>= 0)."""
    d = t.astype(LD) - LD(tau)
    x = LD(a) * d * d
    Wl = np.ones(len(t), dtype=LD) if W is None else np.asarray(W, dtype=np.float64).astype(LD)
    return Wl * np.exp(-x), x


def wwz_cell_ref(y, t, W, f, tau, a, r, center=True, removed=None):
    """One cell, all signals of y (N, ns); ``center``, ``removed``: lomb_ref's center_data and the means to remove (None: the cell's own; the
    floating mean makes everything but the raw sums invariant under them) -> None for an empty cell, else a dict: ``fit`` (lomb_ref's dict of the slice), ``start``,
    ``count``, ``Wg`` (the doubles lomb_ref read), ``Wgl`` and ``x`` (long double), ``neff``, and per signal ``power``, ``amplitude``,
    ``wwz``, ``a``, ``b``, ``c``, ``p``, ``YYf`` (YY after the floating mean) and ``noise`` (the constant-signal threshold)."""
    y = np.asarray(y, dtype=np.float64).reshape(len(t), -1)
    start, count = reach(t, tau, r)
    if count == 0:
        return None
    sl = slice(start, start + count)
    Wgl, x = weights(t[sl], None if W is None else W[sl], tau, a)
    Wg = Wgl.astype(np.float64)
    if not Wg.sum() > 0:
        return None
    fit = lomb_ref(y[sl], t[sl], [f], W=Wg, fit_mean=True, center_data=center, removed=removed)
    S1, S2 = Wgl.sum(), (Wgl * Wgl).sum()
    neff = S1 * S1 / S2
    p, YYf = fit["p"][0], fit["YYf"]
    # the threshold of lomb_ref's own standard power: YY <= noise -> 0
    w = Wg.astype(LD) / Wg.astype(LD).sum()
    R = (w[:, None] * y[sl].astype(LD) ** 2).sum(axis=0)
    noise = yy_noise(count, center, True, R, fit["YY"])
    rest = YYf - p
    with np.errstate(all="ignore"):
        z = np.where(rest > noise, (neff - 3) * p / (2 * np.where(rest > noise, rest, LD(1))), LD(np.inf))
    z = np.where((neff > 3) & (YYf > noise) & ~fit["degenerate"][0], z, LD(0))
    return {"fit": fit, "start": start, "count": count, "Wg": Wg, "Wgl": Wgl, "x": x, "neff": neff, "degenerate": bool(fit["degenerate"][0]),
            "power": fit["power"][0], "amplitude": np.sqrt(fit["a"][0] ** 2 + fit["b"][0] ** 2), "wwz": z, "a": fit["a"][0], "b": fit["b"][0],
            "c": fit["c"][0], "p": p, "YYf": YYf, "noise": noise}


def wwz_foster(y, t, W, f, tau, a, r):
    """Foster's own formulation (AJ 112, 1709, section 5) of one cell and ONE signal, long double: the weighted projection onto
    phi_1 = 1, phi_2 = cos w (t - tau), phi_3 = sin w (t - tau) with w = 2 pi f and statistical weights w_n = W g / sum W g:
      S_ab = <phi_a | phi_b> = sum w phi_a phi_b,  y_a = sum_b S^-1_ab <phi_b | x>  (the least-squares coefficients),
      Vx = <x | x> - <1 | x>^2,   Vy = <y | y> - <1 | y>^2  with y(t) = sum y_a phi_a(t) the model,
      Neff = (sum W g)^2 / sum (W g)^2,   Z = (Neff - 3) Vy / (2 (Vx - Vy)),   WWA = sqrt(y_2^2 + y_3^2).
    -> dict(Z, WWA, Vx, Vy, neff, coef = (y_1, y_2, y_3)).  The angle w (t - tau) is formed from exact turns where the test's inputs make
    f t and f tau exact; here it is plain long double, which is accurate to 1e-15 for the sizes the host test uses."""
    start, count = reach(t, tau, r)
    sl = slice(start, start + count)
    Wgl, _ = weights(t[sl], None if W is None else W[sl], tau, a)
    w = Wgl / Wgl.sum()
    x = np.asarray(y, dtype=np.float64)[sl].astype(LD)
    ang = 2 * np.arccos(LD(-1)) * LD(f) * (t[sl].astype(LD) - LD(tau))
    Phi = np.stack([np.ones(count, dtype=LD), np.cos(ang), np.sin(ang)], axis=1)
    S = (Phi * w[:, None]).T @ Phi
    rhs = (Phi * w[:, None]).T @ x
    # 3 x 3 solve in long double (numpy.linalg works in double): Cramer's rule
    def det3(M):
        return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
                + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))
    D = det3(S)
    coef = []
    for i in range(3):
        M = S.copy()
        M[:, i] = rhs
        coef.append(det3(M) / D)
    coef = np.array(coef, dtype=LD)
    model = Phi @ coef
    Vx = (w * x * x).sum() - (w * x).sum() ** 2
    Vy = (w * model * model).sum() - (w * model).sum() ** 2
    neff = Wgl.sum() ** 2 / (Wgl * Wgl).sum()
    return {"Z": (neff - 3) * Vy / (2 * (Vx - Vy)), "WWA": np.sqrt(coef[1] ** 2 + coef[2] ** 2), "Vx": Vx, "Vy": Vy, "neff": neff, "coef": coef}
