"""Reference for lombscargle: the definition of include/lpvspectral.h (g4) in numpy ``longdouble``, phases from EXACT products.

The phase of (f, t) is 2 pi (f t) with the product formed without error (Dekker's two-product in double: p + e = f t exactly), reduced
to one cycle exactly (p - rint(p) is exact), and only then widened: nothing in the reference grows with |f t|.  Everything after the
trigonometry is plain long-double arithmetic in the order the definition is written."""
import numpy as np

LD = np.longdouble
TWO_PI = 2 * np.arccos(LD(-1))
DEGENERATE = LD(2.0) ** -40


def _split(a):
    c = 134217729.0 * a                                # 2^27 + 1 (Veltkamp)
    hi = c - (c - a)
    return hi, a - hi


def exact_turns(f, t):
    """f_k t_n minus a whole number as long doubles, shape (Nf, N), |.| <= 1/2 + |e| (e: the rounding error of the double product);
    the inputs are doubles."""
    f = np.asarray(f, dtype=np.float64)[:, None]
    t = np.asarray(t, dtype=np.float64)[None, :]
    p = f * t
    fh, fl = _split(f)
    th, tl = _split(t)
    e = ((fh * th - p) + fh * tl + fl * th) + fl * tl   # p + e == f t exactly
    return (p - np.rint(p)).astype(LD) + e.astype(LD)


def yy_noise(N, center_data, fit_mean, R, YY_before):
    """What counts as YY = 0 for the standard power (csrc/lomb_plan.h: lomb_yy_noise): the residue centring and YY - Y^2 leave of a constant."""
    nu = LD(N + 16) * LD(2.0) ** -53
    return (nu * nu * R if center_data else 0 * R) + (3 * nu * YY_before if fit_mean else 0 * R)


def lomb_ref(y, t, f, W=None, fit_mean=True, center_data=True, normalization="standard", removed=None):
    """-> dict: the raw sums (C, S, C2, S2: (Nf,); YC, YS: (ns, Nf); Y, YY: (ns,)), the sums of the absolute values of their terms under
    the same names with an ``abs_`` prefix, D, the degenerate mask, power (Nf, ns), a, b, c (Nf, ns), the weighted mean (ns,) and the mean
    that was removed.  ``removed``: centre with these means (doubles; what a device formed) instead of the reference's own, so that the
    sums that follow are those of the SAME centred signal."""
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
    phi = TWO_PI * exact_turns(f, t)
    cs, sn = np.cos(phi), np.sin(phi)
    c2, s2 = np.cos(2 * phi), np.sin(2 * phi)
    r = {"removed": removed, "mean": mean, "abs_mean": (w[:, None] * np.abs(y.astype(LD))).sum(axis=0)}
    r["C"], r["S"], r["C2"], r["S2"] = cs @ w, sn @ w, c2 @ w, s2 @ w
    r["abs_C"], r["abs_S"], r["abs_C2"], r["abs_S2"] = np.abs(cs) @ w, np.abs(sn) @ w, np.abs(c2) @ w, np.abs(s2) @ w
    wy = w[:, None] * yl                                # (N, ns)
    r["Y"], r["YY"] = wy.sum(axis=0), (wy * yl).sum(axis=0)
    r["YC"], r["YS"] = (cs @ wy).T, (sn @ wy).T          # (ns, Nf)
    r["abs_YC"], r["abs_YS"] = (np.abs(cs) @ np.abs(wy)).T, (np.abs(sn) @ np.abs(wy)).T
    C, S = r["C"][:, None], r["S"][:, None]
    CC, SS, CS = (1 + r["C2"])[:, None] / 2, (1 - r["C2"])[:, None] / 2, r["S2"][:, None] / 2
    scale = CC + SS
    Y, YY, YC, YS = r["Y"][None, :], r["YY"][None, :], r["YC"].T, r["YS"].T
    noise = yy_noise(N, center_data, fit_mean, R, r["YY"])[None, :]
    if fit_mean:
        YY, YC, YS = YY - Y * Y, YC - Y * C, YS - Y * S
        CC, SS, CS = CC - C * C, SS - S * S, CS - C * S
    D = CC * SS - CS * CS
    deg = (D <= DEGENERATE * scale * scale)[:, 0]
    Ds = np.where(deg[:, None], LD(1), D)
    p = (SS * YC * YC + CC * YS * YS - 2 * CS * YC * YS) / Ds
    a, b = (SS * YC - CS * YS) / Ds, (CC * YS - CS * YC) / Ds
    c = removed[None, :] + ((Y - a * C - b * S) if fit_mean else 0 * a)
    if normalization == "standard":
        YYb = np.broadcast_to(YY, p.shape)
        live = YYb > np.broadcast_to(noise, p.shape)
        power = np.where(live, p / np.where(live, YYb, LD(1)), LD(0))
    else:
        power = p * N / 2
    z = deg[:, None]
    r.update(D=D[:, 0], degenerate=deg, CC=CC[:, 0], SS=SS[:, 0], CS=CS[:, 0], YYf=np.broadcast_to(YY, p.shape)[0], YCf=YC, YSf=YS,
             power=np.where(z, LD(0), power), a=np.where(z, LD(0), a), b=np.where(z, LD(0), b), c=np.where(z, LD(0), c), p=np.where(z, LD(0), p))
    return r


# ---- inputs whose products f t are all inexact (the GPU tests' second family of cases) -------------------------------------------------------
# The first family keeps t on multiples of 2^-10 over a few tens of units and f on multiples of 2^-6: every product is exact and the low
# word e of csrc/lomb_device.h: lomb_sincos is identically zero.  Here t spans [0, 2^20] -- still on the 2^-10 lattice where a test needs
# t - lo or t - tau exact, full-mantissa doubles otherwise -- and f are full-mantissa doubles in (0, 3]: f t reaches 3e6 turns, e is up to
# 2^-54 f t = 2e-10 turns, and a kernel without it misses every bound by orders of magnitude (tests/test_phase_ref_host.py).
LATE_SPAN = 2 ** 20
WIDE_STEP = 0.0123                                    # no binary fraction: the grids a + k D carry natural rounding residuals


def late_times(rng, N, lattice=True):
    """N sorted times in [0, 2^20]: multiples of 2^-10, or full-mantissa doubles."""
    return np.sort(rng.integers(0, LATE_SPAN * 1024, N) / 1024.0 if lattice else rng.uniform(0.0, LATE_SPAN, N))


def wide_freqs(rng, Nf):
    """Nf distinct full-mantissa frequencies in (0, 3], sorted."""
    return np.sort(3.0 - rng.uniform(0.0, 3.0, Nf))


def wide_grid(first, Nf=200):
    """a + k D with a = first * D, as doubles round it (first = 0: the zero frequency leads)."""
    return first * WIDE_STEP + WIDE_STEP * np.arange(Nf)


def block_residual_phase(f, t, block=None):
    """2 pi max|f[k] - f[k0] - (k - k0) D| max|t| in radians, D the end-point step and k0 the first frequency of k's block (csrc/lomb_plan.h:
    lomb_block_residuals), in rational arithmetic: the residual phase whose square the transform path drops."""
    from fractions import Fraction
    fq = [Fraction(float(v)) for v in f]
    D = (fq[-1] - fq[0]) / (len(fq) - 1)
    L = len(fq) if block is None else block
    e = max(abs(fq[k] - fq[k // L * L] - (k - k // L * L) * D) for k in range(len(fq)))
    return float(2 * np.arccos(LD(-1))) * float(e) * float(np.abs(t).max())
