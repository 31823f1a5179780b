"""Exact-phase references for angular frequencies, and numpy restatements of the device's three phase formations.  Shared by
tests/test_phase_ref_host.py (which proves both on the CPU) and the GPU tests that put weight on the low words of the phases.

THE PHASE.  exact_turns_angular(w, x) is w_f x_k / (2 pi) minus a whole number, for doubles of any magnitude:
    1  w x = p + e exactly (Dekker's two-product, Veltkamp split as tests/_lomb_ref.py: _split);
    2  p = p1 + p2, halves of at most 27 bits each (the same split);
    3  1 / (2 pi) = sum_i c_i, six chunks of 24 bits each (144 bits below 2^0), from a 100-digit pi in rational arithmetic: every
       product p_h c_i has at most 51 bits and is exact in double;
    4  each product minus its rint is exact;
    5  the twelve fractions are added in long double, reducing by rint after each addition (at most 2^-65 per addition);
    6  e / (2 pi) joins last (|e| <= 2^-53 |p|: its long-double rounding is below 2^-70 up to |w x| = 2^47).
What is cut off 1 / (2 pi) is below 2^-147: 2^-100 turns at |w x| = 2^47.  tests/test_phase_ref_host.py holds the result to 1e-18 turns
against fractions.Fraction with the same pi.  Nothing here grows with |w x|.

THE REFERENCES mirror oracle.gram_phase_ld and tests/_eval_ref.py: evaluate_ld with these phases; everything after the trigonometry is
plain long-double arithmetic.  Column order: oracle.lpv_regressor(..., permuted=True) and oracle.get_fourier_regressor.

THE RESTATEMENTS (lomb_turns, nu_turns, nudft_trig) form the phase the way csrc/lomb_device.h: lomb_sincos, csrc/nufft_coord.h:
nu_phase_turns and csrc/nudft.hip (p + d, first order in d) do, with the error of every fused multiply-add taken from the Dekker split,
and evaluate the trigonometry of that phase in long double: they model the per-term phase error of the kernels, not the device's
sincos nor the summation.  ``mutate`` drops ("x:drop") or negates ("x:neg") one low word: e; tl, D_lo; fe, wl, d."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
PI_DIGITS = "3.1415926535897932384626433832795028841971693993751058209749445923078164062862089986280348253421170679"
PI_Q = Fraction(PI_DIGITS)                               # |PI_Q - pi| < 1e-100
TWO_PI_LD = 2 * np.arccos(LD(-1))
NCHUNK, CHUNK_BITS = 6, 24


def _inv_two_pi_chunks():
    inv = 1 / (2 * PI_Q)
    out, prev = [], 0
    for i in range(1, NCHUNK + 1):
        top = int(inv * 2 ** (CHUNK_BITS * i))          # floor: inv > 0
        out.append(float(top - prev * 2 ** CHUNK_BITS) * 2.0 ** (-CHUNK_BITS * i))     # a 24-bit integer times a power of two
        prev = top
    return tuple(out)


INV_TWO_PI_CHUNKS = _inv_two_pi_chunks()


def split(a):
    """Veltkamp: a = hi + lo, at most 26 and 27 significant bits."""
    c = 134217729.0 * a                                  # 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def two_product(a, b):
    """(p, e): p = fl(a b), p + e = a b exactly (e is what fma(a, b, -p) returns)."""
    p = a * b
    ah, al = split(a)
    bh, bl = split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _wrap(a):
    return a - np.rint(a)


def exact_turns_angular(w, x):
    """w_f x_k / (2 pi) minus a whole number, (Nf, N) long doubles in [-1/2, 1/2]; w, x doubles of any magnitude."""
    w = np.asarray(w, np.float64).reshape(-1)[:, None]
    x = np.asarray(x, np.float64).reshape(-1)[None, :]
    p, e = two_product(w, x)
    acc = np.zeros(p.shape, LD)
    for c in INV_TWO_PI_CHUNKS:
        for h in split(p):
            acc = _wrap(acc + _wrap(h * c).astype(LD))   # h c: exact in double; its fraction: exact
    return _wrap(acc + e.astype(LD) / TWO_PI_LD)


def turns_fraction(w, x):
    """The same from rational arithmetic (one pair of doubles): a Fraction in [-1/2, 1/2]."""
    q = Fraction(float(w)) * Fraction(float(x)) / (2 * PI_Q)
    return q - round(q)


def trig_exact(w, x):
    """cos, sin of the real products w_f x_k: (Nf, N) long doubles."""
    ph = TWO_PI_LD * exact_turns_angular(w, x)
    return np.cos(ph), np.sin(ph)


# ---- the references ----------------------------------------------------------------------------------------------------------------------
def gram_of(Phi, Y=None, W=None, plain=False):
    """Phi' W Phi and Phi' W Y of a long-double regressor (N x n).  plain: numpy's long-double products (slow: no BLAS).  Otherwise
    Phi = Pd + Pl, Pd its rounding to doubles: Pd' W Pd and Pd' W Y are accumulated in long double by oracle.gram_ld (C, and rounded to
    doubles once: 2^-53 of the entry), the cross terms Pd' W Pl + Pl' W Pd and Pl' W Y -- 2^-53 of the scale themselves -- in doubles, and
    Pl' W Pl (2^-106) is dropped: within 2^-52 of the scale of the plain product, which tests/test_phase_ref_host.py checks."""
    N = Phi.shape[0]
    Wl = np.ones(N, LD) if W is None else np.asarray(W, np.float64).astype(LD)
    Yl = None if Y is None else np.asarray(Y, np.float64).astype(LD)
    if plain:
        return Phi.T @ (Wl[:, None] * Phi), (None if Y is None else Phi.T @ (Wl.reshape((N,) + (1,) * (Yl.ndim - 1)) * Yl))
    from oracle import oracle
    Pd = np.asfortranarray(Phi.astype(np.float64))
    Pl = (Phi - Pd.astype(LD)).astype(np.float64)
    Wd = Wl.astype(np.float64)
    G0, _, b0, _ = oracle.gram_ld(Pd, None if Y is None else np.asarray(Y, np.float64), None if W is None else Wd)
    X = Pd.T @ (Wd[:, None] * Pl)
    G = G0.astype(LD) + (X + X.T).astype(LD)
    if Y is None:
        return G, None
    Yd = np.asarray(Y, np.float64)
    return G, b0.astype(LD) + (Pl.T @ (Wd.reshape((N,) + (1,) * (Yd.ndim - 1)) * Yd)).astype(LD)


def lpv_gram_exact(X, w, K, Y=None, plain=False):
    """-> (G, b, C, s).  Phi[k][f 2nb + c nb + j] = (c ? -sin : cos)(w_f x_k) K[k][j] (oracle.lpv_regressor, permuted);
    G = Phi' Phi (n x n), b = Phi' Y (n or n x ns; None without Y) by gram_of;
    C[j][j'] = sum_k |K_kj K_kj'| and s[j] (or s[j][q]) = sum_k |K_kj y_kq|: the scales the structured forms are held to."""
    K = np.asarray(K, np.float64)
    N, nb = K.shape
    Nf = len(w)
    cs, sn = trig_exact(w, X)                            # (Nf, N)
    Kl = K.astype(LD)
    Phi = np.empty((N, Nf, 2, nb), LD)
    Phi[:, :, 0, :] = cs.T[:, :, None] * Kl[:, None, :]
    Phi[:, :, 1, :] = -sn.T[:, :, None] * Kl[:, None, :]
    G, b = gram_of(Phi.reshape(N, 2 * Nf * nb), Y, None, plain)
    C = np.abs(Kl).T @ np.abs(Kl)
    return G, b, C, (None if Y is None else np.abs(Kl).T @ np.abs(np.asarray(Y, np.float64).astype(LD)))


def fourier_gram_exact(t, w, y=None, zerofreq=False, W=None, plain=False):
    """-> (G, b, scale_G, scale_b) of oracle.get_fourier_regressor's columns [cos .. | -sin ..] / sqrt(2 Nf) (the sine of a leading zero
    frequency is left out), w_f = fl(2 pi f_f) as the library rounds it, weights W; scale_G = sum_k |W_k| / (2 Nf),
    scale_b = sum_k |W_k y_k| / sqrt(2 Nf)."""
    Nf, N = len(w), len(t)
    cs, sn = trig_exact(w, t)
    dd = 1 / np.sqrt(LD(2 * Nf))
    A = np.concatenate([cs, -sn[1:] if zerofreq else -sn], axis=0).T * dd           # (N, n)
    Wl = np.ones(N, LD) if W is None else np.asarray(W, np.float64).astype(LD)
    G, b = gram_of(A, y, W, plain)
    sG = np.abs(Wl).sum() / (2 * Nf)
    return G, b, sG, (None if y is None else np.abs(Wl * np.asarray(y, np.float64).astype(LD)).sum() * dd)


def evaluate_exact(P, w, x, K=None, scale=1.0):
    """tests/_eval_ref.py: evaluate_ld with the phases of the real products w_f x_m: (yhat, S), each (M, nc) long doubles."""
    P = np.asarray(P, np.complex128)
    P = P.reshape(P.shape[0], -1)
    Nf, M, nc = len(w), len(x), P.shape[1]
    nb = P.shape[0] // Nf
    K = np.ones((M, 1), LD) if K is None else K
    cs, sn = trig_exact(w, x)
    cs, sn = cs.T, sn.T                                  # (M, Nf)
    yh, S = np.zeros((M, nc), LD), np.zeros((M, nc), LD)
    for c in range(nc):
        for j in range(nb):
            pj = P[j * Nf:(j + 1) * Nf, c]
            re, im = pj.real.astype(LD), pj.imag.astype(LD)
            yh[:, c] += K[:, j] * (cs @ re - sn @ im)
            S[:, c] += np.abs(K[:, j]) * np.sqrt(re * re + im * im).sum()
    s = LD(scale)
    return s * yh, s * S


# ---- what the kernel headers themselves drop ---------------------------------------------------------------------------------------------
def _dd(q):
    """A rational as a double-double: (hi, lo) with hi = fl(q), lo = fl(q - hi)."""
    hi = float(q)
    return hi, float(q - Fraction(hi))


def progression(w):
    """a, D (Fractions: exact) and eps (doubles) of w_f = a + f D + eps_f, the split of csrc/gram_form_plan.h: make_ap_slots, which works
    it in double-double (at least 100 bits; tests/test_gram_form_plan.py holds its tables to these values)."""
    wq = [Fraction(float(v)) for v in np.asarray(w, np.float64)]
    a, D = wq[0], ((wq[-1] - wq[0]) / (len(wq) - 1) if len(wq) > 1 else Fraction(0))
    return a, D, np.array([float(v - (a + f * D)) for f, v in enumerate(wq)])


def merged_slot(w, xmax, limit=1e-7):
    """(merged, s0, delta) of make_ap_slots: 2a = s0 D + delta with 0 <= s0 < Nf and |delta| max|x| within the admission limit."""
    a, D, _ = progression(w)
    if D == 0:
        return False, None, 0.0
    j0 = round(2 * a / D)
    delta = float(2 * a - j0 * D)
    ok = 0 <= j0 < len(w) and abs(delta) * xmax <= limit
    return ok, (j0 if ok else None), (delta if ok else 0.0)


def second_order(w, x):
    """q of the structured forms' bound: ((2 emax + |delta|) max|x|)^2 / 2, the dropped second order of the residuals, plus
    (u max|w| max|x|)^2 / 2, csrc/nudft.hip's first-order use of d.  Long doubles, from the inputs alone."""
    xm = LD(np.abs(np.asarray(x, np.float64)).max())
    wm = LD(np.abs(np.asarray(w, np.float64)).max())
    _, _, eps = progression(w)
    _, _, delta = merged_slot(w, float(xm))
    r = (2 * LD(np.abs(eps).max()) + abs(LD(delta))) * xm
    return r * r / 2 + (LD(U) * wm * xm) ** 2 / 2


# ---- restatements of the device's phase formations ---------------------------------------------------------------------------------------
def _mut(mutate, word, v):
    if mutate == word + ":drop":
        return 0.0 * v
    if mutate == word + ":neg":
        return -v
    return v


def lomb_turns(f, t, mutate=None):
    """csrc/lomb_device.h: lomb_sincos.  p = f t, e = fma(f, t, -p), r = (p - rint(p)) + e: the turns the device hands to sincospi, (Nf, N)
    doubles."""
    f = np.asarray(f, np.float64).reshape(-1)[:, None]
    t = np.asarray(t, np.float64).reshape(-1)[None, :]
    p, e = two_product(f, t)
    return (p - np.rint(p)) + _mut(mutate, "e", e)


def lomb_turns_exact(f, t):
    """f t minus a whole number without the rounding of r: (Nf, N) long doubles (tests/_lomb_ref.py: exact_turns)."""
    f = np.asarray(f, np.float64).reshape(-1)[:, None]
    t = np.asarray(t, np.float64).reshape(-1)[None, :]
    p, e = two_product(f, t)
    return (p - np.rint(p)).astype(LD) + e.astype(LD)


I2PI_HI, I2PI_LO = 0.15915494309189535, -9.8393384885635288e-18       # csrc/nufft_coord.h


def nu_turns(D_hi, D_lo, x, mutate=None):
    """csrc/nufft_coord.h: nu_phase_turns, (D_hi + D_lo) x in turns reduced to [0, 1): (N,) doubles."""
    x = np.asarray(x, np.float64)
    th, fe = two_product(np.float64(D_hi), x)
    tl = _mut(mutate, "tl", _mut(mutate, "fe", fe) + _mut(mutate, "D_lo", np.float64(D_lo) * x))
    uh, ue = two_product(th, np.float64(I2PI_HI))
    ul = ue + (th * I2PI_LO + tl * I2PI_HI)
    r = (uh - np.rint(uh)) + ul
    return r - np.floor(r)


def dd_turns_exact(hi, lo, x):
    """(hi + lo) x / (2 pi) minus a whole number, (len(hi), N) long doubles: the phase of the double-double frequency itself."""
    return _wrap(exact_turns_angular(hi, x) + exact_turns_angular(lo, x))


def nudft_trig(wh, wl, x, mutate=None):
    """csrc/nudft.hip, step A: p = wh x, d = fma(wh, x, -p) + wl x, (c, s) = sincos(p), c2 = c - d s, s2 = s + d c.  sincos(p) is taken in
    long double at the double p (its own phase by exact_turns_angular(1, p)); -> (cos, sin), (len(wh), N) long doubles."""
    wh = np.asarray(wh, np.float64).reshape(-1)[:, None]
    wl = np.asarray(wl, np.float64).reshape(-1)[:, None]
    x = np.asarray(x, np.float64).reshape(-1)[None, :]
    p, fe = two_product(wh, x)
    d = _mut(mutate, "d", _mut(mutate, "fe", fe) + _mut(mutate, "wl", wl * x))
    ph = TWO_PI_LD * exact_turns_angular(np.ones(1), p.reshape(-1)).reshape(p.shape)
    c, s = np.cos(ph), np.sin(ph)
    dl = d.astype(LD)
    return c - dl * s, s + dl * c


# ---- host mirror of the slot tables (csrc/gram_form_plan.h: make_ap_slots) ---------------------------------------------------------------
def ap_slot_tables(w, xmax):
    """dict: merged, s0, delta, eps, and in double-double (hi, lo) the slot frequencies ``om``, the right-hand side's ``omr`` and the eight
    in-group offsets ``step``: the exact rationals of make_ap_slots' layout, rounded to double-double."""
    a, D, eps = progression(w)
    Nf = len(w)
    nf8, s8 = -(-Nf // 8) * 8, -(-(2 * Nf - 1) // 8) * 8
    merged, s0, delta = merged_slot(w, xmax)
    if merged:
        om = [j * D for j in range(-(-(s0 + 2 * Nf - 1) // 8) * 8)]
    else:
        s0 = nf8
        om = [m * D for m in range(nf8)] + [2 * a + q * D for q in range(s8)]
    tab = lambda qs: tuple(np.array(c) for c in zip(*[_dd(q) for q in qs]))     # noqa: E731
    return dict(merged=merged, s0=s0, delta=delta, eps=eps, nf8=nf8, om=tab(om), omr=tab([a + f * D for f in range(nf8)]),
                step=tab([b * D for b in range(8)]))
