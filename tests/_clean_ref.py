"""References of CLEAN (include/lpvspectral.h g11; csrc/clean.hip, csrc/clean_plan.h).

``clean_model``   the float64 MODEL of the loop: separate real arithmetic on numpy float64 arrays -- no complex dtype, whose products
                  numpy may form in another order --, every product, sum and quotient one rounded operation in the order the header
                  states.  The device is held to it bit for bit.
``clean_loop_ld`` the same loop in np.longdouble, with the gap between the best and the second-best admissible P of every iteration:
                  what the model's picks are checked against, and what says that a case is unambiguous.
``sums_ld``       D and Wn as long-double sums, with the sums of the terms' moduli the bounds need.
``restore_ld``    the restoration as a long-double gather.
Spectra are pairs (re, im) of real arrays here; ``to_complex`` / ``from_complex`` convert at the boundary."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
MIN_DEN = 2.0 ** -20
NITER, TOL, EMPTY = 0, 1, 2


def from_complex(z):
    z = np.asarray(z)
    return np.ascontiguousarray(z.real.astype(np.float64)), np.ascontiguousarray(z.imag.astype(np.float64))


def to_complex(re, im):
    out = np.empty(np.shape(re), dtype=np.complex128)
    out.real, out.imag = re, im
    return out


def exact_record(seed, N, ns, span=40):
    """The exact-phase family of tests/_bls_ref.py: t in multiples of 2^-10 (sorted), so that every product with a multiple of 2^-6 is
    exact in double; signals with two lines and noise; weights in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, span * 1024, N) / 1024.0)
    y = (np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(ns)[None, :]) * (1.0 + np.arange(ns))[None, :]
         + 0.6 * np.cos(2 * np.pi * 2.75 * t[:, None] - 1.1) + 0.25 * rng.standard_normal((N, ns)) + 0.75)
    W = rng.uniform(0.5, 2.0, N)
    return t, y, W


def planted_record(seed):
    """The planted case: 400 times in (-8, 8) on multiples of 2^-10, df = 1/64, Nf = 257, lines at bins 40 and 93."""
    t = np.round(np.sort(np.random.default_rng(seed).uniform(-8, 8, 400)) * 1024) / 1024
    df, Nf = 1.0 / 64.0, 257
    y = np.cos(2 * np.pi * (40 * df) * t + 0.7) + 0.6 * np.cos(2 * np.pi * (93 * df) * t - 1.1)
    return t, y, df, Nf


# The cases the GPU's loop is held to bit for bit (tests/test_gpu_clean.py), and whose unambiguity tests/test_clean_ref_host.py asserts.
# name -> (record, N, Nf, ns, gain, niter, tol).  Nf: below, at and above the 256 bins of one pass of 64 threads x 4 bins, not a multiple of
# it, several passes, the last size whose residual fits the LDS budget (8192) and the first that does not; the last two with 64
# iterations.  The records carry noise, so that a run never reaches the rounding floor, where picks would be decided by roundings.
LOOP_CASES = {
    "nf2": ("exact", 257, 2, 1, 0.5, 300, 2.0 ** -20),
    "nf3": ("exact", 257, 3, 3, 1.0, 300, 2.0 ** -20),
    "nf255": ("exact", 257, 255, 1, 0.5, 300, 2.0 ** -20),
    "nf256": ("exact", 1500, 256, 3, 0.1, 300, 0.0),
    "nf257": ("exact", 257, 257, 1, 1.0, 300, 2.0 ** -20),
    "nf257-one": ("exact", 257, 257, 3, 0.5, 1, 0.0),
    "nf257-zero": ("exact", 257, 257, 1, 0.5, 0, 0.0),
    "nf1030": ("exact", 1500, 1030, 3, 0.5, 300, 0.0),
    "nf8192": ("exact", 257, 8192, 1, 0.5, 64, 0.0),
    "nf8193": ("exact", 257, 8193, 3, 0.5, 64, 0.0),
    "planted": ("planted", 400, 257, 1, 0.5, 300, 1e-6),
    "uniform": ("uniform", 64, 3, 1, 0.5, 300, 0.0),
}


def loop_case(name):
    """dict(t, y (N, ns), W or None, df, Nf, ns, gain, niter, tol) of a case of LOOP_CASES."""
    kind, N, Nf, ns, gain, niter, tol = LOOP_CASES[name]
    if kind == "planted":
        t, y, df, _ = planted_record(0)
        y, W = y[:, None], None
    elif kind == "uniform":                                                  # t = 0 .. 63, df = 1/2: Wn_2p = 1 at every p -- no bin is admissible
        t = np.arange(64.0)
        y, W, df = np.cos(2 * np.pi * 0.25 * t)[:, None] + 0.5, None, 0.5
    else:
        t, y, W = exact_record(Nf, N, ns)
        df = 1.0 / 64.0
    return dict(t=t, y=y, W=W, df=df, Nf=Nf, ns=ns, gain=gain, niter=niter, tol=tol)


def host_spectra(case):
    """D [ns][Nf] and Wn [2 Nf - 1] of a case as complex128: the long-double sums rounded to double."""
    (Dre, Dim), (Wre, Wim), *_ = sums_ld(case["y"], case["t"], case["df"], case["Nf"], W=case["W"])
    return to_complex(Dre.astype(np.float64), Dim.astype(np.float64)), to_complex(Wre.astype(np.float64), Wim.astype(np.float64))


def sums_ld(y, t, df, Nf, W=None, center=True, removed=None):
    """Long-double D [ns][Nf] and Wn [2 Nf - 1] as (re, im) pairs, and absD [ns][Nf], absW: the sums of the terms' moduli.  The phases are
    those of the products (m df) t formed in long double from the double m df -- exact for the exact-phase family.  removed: the
    means to centre with (None: the long-double weighted means)."""
    t = np.asarray(t, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(len(t), -1)
    Wl = np.ones(len(t), dtype=LD) if W is None else np.asarray(W).astype(LD)
    w = Wl / Wl.sum()
    yl = y.astype(LD)
    mean = (w[:, None] * yl).sum(axis=0) if removed is None else np.asarray(removed).astype(LD)
    yc = yl - mean[None, :] if center else yl
    f = (np.arange(2 * Nf - 1, dtype=np.float64) * np.float64(df)).astype(LD)
    turns = f[:, None] * t.astype(LD)[None, :]
    turns = turns - np.rint(turns)
    ang = LD("6.283185307179586476925286766559005768") * turns
    c, s = np.cos(ang), np.sin(ang)
    Wn = ((c * w[None, :]).sum(axis=1), -(s * w[None, :]).sum(axis=1))
    wy = w[:, None] * yc                                                      # (N, ns)
    Dre = c[:Nf] @ wy
    Dim = -(s[:Nf] @ wy)
    absD = (np.abs(c[:Nf]) @ np.abs(wy)).T, (np.abs(s[:Nf]) @ np.abs(wy)).T
    absW = (np.abs(c) * w[None, :]).sum(axis=1), (np.abs(s) * w[None, :]).sum(axis=1)
    return (Dre.T, Dim.T), Wn, absD, absW, (w[:, None] * np.abs(yc)).sum(axis=0), (w[:, None] * np.abs(yl)).sum(axis=0)


def _loop(Dre, Dim, Wre, Wim, gain, niter, tol, T, track_gap):
    """The loop of g11 for one signal in the arithmetic of dtype T, operation for operation."""
    Nf = len(Dre)
    K = Nf - 1
    Rre, Rim = np.array(Dre, dtype=T), np.array(Dim, dtype=T)
    Wre, Wim = np.asarray(Wre, dtype=T), np.asarray(Wim, dtype=T)
    gain, tol = T(gain), T(tol)
    Cre, Cim = np.zeros(Nf, dtype=T), np.zeros(Nf, dtype=T)
    w2r, w2i = Wre[0:2 * K + 1:2], Wim[0:2 * K + 1:2]
    den = T(1) - (w2r * w2r + w2i * w2i)
    adm = den >= T(MIN_DEN)
    picks = np.full(niter, -1, dtype=np.int32)
    pvr, pvi = np.zeros(niter, dtype=T), np.zeros(niter, dtype=T)
    k = np.arange(Nf)
    status, it, thr, gaps = NITER, 0, T(0), []
    with np.errstate(over="ignore", invalid="ignore"):
        while it < niter:
            P = Rre * Rre + Rim * Rim
            Pa = np.where(adm & ~np.isnan(P), P, T(-1))
            p = int(np.argmax(Pa))                                            # the first of equal maxima: the lowest index
            if not Pa[p] >= 0:
                status = EMPTY
                break
            if track_gap:
                rest = np.delete(Pa, p)
                second = rest.max() if len(rest) and rest.max() >= 0 else T(0)
                gaps.append(float((Pa[p] - second) / Pa[p]) if Pa[p] > 0 else 0.0)
            if it == 0:
                thr = (tol * tol) * P[p]
            if tol > 0 and P[p] <= thr:
                status = TOL
                break
            r, q, u, v = Rre[p], Rim[p], w2r[p], w2i[p]
            tr = r * u + q * v
            ti = r * v - q * u
            cr = gain * ((r - tr) / den[p])
            ci = gain * ((q - ti) / den[p])
            Cre[p] = Cre[p] + cr
            Cim[p] = Cim[p] + ci
            picks[it], pvr[it], pvi[it] = p, cr, ci
            m1 = k - p
            a1, b1 = Wre[np.abs(m1)], np.where(m1 < 0, -Wim[np.abs(m1)], Wim[np.abs(m1)])
            a2, b2 = Wre[k + p], Wim[k + p]
            ur = (cr * a1 - ci * b1) + (cr * a2 + ci * b2)
            ui = (cr * b1 + ci * a1) + (cr * b2 - ci * a2)
            Rre = Rre - ur
            Rim = Rim - ui
            it += 1
    out = dict(R=(Rre, Rim), C=(Cre, Cim), picks=picks, pick_values=(pvr, pvi), iterations=it, status=status, admissible=adm, den=den)
    if track_gap:
        out["gaps"] = np.array(gaps)
    return out


def clean_model(D, Wn, gain, niter, tol):
    """The float64 model on one signal: D, Wn complex (or (re, im) pairs)."""
    Dre, Dim = D if isinstance(D, tuple) else from_complex(D)
    Wre, Wim = Wn if isinstance(Wn, tuple) else from_complex(Wn)
    return _loop(Dre, Dim, Wre, Wim, gain, niter, tol, np.float64, False)


def clean_loop_ld(D, Wn, gain, niter, tol):
    """The same loop in long double on the same (double) inputs; ``gaps``: per iteration (P_best - P_second) / P_best over the admissible bins."""
    Dre, Dim = D if isinstance(D, tuple) else from_complex(D)
    Wre, Wim = Wn if isinstance(Wn, tuple) else from_complex(Wn)
    return _loop(Dre, Dim, Wre, Wim, gain, niter, tol, LD, True)


def conservation(D, Wn, R, C):
    """(residue, bound) of D_k = R_k + sum_p [C_p Wn_{k-p} + conj(C_p) Wn_{k+p}], evaluated in long double over the nonzero components:
    the largest |residue| per entry and, per entry, sum|terms| = |R_k| + sum_p |C_p| (|Wn_{k-p}| + |Wn_{k+p}|) (components: re and im
    each bounded by the moduli)."""
    Dre, Dim = (a.astype(LD) for a in (D if isinstance(D, tuple) else from_complex(D)))
    Wre, Wim = (a.astype(LD) for a in (Wn if isinstance(Wn, tuple) else from_complex(Wn)))
    Rre, Rim = (a.astype(LD) for a in (R if isinstance(R, tuple) else from_complex(R)))
    Cre, Cim = (a.astype(LD) for a in (C if isinstance(C, tuple) else from_complex(C)))
    Nf = len(Dre)
    k = np.arange(Nf)
    sre, sim, mag = Rre.copy(), Rim.copy(), np.hypot(Rre, Rim)
    for p in np.nonzero((Cre != 0) | (Cim != 0))[0]:
        m1 = k - p
        a1, b1 = Wre[np.abs(m1)], np.where(m1 < 0, -Wim[np.abs(m1)], Wim[np.abs(m1)])
        a2, b2 = Wre[k + p], Wim[k + p]
        sre = sre + (Cre[p] * a1 - Cim[p] * b1) + (Cre[p] * a2 + Cim[p] * b2)
        sim = sim + (Cre[p] * b1 + Cim[p] * a1) + (Cre[p] * b2 - Cim[p] * a2)
        mag = mag + np.hypot(Cre[p], Cim[p]) * (np.hypot(a1, b1) + np.hypot(a2, b2))
    return np.maximum(np.abs(sre - Dre), np.abs(sim - Dim)), mag


# ---- planted spectra: the tie rule, the stop and the cut decide every pick --------------------------------------------------------------------
# The loop takes any finite D and Wn, so ties are planted where records never produce them.  With the DELTA WINDOW Wn = (1, 0, 0, ...):
# den_0 = 0 (bin 0 is inadmissible) and den_p = 1 elsewhere; a pick of bin p has c = gain R_p, changes bin p alone (every other bin has
# +-0 subtracted) and leaves R_p - c there.  With gain 1/2 or 1 and D of small Gaussian integers every operation is exact, so the answer
# is known in closed form and delta_oracle states it without the model.  No -0.0 may enter: x - (-0.0) turns a residual of -0.0 into +0.0
# in the loop's update pass, which the oracle does not walk (asserted on its input; none arises from +0.0 and exact halvings).
PLANTED_NF = [256 * w - 1 for w in range(1, 17)] + [2, 3, 65, 8192, 8193]      # threads = 64 w with a ragged last stride; the edges of the plan
MODEL_NF_MOST = 1030                                                           # beyond it the device is held to the oracle alone (the model is slow)
_UNITS25 = ((5, 0), (3, 4), (-4, 3), (0, -5), (-3, -4))                        # |.|^2 = 25, five different bit patterns
_UNITS1 = ((1, 0), (0, 1), (-1, 0), (0, -1))


def _gaussian(pairs, Nf):
    z = np.zeros(Nf, dtype=np.complex128)
    z.real = [pairs[k % len(pairs)][0] for k in range(Nf)]
    z.imag = [pairs[k % len(pairs)][1] for k in range(Nf)]
    return z + 0.0                                                             # (-0.0 + 0.0 = +0.0: no negative zero)


def delta_window(Nf):
    Wn = np.zeros(2 * Nf - 1, dtype=np.complex128)
    Wn[0] = 1.0
    return Wn


def planted_spectra(Nf):
    """D [4][Nf]: 0 all bins 5; 1 the five Gaussian integers of modulus 5 in turn (P ties, the residual's bits do not); 2 modulus 5 at
    the bins 1 + 64 j only -- the same lane of every wave and stride -- and modulus 1 elsewhere; 3 zero."""
    D = np.zeros((4, Nf), dtype=np.complex128)
    D[0] = 5.0
    D[1] = _gaussian(_UNITS25, Nf)
    D[2] = _gaussian(_UNITS1, Nf)
    at = np.arange(1, Nf, 64)
    D[2, at] = _gaussian(_UNITS25, len(at))
    D.setflags(write=False)
    return D


def delta_oracle(D, gain, niter, tol):
    """The loop on the delta window as a scalar simulation, independent of _loop: a heap of (-P_p, p) over the bins 1 .. Nf - 1 -- its
    top is the largest P at the lowest index --, c = gain R_p, C_p += c, R_p -= c.  -> the dict of clean_model, spectra as complex arrays."""
    import heapq
    D = np.asarray(D, dtype=np.complex128)
    Nf = len(D)
    re, im = [float(v) for v in D.real], [float(v) for v in D.imag]
    assert not np.signbit(D.real[D.real == 0]).any() and not np.signbit(D.imag[D.imag == 0]).any(), "the oracle takes no -0.0"
    cre, cim = [0.0] * Nf, [0.0] * Nf
    heap = [(-(re[p] * re[p] + im[p] * im[p]), p) for p in range(1, Nf)]
    heapq.heapify(heap)
    picks, pvr, pvi = [-1] * niter, [0.0] * niter, [0.0] * niter
    it, status, thr = 0, NITER, 0.0
    while it < niter:
        if not heap:
            status = EMPTY
            break
        negP, p = heap[0]
        P = -negP
        assert P == P, "a NaN arose"
        if it == 0:
            thr = (tol * tol) * P
        if tol > 0 and P <= thr:
            status = TOL
            break
        cr, ci = gain * re[p], gain * im[p]
        cre[p], cim[p] = cre[p] + cr, cim[p] + ci
        re[p], im[p] = re[p] - cr, im[p] - ci
        picks[it], pvr[it], pvi[it] = p, cr, ci
        heapq.heapreplace(heap, (-(re[p] * re[p] + im[p] * im[p]), p))
        it += 1
    return dict(R=to_complex(np.array(re), np.array(im)), C=to_complex(np.array(cre), np.array(cim)), picks=np.array(picks, dtype=np.int32).reshape(niter),
                pick_values=to_complex(np.array(pvr).reshape(niter), np.array(pvi).reshape(niter)), iterations=it, status=status, admissible=Nf - 1)


def model_as_complex(m):
    """A result of clean_model in the oracle's layout (spectra as complex arrays, admissible as a count)."""
    return dict(R=to_complex(*m["R"]), C=to_complex(*m["C"]), picks=m["picks"], pick_values=to_complex(*m["pick_values"]), iterations=m["iterations"],
                status=m["status"], admissible=int(m["admissible"].sum()))


def same_result(a, b):
    """The first key at which two results (delta_oracle's layout) differ in a byte, or None."""
    for key in ("picks", "pick_values", "C", "R"):
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            return key
    for key in ("iterations", "status", "admissible"):
        if int(a[key]) != int(b[key]):
            return key
    return None


def sidelobe_window(Nf):
    """Wn_0 = 1 with dyadic sidelobes: every admissible bin still ties at iteration 0 (den_1 = 1 - 2^-8, den_p = 1 beyond), and from
    the first pick on the update pass moves the neighbours by exact dyadic amounts."""
    Wn = delta_window(Nf)
    for m, v in ((1, complex(2.0 ** -3, 0.0)), (2, complex(0.0, -2.0 ** -4)), (5, complex(2.0 ** -6, 2.0 ** -6))):
        if m < len(Wn):
            Wn[m] = v
    return Wn


def cut_doubles():
    """(at, above, below): doubles wr near sqrt(1 - 2^-20) with den = fl(1 - fl(wr wr)) == 2^-20 exactly (None if no double gives it),
    the closest with den > 2^-20 and the closest with den < 2^-20.  1 - x is exact for x in [1/2, 1], so den == 2^-20 asks for
    fl(wr wr) == 1 - 2^-20; squares of neighbouring doubles there are 2^-52 apart, twice the spacing of the products, so about every
    other double of the products is hit: found by a search of the neighbours, nothing assumed."""
    den = lambda w: np.float64(1.0) - np.float64(w) * np.float64(w)            # noqa: E731
    w0 = np.sqrt(np.float64(1.0) - np.float64(MIN_DEN))
    near = [w0]
    lo = hi = w0
    for _ in range(64):
        lo, hi = np.nextafter(lo, 0.0), np.nextafter(hi, 2.0)
        near += [lo, hi]
    near = sorted(near)                                                        # den falls as wr grows
    at = [w for w in near if den(w) == MIN_DEN]
    above, below = [w for w in near if den(w) > MIN_DEN], [w for w in near if den(w) < MIN_DEN]
    return (float(at[0]) if at else None), float(above[-1]), float(below[0])


CUT_NF = 1023                                                                  # 256 threads: bin k is thread k mod 256's, wave (k mod 256) >> 6
CUT_BINS = {"at": (10, 330, 650), "above": (100, 420, 740), "below": (150, 470, 790)}     # k mod 256 = 10, 74, 138 / 100, 164, 228 / 150, 214, 22: three waves each


def cut_case():
    """(D [2][Nf], Wn, found): the delta window with Wn_2p at the cut, just above and just below it, each at three bins whose threads
    sit in different waves (CUT_BINS).  The bins below the cut carry the largest |D|, those at and just above it the next largest,
    so that the first picks are theirs; the rest are integers of modulus <= 3 (real: see below).  found: whether a double sits AT the cut (its
    bins then take the value just above: the other two legs stand)."""
    at, above, below = cut_doubles()
    Nf = CUT_NF
    Wn = delta_window(Nf)
    rng = np.random.default_rng(23)
    D = np.zeros((2, Nf), dtype=np.complex128)
    D.real, D.imag = rng.integers(-3, 4, (2, Nf)), rng.integers(-4, 5, (2, Nf))
    D.imag = 0.0                                                               # real: with Wn_2p real and den = 2^-20 a pick multiplies an imaginary part by 2^21
    D = D + 0.0
    for name, w in (("at", above if at is None else at), ("above", above), ("below", below)):
        for j, p in enumerate(CUT_BINS[name]):
            Wn[2 * p] = w
            D[:, p] = (9.0 + j) if name == "below" else (6.0 + j if name == "at" else 6.5 + j)
    D.setflags(write=False)
    Wn.setflags(write=False)
    return D, Wn, at is not None


def clean_sigma(Wn, df):
    """csrc/clean_plan.h clean_sigma, operation for operation."""
    Wre, Wim = Wn if isinstance(Wn, tuple) else from_complex(Wn)
    P = Wre * Wre + Wim * Wim
    df = np.float64(df)
    c = np.float64(0.8493218002880191)
    for m in range(1, len(P)):
        if P[m] < 0.5:
            frac = (P[m - 1] - 0.5) / (P[m - 1] - P[m]) if P[m - 1] > P[m] else np.float64(0.0)
            return float(((np.float64(m - 1) + frac) * df) * c)
    return float((np.float64(len(P) - 1) * df) * c)


def restore_ld(R, C, df, sigma):
    """(S as (re, im) long double, sum|terms| per entry, the number of nonzero components)."""
    Rre, Rim = (a.astype(LD) for a in (R if isinstance(R, tuple) else from_complex(R)))
    Cre, Cim = (a.astype(LD) for a in (C if isinstance(C, tuple) else from_complex(C)))
    Nf = len(Rre)
    x = (np.arange(2 * Nf - 1, dtype=np.float64) * np.float64(df)).astype(LD)
    B = np.exp(-(x * x) / (LD(2) * (LD(sigma) * LD(sigma))))
    k = np.arange(Nf)
    sre, sim, mag = Rre.copy(), Rim.copy(), np.maximum(np.abs(Rre), np.abs(Rim))
    comps = np.nonzero((Cre != 0) | (Cim != 0))[0]
    for p in comps:
        b1, b2 = B[np.abs(k - p)], B[k + p]
        sre = sre + (Cre[p] * b1 + Cre[p] * b2)
        sim = sim + (Cim[p] * b1 - Cim[p] * b2)
        mag = mag + np.maximum(np.abs(Cre[p]), np.abs(Cim[p])) * (b1 + b2)
    return (sre, sim), mag, len(comps)
