"""References for the box least squares periodogram (bls: csrc/bls.hip, csrc/bls_plan.h; include/lpvspectral.h g9).  Shared by
tests/test_bls_ref_host.py (which proves them on the CPU) and tests/test_gpu_bls.py.

bls_model     the definition as the device computes it, restated in numpy: the moments by the device's fixed trees (device_sum), YY as the
              order-free integer sum of its terms (order_free_yy), the quantisation to 64-bit integers, the fold by the exact product's phase, integer histograms and box sums, the objective in
              double from the integers in the stated order of operations, the tie rule.  Integers are compared exactly, doubles to a few ulp.
              It also reports, per (frequency, signal), the GAP between the best objective and the best one of a box with other (r, s), in ulp,
              and GAP2, which sets the boxes with the complement's sums (R - r, S - s) aside as well: with dips_only = False a box and its
              complement have bit-equal objectives, a tie the rule decides (narrowest, then earliest), and gap = 0 there by construction.
bls_ref_ld    the definition in long double straight from the samples: no quantisation, the exact phase (tests/_phase_ref.py), every
              box summed bin by bin.
bls_bounds    how far the two may differ -- derived, to first order, from the quantisation and the roundings (nothing fitted):
  u = 2^-53, ym = max |y - ybar|, a = sum w |y - ybar|, em = (N + 16) u sum w |y| (the error of the device's mean; 0 without centring);
  a box sum of wy is off by at most   es = (N + 5) u a + em + (N / 2) 2^-shy :  w_n carries the error of the tree sum W ((N + 2) u, with its
      own division), wy_n three roundings (the division, y - ybar, the product) and em, and n <= N terms are each off by half a quantum;
  a box weight r by at most           er(r) = (N + 2) u r + (N / 2) 2^-60;
  Delta = s^2 / r + sc^2 / rc - S^2 / R with |s / r|, |sc / rc|, |S / R| <= ym (weighted means of y - ybar) and r, rc, R <= 1 + er:
      |dDelta| <= B = 6 ym es + 3 ym^2 er(1) + 24 u ym^2   (the last: at most 8 roundings on each of three terms, each term <= ym^2);
  it holds for EVERY box, so the maxima of the two objectives differ by at most B, and a box that is best for one is within 2 B of the
  other's best;
  power: standard B / YY + p ((N + 19) u + 2 em a / YY) + 2 u (the device's YY: a sum of rounded products formed with its mean, itself
      within 2 u of exact -- the allowance is that of a tree sum, which covers it); chi2
      sum W B + (N + 2) u |power|;
  depth = sc / rc - s / r of the SAME box: es (1 / r + 1 / rc) + ym (er(r) / r + er(rc) / rc) + 6 u ym;
  depth_err, relative: (max(er(r) / r, er(rc) / rc) + (N + 2) u) / 2 + 4 u."""
import numpy as np

from _phase_ref import lomb_turns_exact, two_product

LD = np.longdouble
U = 2.0 ** -53
WSHIFT = 60


# ---- the device's moments (csrc/lomb.hip: lomb_scan / lomb_mean / lomb_center kernels, lomb_tree_kernel) --------------------------------------
def _tree256(v):
    v = np.array(v, dtype=np.float64)
    s = 128
    while s:
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
        s >>= 1
    return v[..., 0]


def device_sum(x):
    """The sum the moment kernels form: a pairwise tree over each slab of 256, thread t of the second kernel adds the slabs t, t + 256, ...
    in ascending order, then the same tree."""
    x = np.asarray(x, np.float64)
    nslab = -(-len(x) // 256)
    part = _tree256(np.concatenate([x, np.zeros(nslab * 256 - len(x))]).reshape(nslab, 256))
    acc = np.zeros(256)
    for i0 in range(0, nslab, 256):
        c = part[i0:i0 + 256]
        acc[:len(c)] = acc[:len(c)] + c
    return float(_tree256(acc))


def device_moments(y, W, center):
    """y: (N, ns).  -> sumW, w (N,), mean (ns,), wy (ns, N), YY (ns,), Rg (ns,) with the device's bits."""
    N, ns = y.shape
    Wv = np.ones(N) if W is None else np.asarray(W, np.float64)
    sumW = device_sum(Wv)
    w = Wv / sumW
    mean = np.array([device_sum(w * y[:, c]) for c in range(ns)])
    wy, YY, Rg = np.zeros((ns, N)), np.zeros(ns), np.zeros(ns)
    for c in range(ns):
        yc = y[:, c] - (mean[c] if center else 0.0)
        wy[c] = w * yc
        YY[c] = device_sum(wy[c] * yc)
        Rg[c] = device_sum((w * y[:, c]) * y[:, c])
    return sumW, w, mean, wy, YY, Rg


def yy_noise(N, center, Rg):
    nu = (N + 16.0) * U
    return nu * nu * Rg if center else 0.0


# ---- quantisation and fold ------------------------------------------------------------------------------------------------------------------
def log2_ceil(N):
    L = 0
    while (1 << L) < N:
        L += 1
    return L


def shift_y(A, N):
    """61 - ceil(log2 N) - (ilogb(A) + 1); frexp's exponent IS ilogb + 1."""
    return 61 - log2_ceil(N) - int(np.frexp(A)[1])


def quantise(v, shift):
    return np.rint(np.ldexp(np.asarray(v, np.float64), shift)).astype(np.int64)


def order_free_yy(v, N):
    """csrc/bls_plan.h: bls_yy_words / bls_yy.  The terms v_n = wy_n (y_n - ybar) >= 0 cut into two integer words against the largest, the
    words added as integers (Python ints here), YY = hi 2^-sv + lo 2^-(sv + 61 - L): the same bits for any order of the terms."""
    v = np.asarray(v, np.float64)
    M = v.max()
    if not M > 0:
        return 0.0
    if not np.isfinite(M):
        return np.inf
    L = log2_ceil(N)
    sv = shift_y(M, N)
    x = np.ldexp(v, sv)
    h = np.rint(x)
    hi = sum(int(a) for a in h)
    lo = sum(int(a) for a in np.rint(np.ldexp(x - h, 61 - L)))
    return float(np.ldexp(float(hi), -sv) + np.ldexp(float(lo), -(sv + 61 - L)))


def fold_bins(f, t, nbins):
    """(Nf, N) ints: the device's bins; and the products phi nbins (doubles) they are the floors of."""
    p, e = two_product(np.asarray(f, np.float64).reshape(-1)[:, None], np.asarray(t, np.float64).reshape(-1)[None, :])
    phi = (p - np.rint(p)) + e
    phi = np.where(phi < 0.0, phi + 1.0, phi)
    x = phi * float(nbins)
    return np.minimum(nbins - 1, np.floor(x).astype(np.int64)), x


def _box_sums(H, kmin, kmax):
    """H: (nbins,) -> (kmax - kmin + 1, nbins): the sums over b .. b + k - 1, wrapping (integers: from prefix sums; exact)."""
    nb = len(H)
    P = np.concatenate([np.zeros(1, H.dtype), np.cumsum(np.concatenate([H, H]))])
    return np.stack([P[k:k + nb] - P[:nb] for k in range(kmin, kmax + 1)])


def _widths(k, Nf):
    return np.broadcast_to(np.asarray(k, np.int64), (Nf,))


def bls_model(y, t, f, W=None, nbins=64, kmin=1, kmax=8, min_count=1, dips_only=True, center_data=True, normalization="standard"):
    y = np.asarray(y, np.float64)
    y = y.reshape(len(y), -1)
    N, ns = y.shape
    f = np.asarray(f, np.float64).reshape(-1)
    Nf, unit = len(f), W is None
    kmin, kmax = _widths(kmin, Nf), _widths(kmax, Nf)
    sumW, w, mean, wy, YY_tree, Rg = device_moments(y, W, center_data)
    YY = np.array([order_free_yy(wy[c] * (y[:, c] - (mean[c] if center_data else 0.0)), N) for c in range(ns)])
    A = np.abs(wy).max(axis=1)
    shy = [shift_y(a, N) if a > 0 else 0 for a in A]
    qy = np.stack([quantise(wy[c], shy[c]) if A[c] > 0 else np.zeros(N, np.int64) for c in range(ns)])
    qw = None if unit else quantise(w, WSHIFT)
    bins, _ = fold_bins(f, t, nbins)
    out = {k: np.zeros((Nf, ns)) for k in ("power", "depth", "depth_err", "gap", "gap2", "dq")}
    out.update({k: np.zeros((Nf, ns), np.int64) for k in ("start", "width", "count", "degenerate")})
    hist, hcount = np.zeros((Nf, 1 + ns, nbins), np.int64), np.zeros((Nf, nbins), np.int64)
    for k in range(Nf):
        np.add.at(hcount[k], bins[k], 1)
        if unit:
            hist[k, 0] = hcount[k]
        else:
            np.add.at(hist[k, 0], bins[k], qw)
        for c in range(ns):
            np.add.at(hist[k, 1 + c], bins[k], qy[c])
        cnt = _box_sums(hcount[k], kmin[k], kmax[k])
        r = cnt if unit else _box_sums(hist[k, 0], kmin[k], kmax[k])
        R = N if unit else int(hist[k, 0].sum())
        rc = R - r
        ok = (cnt >= min_count) & (N - cnt >= min_count) & (r > 0) & (rc > 0)
        rd, rcd = r.astype(np.float64), rc.astype(np.float64)
        for c in range(ns):
            s = _box_sums(hist[k, 1 + c], kmin[k], kmax[k])
            S = int(hist[k, 1 + c].sum())
            sc = S - s
            valid = ok.copy()
            if dips_only:
                valid &= np.array(s.astype(object) * rc.astype(object) < sc.astype(object) * r.astype(object), dtype=bool)
            sd, scd, Sd = s.astype(np.float64), sc.astype(np.float64), float(S)
            with np.errstate(all="ignore"):
                dq = ((sd * sd) / rd + (scd * scd) / rcd) - (Sd * Sd) / float(R)
            noise = yy_noise(N, center_data, Rg[c])
            live = valid.any() and A[c] > 0 and YY[c] > noise and np.isfinite(YY[c])
            if live:
                masked = np.where(valid, dq, -np.inf)
                i, b = np.unravel_index(np.argmax(masked), masked.shape)      # the first maximum in (k, b) order: narrowest, then earliest
                best = masked[i, b]
                other = valid & ~((r == r[i, b]) & (s == s[i, b]))
                second = masked[other].max() if other.any() else -np.inf
                out["gap"][k, c] = (best - second) / np.spacing(abs(best)) if best != 0 else np.inf
                # gap2: the complement of the best box, the sums (R - r, S - s), is set aside too.  Its objective has the best one's BITS
                # (the two quotients change places and the sum commutes), so that tie is the rule's to decide, exactly, not a near-tie
                other &= ~((r == R - r[i, b]) & (s == S - s[i, b]))
                second = masked[other].max() if other.any() else -np.inf
                out["gap2"][k, c] = (best - second) / np.spacing(abs(best)) if best != 0 else np.inf
                out["dq"][k, c] = best
                dpos = max(best, 0.0)
                delta = np.ldexp(dpos * float(N), -2 * shy[c]) if unit else np.ldexp(dpos, WSHIFT - 2 * shy[c])
                live = bool(np.isfinite(delta))
            if not live:
                out["degenerate"][k, c] = 1
                out["gap"][k, c] = out["gap2"][k, c] = np.inf
                continue
            rt = float(r[i, b]) / float(N) if unit else np.ldexp(float(r[i, b]), -WSHIFT)
            rct = float(rc[i, b]) / float(N) if unit else np.ldexp(float(rc[i, b]), -WSHIFT)
            out["depth"][k, c] = np.ldexp(float(sc[i, b]) / rct - float(s[i, b]) / rt, -shy[c])
            out["depth_err"][k, c] = np.sqrt((1.0 / rt + 1.0 / rct) / sumW)
            out["power"][k, c] = sumW * delta if normalization == "chi2" else min(1.0, delta / YY[c])
            out["start"][k, c], out["width"][k, c], out["count"][k, c] = b, kmin[k] + i, cnt[i, b]
    out.update(hist=hist, hcount=hcount, shy=shy, sumW=sumW, mean=mean, YY=YY, YY_tree=YY_tree, ndeg=int(out["degenerate"].sum()))
    return out


# ---- the definition in long double -----------------------------------------------------------------------------------------------------------
def ld_bins(f, t, nbins):
    phi = lomb_turns_exact(f, t)                                               # f t minus a whole number, in [-1/2, 1/2]: exact
    phi = np.where(phi < 0, phi + 1, phi)
    return np.minimum(nbins - 1, np.floor(phi * LD(nbins)).astype(np.int64)), phi


def _roll_sums(H, kmin, kmax):
    """(kmax - kmin + 1, nbins): every box summed bin by bin."""
    acc, rows = np.zeros_like(H), []
    for k in range(1, kmax + 1):
        acc = acc + np.roll(H, -(k - 1))
        if k >= kmin:
            rows.append(acc.copy())
    return np.stack(rows)


def bls_ref_ld(y, t, f, W=None, nbins=64, kmin=1, kmax=8, min_count=1, dips_only=True, center_data=True, normalization="standard", keep_table=False):
    """-> dict of (Nf, ns) arrays power, depth, depth_err, delta, r, rc (long doubles), start, width, count, none (no valid box) and, with
    keep_table, ``table``: table[k][c] = (delta, r, rc, s, sc, valid), each (widths, nbins), to evaluate any box."""
    y = np.asarray(y, np.float64)
    y = y.reshape(len(y), -1).astype(LD)
    N, ns = y.shape
    f = np.asarray(f, np.float64).reshape(-1)
    Nf = len(f)
    kmin, kmax = _widths(kmin, Nf), _widths(kmax, Nf)
    Wl = np.ones(N, LD) if W is None else np.asarray(W, np.float64).astype(LD)
    sumW = Wl.sum()
    w = Wl / sumW
    mean = (w[:, None] * y).sum(axis=0) if center_data else np.zeros(ns, LD)
    yc = y - mean
    wy = w[:, None] * yc
    YY = (wy * yc).sum(axis=0)
    bins, _ = ld_bins(f, t, nbins)
    out = {k: np.zeros((Nf, ns), LD) for k in ("power", "depth", "depth_err", "delta", "r", "rc")}
    out.update({k: np.zeros((Nf, ns), np.int64) for k in ("start", "width", "count", "none")})
    table = []
    for k in range(Nf):
        HC, HW = np.zeros(nbins, np.int64), np.zeros(nbins, LD)
        np.add.at(HC, bins[k], 1)
        np.add.at(HW, bins[k], w)
        cnt, r = _roll_sums(HC, kmin[k], kmax[k]), _roll_sums(HW, kmin[k], kmax[k])
        R = HW.sum()
        rc = R - r
        ok = (cnt >= min_count) & (N - cnt >= min_count) & (r > 0) & (rc > 0)
        row = []
        for c in range(ns):
            HY = np.zeros(nbins, LD)
            np.add.at(HY, bins[k], wy[:, c])
            s = _roll_sums(HY, kmin[k], kmax[k])
            S = HY.sum()
            sc = S - s
            with np.errstate(all="ignore"):
                delta = s * s / r + sc * sc / rc - S * S / R
                valid = ok & (s / r < sc / rc) if dips_only else ok.copy()
            if keep_table:
                row.append((delta, r, rc, s, sc, valid))
            if not valid.any():
                out["none"][k, c] = 1
                continue
            masked = np.where(valid, delta, -np.inf)
            i, b = np.unravel_index(np.argmax(masked), masked.shape)
            d = max(masked[i, b], LD(0))
            out["delta"][k, c] = d
            out["r"][k, c], out["rc"][k, c] = r[i, b], rc[i, b]
            out["depth"][k, c] = sc[i, b] / rc[i, b] - s[i, b] / r[i, b]
            out["depth_err"][k, c] = np.sqrt((1 / r[i, b] + 1 / rc[i, b]) / sumW)
            out["power"][k, c] = sumW * d if normalization == "chi2" else d / YY[c]
            out["start"][k, c], out["width"][k, c], out["count"][k, c] = b, kmin[k] + i, cnt[i, b]
        table.append(row)
    out.update(table=table, YY=YY, sumW=sumW, kmin=kmin)
    return out


def ref_at_box(one, width, start, normalization="standard"):
    """What bls_ref_ld(..., keep_table=True) of ONE frequency and signal gives for the box (width, start), not only for its best one:
    dict of valid, delta, power, depth, depth_err, r, rc (long doubles)."""
    delta, r, rc, s, sc, valid = one["table"][0][0]
    i, b = int(width - one["kmin"][0]), int(start)
    d = max(delta[i, b], LD(0))
    return dict(valid=bool(valid[i, b]), delta=delta[i, b], r=r[i, b], rc=rc[i, b], depth=sc[i, b] / rc[i, b] - s[i, b] / r[i, b],
                depth_err=np.sqrt((1 / r[i, b] + 1 / rc[i, b]) / one["sumW"]), power=one["sumW"] * d if normalization == "chi2" else d / one["YY"][0])


def bls_bounds(y, W, center_data, shy):
    """The first-order bounds of the module docstring for one call: dict of (ns,) arrays ``B`` (on Delta), ``es``, ``ym``, ``a``, ``em``,
    ``YY``, and the functions of a box's (r, rc) as methods of the returned object."""
    y = np.asarray(y, np.float64)
    y = y.reshape(len(y), -1).astype(LD)
    N, ns = y.shape
    Wl = np.ones(N, LD) if W is None else np.asarray(W, np.float64).astype(LD)
    w = Wl / Wl.sum()
    mean = (w[:, None] * y).sum(axis=0) if center_data else np.zeros(ns, LD)
    yc = y - mean
    ym, a = np.abs(yc).max(axis=0), (w[:, None] * np.abs(yc)).sum(axis=0)
    em = (N + 16) * U * (w[:, None] * np.abs(y)).sum(axis=0) if center_data else np.zeros(ns, LD)
    q = np.array([np.ldexp(1.0, -int(s)) for s in shy], LD)
    es = (N + 5) * U * a + em + (N / 2) * q
    er1 = (N + 2) * U + (N / 2) * LD(2.0) ** -60
    B = 6 * ym * es + 3 * ym * ym * er1 + 24 * U * ym * ym
    YY = (w[:, None] * yc * yc).sum(axis=0)
    return Bounds(N, float(Wl.sum()), B, es, ym, a, em, YY)


class Bounds:
    def __init__(self, N, sumW, B, es, ym, a, em, YY):
        self.N, self.sumW, self.B, self.es, self.ym, self.a, self.em, self.YY = N, sumW, B, es, ym, a, em, YY

    def _er_rel(self, r):
        return (self.N + 2) * U + (self.N / 2) * LD(2.0) ** -60 / r

    def power(self, c, p, normalization):
        if normalization == "chi2":
            return self.sumW * self.B[c] + (self.N + 2) * U * abs(p)
        return self.B[c] / self.YY[c] + abs(p) * ((self.N + 19) * U + 2 * self.em[c] * self.a[c] / self.YY[c]) + 2 * U

    def depth(self, c, r, rc):
        return self.es[c] * (1 / r + 1 / rc) + self.ym[c] * (self._er_rel(r) + self._er_rel(rc)) + 6 * U * self.ym[c]

    def depth_err_rel(self, r, rc):
        return (max(self._er_rel(r), self._er_rel(rc)) + (self.N + 2) * U) / 2 + 4 * U


# ---- the family's inputs: f t, the fold and the bin are exact ----------------------------------------------------------------------------------
def base_case(seed=0, N=1500, span=375.0, Nf=70, ns=1, depth=0.5, q=0.05, f0=1.25, sigma=0.25, bump=False):
    """t in multiples of 2^-10 over ``span``, f in multiples of 2^-6 from 1/4 (70: up to 2.40625), noise of sigma 1/4 and a dip of
    ``depth`` lasting the share q of a period at f0 that straddles phase 0 (phases in [0.97, 1) and [0, q - 0.03): at 100 bins exactly
    the bins 97, 98, 99, 0, 1); signal c > 0: the same dip at f0 + c / 4 with depth (1 + c) / 2.  bump: the box is raised, not lowered."""
    rng = np.random.default_rng(seed)
    t = np.round(rng.random(N) * span * 1024) / 1024
    f = 0.25 + np.arange(Nf) / 32.0
    y = sigma * rng.standard_normal((N, ns))
    for c in range(ns):
        ph = np.mod((f0 + c / 4.0) * t, 1.0)                                   # exact: a multiple of 2^-12 below 2^11
        inside = (ph >= 0.97) | (ph < q - 0.03)
        y[inside, c] += (depth * (1 + c) if c else depth) * (1.0 if bump else -1.0)
    return t, f, (y[:, 0] if ns == 1 else y)


COMPLEMENT_NBINS = (8, 64, 128, 256, 512)


def complement_case(weighted):
    """The inputs of the complement ties (dips_only = False, kmin = 1, widths up to nbins / 2 and, in the model, up to nbins - 1):
    base_case(N = 257, span = 64), with unit weights or W.  -> t, f, y, W or None."""
    t, f, y = base_case(seed=0, N=257, span=64.0, Nf=70, ns=1)
    W = 0.5 + np.random.default_rng(100 + 257).random(len(t)) if weighted else None
    return t, f, y, W


HALF_K = 24                                                                    # f[24] = 1


def half_case(weighted):
    """A record on which the tie DECIDES the answer at every nbins of COMPLEMENT_NBINS: 512 samples whose phases at f = 1 are
    (2 b + 1) / 1024, b = 0 .. 511 -- one in every one of 512 bins, equally many in every bin of a coarser power of two --, low over
    the phases [1/4, 3/4) and high elsewhere, under noise a twentieth of the step.  At f = 1 the best box is HALF the bins wide and
    starts at nbins / 4; its complement starts nbins / 2 further on with the same objective, bit for bit, and is among the boxes the
    device searches (widths up to nbins / 2).  Asserted on the model by tests/test_bls_ref_host.py.  -> t, f, y, W or None."""
    rng = np.random.default_rng(12)
    b = np.arange(512)
    t = rng.integers(0, 64, 512) + (2 * b + 1) / 1024.0
    f = 0.25 + np.arange(70) / 32.0
    y = np.where((b >= 128) & (b < 384), -1.0, 1.0) + 0.05 * rng.standard_normal(512)
    perm = rng.permutation(512)
    W = 0.5 + rng.random(512) if weighted else None
    return t[perm], f, y[perm], W
