"""References for the fold statistics (pdm / aov, conditional_entropy: csrc/fold.hip, csrc/fold_plan.h; include/lpvspectral.h g10).
Shared by tests/test_fold_ref_host.py (which proves them on the CPU) and tests/test_gpu_fold.py.

pdm_model / cent_model     the definition as the device computes it, restated in numpy: the moments, the quantisation and the fold of
                           tests/_bls_ref.py, integer histograms and coarse-bin sums (int64: every subset sum stays below 2^61), then the
                           double arithmetic of fold_plan.h in ITS order (device_order_sum: thread tid adds its terms tid, tid + 256, ...
                           ascending, a tree over each wave of 64, the four wave sums as (W0 + W1) + (W2 + W3)).
pdm_ref_ld / cent_ref_ld   the definition in long double from the unquantised record: the exact phase (tests/_phase_ref.py), every coarse
                           bin summed fine bin by fine bin.

BOUNDS (u = 2^-53; nothing is fitted to the device).
Device against model.  Integers (hist, hcount, nonempty, degenerate, the value bins through hist, ylim) are equal.
  explained: device and model do the same IEEE operations in the same order, so they agree unless the compiler contracts a product and
    a sum.  The roundings on the way, each 2^-53 of its operand: per term two conversions, a product and a quotient (4); on any path of the
    sum A = ceil(nfine / 256) + 8 additions of non-negative terms; the division by covers (1); S S / R (three conversions, a product, a
    quotient: 5); the subtraction (1); the scaling by N (1); the quotient by YY (1) -- PDM_ULPS(nfine) = 13 + A in all.  The terms before
    the subtraction are as large as ``gross`` = the pooled sum over YY, so the allowance is PDM_ULPS u max(gross, explained): absolute
    where S S / R cancels most of the sum (center_data = False), relative otherwise.
  entropy: per side a quotient (1), the log (2: the device's and numpy's are each within 2 ulp), a product (1), A = ceil(cells / 256) + 8
    additions and the division by N (1): 5 + A.  log(x (1 + d)) moves by d whatever x, so a term n_ij log(..) moves by n_ij d and the sum
    over N by at most d: that part is ABSOLUTE.  With both sides: |H_dev - H_model| <= CENT_C(cells) u (1 + H), CENT_C = 2 (5 + A).
Device against long double.
  pdm, in the manner of tests/_bls_ref.py: bls_bounds.  A coarse-bin sum of wy is off by es_m, of the weights by er(r_m), and
    d(s^2 / r) = 2 (s / r) ds - (s / r)^2 dr with |s / r| <= ym.  Every sample lies in exactly ``covers`` coarse bins, so
    sum_m es_m <= covers es and sum_m er(r_m) <= covers er(1) (es, er(1): the whole-record bounds of bls_bounds: (N + 5) u a + em +
    (N / 2) 2^-shy and (N + 2) u + (N / 2) 2^-60), and the division by covers takes the factor back; S S / R adds the same again:
        |dSB| <= B = 4 ym es + 2 ym^2 er(1) + PDM_ULPS u ym^2     (each term of the sum is at most ym^2 r_m, the sum / covers at most ym^2)
    explained: B / YY + p ((N + 19) u + 2 em a / YY) + 2 u, as bls's standard power.
  cent: the counts are exact (integers), so only the epilogue differs: the same CENT_C u (1 + H)."""
import numpy as np

from _bls_ref import LD, U, WSHIFT, bls_bounds, device_moments, fold_bins, ld_bins, order_free_yy, quantise, shift_y, yy_noise


def device_order_sum(terms):
    """terms: (..., n) non-negative doubles -> (...): the sum in the order of csrc/fold_plan.h."""
    terms = np.asarray(terms, np.float64)
    n = terms.shape[-1]
    nch = -(-n // 256)
    pad = np.zeros(terms.shape[:-1] + (nch * 256 - n,))
    v = np.concatenate([terms, pad], axis=-1).reshape(terms.shape[:-1] + (nch, 256))
    acc = np.zeros(terms.shape[:-1] + (256,))
    for ch in range(nch):
        acc = acc + v[..., ch, :]
    w = acc.reshape(terms.shape[:-1] + (4, 64)).copy()
    off = 32
    while off:
        w[..., :off] = w[..., :off] + w[..., off:2 * off]
        off >>= 1
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def pdm_ulps(nfine):
    return 13 + (-(-nfine // 256) + 8)


def cent_c(cells):
    return 2 * (5 + (-(-cells // 256) + 8))


def _coarse(H, covers):
    """H: (..., nfine) integers -> the sums over m .. m + covers - 1, wrapping (exact)."""
    n = H.shape[-1]
    P = np.concatenate([np.zeros(H.shape[:-1] + (1,), H.dtype), np.cumsum(np.concatenate([H, H], axis=-1), axis=-1)], axis=-1)
    return P[..., covers:covers + n] - P[..., :n]


def pdm_model(y, t, f, W=None, nbins=10, covers=1, center_data=True):
    y = np.asarray(y, np.float64)
    y = y.reshape(len(y), -1)
    N, ns = y.shape
    f = np.asarray(f, np.float64).reshape(-1)
    Nf, unit, nfine = len(f), W is None, nbins * covers
    sumW, w, mean, wy, YY_tree, Rg = device_moments(y, W, center_data)
    YY = np.array([order_free_yy(wy[c] * (y[:, c] - (mean[c] if center_data else 0.0)), N) for c in range(ns)])
    A = np.abs(wy).max(axis=1)
    shy = [shift_y(a, N) if a > 0 else 0 for a in A]
    qy = np.stack([quantise(wy[c], shy[c]) if A[c] > 0 else np.zeros(N, np.int64) for c in range(ns)])
    qw = None if unit else quantise(w, WSHIFT)
    bins, _ = fold_bins(f, t, nfine)
    hist, hcount = np.zeros((Nf, 1 + ns, nfine), np.int64), np.zeros((Nf, nfine), np.int64)
    for k in range(Nf):
        hcount[k] = np.bincount(bins[k], minlength=nfine)
        if unit:
            hist[k, 0] = hcount[k]
        else:
            np.add.at(hist[k, 0], bins[k], qw)
        for c in range(ns):
            np.add.at(hist[k, 1 + c], bins[k], qy[c])
    r = _coarse(hcount if unit else hist[:, 0], covers)                        # (Nf, nfine)
    Rtot = np.full(Nf, N, np.int64) if unit else hist[:, 0].sum(axis=1)
    has = r > 0
    M = has.sum(axis=1)
    bins_ok = (M > covers) & (covers * N > M)
    rd = np.where(has, r, 1).astype(np.float64)
    out = dict(explained=np.zeros((Nf, ns)), gross=np.zeros((Nf, ns)), degenerate=np.zeros((Nf, ns), np.int64))
    for c in range(ns):
        s = _coarse(hist[:, 1 + c], covers)
        sd = s.astype(np.float64)
        terms = np.where(has, (sd * sd) / rd, 0.0)
        tot = device_order_sum(terms)
        Sd = hist[:, 1 + c].sum(axis=1).astype(np.float64)
        with np.errstate(all="ignore"):
            pooled = tot / float(covers)
            sb = pooled - (Sd * Sd) / Rtot.astype(np.float64)
            dpos = np.where(sb > 0.0, sb, 0.0)
            if unit:
                delta, gross = np.ldexp(dpos * float(N), -2 * shy[c]), np.ldexp(pooled * float(N), -2 * shy[c])
            else:
                delta, gross = np.ldexp(dpos, WSHIFT - 2 * shy[c]), np.ldexp(pooled, WSHIFT - 2 * shy[c])
            live = bins_ok & (A[c] > 0) & (YY[c] > yy_noise(N, center_data, Rg[c])) & np.isfinite(YY[c]) & np.isfinite(delta)
            out["explained"][:, c] = np.where(live, np.minimum(1.0, delta / YY[c]), 0.0)
            out["gross"][:, c] = np.where(live, gross / YY[c], 0.0)
        out["degenerate"][:, c] = ~live
    out.update(hist=hist, hcount=hcount, nonempty=M, shy=shy, YY=YY, sumW=sumW, ndeg=int(out["degenerate"].sum()))
    return out


def theta_of(explained, M, N, covers, degenerate):
    """What the Python layer forms from the device's outputs.  explained, degenerate: (Nf, ns); M: (Nf,)."""
    M = np.asarray(M, np.float64)[:, None]
    with np.errstate(all="ignore"):
        return np.where(degenerate != 0, 1.0, (1.0 - explained) * (covers * (N - 1.0)) / (covers * float(N) - M))


def aov_of(explained, M, N, degenerate):
    M = np.asarray(M, np.float64)[:, None]
    with np.errstate(all="ignore"):
        return np.where(degenerate != 0, 0.0, np.where(explained < 1.0, explained / (1.0 - explained) * (N - M) / (M - 1.0), np.inf))


def pdm_ref_ld(y, t, f, W=None, nbins=10, covers=1, center_data=True):
    """-> dict of (Nf, ns) long doubles ``explained`` (not clamped to 1), ``SB``; ``nonempty`` (Nf,); ``YY`` (ns,)."""
    y = np.asarray(y, np.float64)
    y = y.reshape(len(y), -1).astype(LD)
    N, ns = y.shape
    f = np.asarray(f, np.float64).reshape(-1)
    Nf, nfine = len(f), nbins * covers
    Wl = np.ones(N, LD) if W is None else np.asarray(W, np.float64).astype(LD)
    w = Wl / Wl.sum()
    mean = (w[:, None] * y).sum(axis=0) if center_data else np.zeros(ns, LD)
    yc = y - mean
    wy = w[:, None] * yc
    YY = (wy * yc).sum(axis=0)
    bins, _ = ld_bins(f, t, nfine)
    SB, M = np.zeros((Nf, ns), LD), np.zeros(Nf, np.int64)
    for k in range(Nf):
        HW = np.zeros(nfine, LD)
        np.add.at(HW, bins[k], w)
        HC = np.bincount(bins[k], minlength=nfine)
        r, cnt = np.zeros(nfine, LD), np.zeros(nfine, np.int64)
        for j in range(covers):
            r, cnt = r + np.roll(HW, -j), cnt + np.roll(HC, -j)
        has = r > 0
        M[k] = has.sum()
        for c in range(ns):
            HY = np.zeros(nfine, LD)
            np.add.at(HY, bins[k], wy[:, c])
            s = np.zeros(nfine, LD)
            for j in range(covers):
                s = s + np.roll(HY, -j)
            SB[k, c] = (s[has] * s[has] / r[has]).sum() / covers - HY.sum() ** 2 / HW.sum()
    with np.errstate(all="ignore"):
        explained = np.where(YY > 0, np.maximum(SB, 0) / np.where(YY > 0, YY, 1), 0)
    return dict(explained=explained, SB=SB, nonempty=M, YY=YY)


def pdm_bounds(y, W, center_data, shy, nfine, explained):
    """(Nf, ns) long doubles: how far the device's ``explained`` may lie from pdm_ref_ld's (module docstring)."""
    bd = bls_bounds(y, W, center_data, shy)
    N = bd.N
    er1 = (N + 2) * U + (N / 2) * LD(2.0) ** -60
    B = 4 * bd.ym * bd.es + 2 * bd.ym * bd.ym * er1 + pdm_ulps(nfine) * U * bd.ym * bd.ym
    return B / bd.YY + np.abs(explained) * ((N + 19) * U + 2 * bd.em * bd.a / bd.YY) + 2 * U


# ---- conditional entropy -------------------------------------------------------------------------------------------------------------------------
def value_bins(y, mbins):
    """y: (N, ns) doubles -> (N, ns) ints, ylim (ns, 2), degenerate (ns,), and u mbins (the doubles the bins are the floors of)."""
    ymin, ymax = y.min(axis=0), y.max(axis=0)
    den = ymax - ymin
    ok = (den > 0) & np.isfinite(den)
    with np.errstate(all="ignore"):
        x = np.where(ok, ((y - ymin) / np.where(ok, den, 1.0)) * float(mbins), 0.0)
    j = np.clip(np.floor(x), 0, mbins - 1).astype(np.int64)
    return j, np.stack([ymin, ymax], axis=1), ~ok, x


def _counts(bins, j, nbins, mbins):
    """bins: (Nf, N), j: (N, ns) -> (Nf, ns, nbins, mbins) int64."""
    Nf, ns = bins.shape[0], j.shape[1]
    H = np.zeros((Nf, ns, nbins * mbins), np.int64)
    for k in range(Nf):
        for c in range(ns):
            H[k, c] = np.bincount(bins[k] * mbins + j[:, c], minlength=nbins * mbins)
    return H.reshape(Nf, ns, nbins, mbins)


def cent_model(y, t, f, nbins=10, mbins=5):
    y = np.asarray(y, np.float64)
    y = y.reshape(len(y), -1)
    N, ns = y.shape
    f = np.asarray(f, np.float64).reshape(-1)
    j, ylim, deg, x = value_bins(y, mbins)
    bins, _ = fold_bins(f, t, nbins)
    H = _counts(bins, j, nbins, mbins)
    rows = np.broadcast_to(H.sum(axis=3, keepdims=True), H.shape)
    has = H > 0
    with np.errstate(all="ignore"):
        q = rows.astype(np.float64) / np.where(has, H, 1).astype(np.float64)
        terms = np.where(has, H.astype(np.float64) * np.log(np.where(has, q, 1.0)), 0.0)
    tot = device_order_sum(terms.reshape(len(f), ns, nbins * mbins))
    return dict(entropy=tot / float(N), hist=H.astype(np.int32), ylim=ylim, degenerate=deg.astype(np.int64), vbin=j, x=x)


def cent_ref_ld(y, t, f, nbins=10, mbins=5):
    """-> (Nf, ns) long doubles: H = sum p_ij ln(p_i / p_ij) from the record, value bins and phases in long double."""
    y = np.asarray(y, np.float64)
    y = y.reshape(len(y), -1).astype(LD)
    N, ns = y.shape
    f = np.asarray(f, np.float64).reshape(-1)
    ymin, ymax = y.min(axis=0), y.max(axis=0)
    den = ymax - ymin
    ok = den > 0
    j = np.clip(np.floor((y - ymin) / np.where(ok, den, 1) * mbins), 0, mbins - 1).astype(np.int64)
    j[:, ~ok] = 0
    bins, _ = ld_bins(f, t, nbins)
    H = _counts(bins, j, nbins, mbins).astype(LD)
    p = H / N
    pi = np.broadcast_to(p.sum(axis=3, keepdims=True), p.shape)
    has = H > 0
    return np.where(has, p * np.log(np.where(has, pi / np.where(has, p, 1), 1)), 0).sum(axis=(2, 3))


def cent_bound(cells, H):
    return cent_c(cells) * U * (1.0 + np.abs(np.asarray(H, LD)))


# ---- the planted period: a sawtooth, which neither a sinusoid nor a box describes ---------------------------------------------------------------
def sawtooth_case(seed=0, N=1500, f0=1.25, sigma=0.25):
    """t of base_case, y = the phase of f0 t in [0, 1) (a sawtooth of unit height) plus noise; the grid: the 55 frequencies of base_case
    from 0.71875 on, so that neither f0 / 2 nor 2 f0 is on it (a sub-harmonic folds as cleanly and would tie)."""
    from _bls_ref import base_case
    t, f, _ = base_case(seed=seed, N=N)
    rng = np.random.default_rng(seed + 77)
    y = np.mod(f0 * t, 1.0) + sigma * rng.standard_normal(N)
    f = f[f >= 0.71875]
    assert len(f) == 55 and f0 in f and f0 / 2 not in f and 2 * f0 not in f
    return t, f, y


# ---- the cases of tests/test_gpu_fold.py (tests/test_fold_ref_host.py proves the references on the same ones) ------------------------------------
# pdm: name -> (N, Nf, nbins, covers, ns, weighted, center_data, (F, TS, passes)); the plan follows csrc/fold_plan.h:
#   LDS = F nfine ((ts + weighted) 8 + 4) <= 63 KiB, ts the smallest of 1, 2, 4 that holds ns, F = 4 halved while fewer than 256 workgroups
PDM_CASES = {
    "n1": (1, 1, 2, 1, 1, False, True, (1, 1, 1)),
    "n255w": (255, 70, 5, 2, 3, True, False, (1, 4, 1)),
    "base10": (1500, 70, 10, 1, 1, False, True, (1, 1, 1)),
    "n256w": (256, 70, 100, 1, 5, True, True, (1, 4, 2)),
    "n257f4": (257, 1030, 8, 4, 2, False, False, (4, 2, 1)),
    "fine2048": (1500, 1030, 512, 4, 1, False, True, (2, 1, 1)),              # 4 x 2048 x 12 = 98304 > 64512
    "fine2048w": (1500, 70, 512, 4, 3, True, True, (1, 2, 2)),                # four signals: 2048 x 44 = 90112 > 64512; two: 57344
    "f4w": (1500, 1030, 10, 1, 3, True, True, (4, 4, 1)),
}
# cent: name -> (N, Nf, nbins, mbins, ns, (F, TS, passes, copies)): LDS = F copies ts cells 4 <= 63 KiB; one copy unless the knob asks for more
CENT_CASES = {
    "n1": (1, 1, 2, 2, 1, (1, 1, 1, 1)),
    "base10x5": (1500, 70, 10, 5, 1, (1, 1, 1, 1)),
    "n255f4": (255, 1030, 20, 8, 3, (4, 4, 1, 1)),
    "n256": (256, 1030, 64, 64, 5, (1, 2, 3, 1)),                             # four signals: 4 x 4096 x 4 = 65536 > 64512
    "n257": (257, 70, 256, 32, 1, (1, 1, 1, 1)),
    "f2": (1500, 1030, 64, 64, 1, (2, 1, 1, 1)),                              # F = 4: 65536 > 64512
    "cells400": (1500, 1030, 20, 20, 3, (4, 4, 1, 1)),                        # (with the knob at 4: 102400 > 64512, two copies: 51200)
}


def case_inputs(N, Nf, ns, weighted):
    """The family's inputs (tests/_bls_ref.py: base_case): f t, the fold and phi n are exact for every n <= 2048."""
    from _bls_ref import base_case
    t, f, y = base_case(seed=0, N=N, span=375.0 if N >= 1000 else 64.0, Nf=70, ns=ns)
    if Nf == 1:
        f = f[32:33]
    elif Nf != 70:
        f = 0.25 + np.arange(Nf) / 64.0
    W = 0.5 + np.random.default_rng(100 + N).random(N) if weighted else None
    return t, f, y, W
