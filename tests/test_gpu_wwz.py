"""wwz on the GPU against tests/_wwz_ref.py: every cell is tests/_lomb_ref.lomb_ref of its own slice under the Gaussian weights (the
reference's own check against Foster's formulation: tests/test_wwz_ref_host.py).

INPUTS follow tests/test_gpu_lomb.py: t and tau in multiples of 2^-10 (below 2^9), f in multiples of 2^-6 in [1/4, 3]: every product
f t and every difference t - tau is exact in double.  70 frequencies (two tiles), 9 times from 2 % before to 2 % beyond a record of 375
units.  Cases: NARROW (1500 samples, c = 1/(8 pi^2), wmin = 1e-9: cells from empty to a few hundred samples), WIDE (3000 samples,
c = 1/(512 pi^2): cells up to the whole record, across the stage of 256 and the slab of 1024), WHOLE (1500 samples, c = 1/(128 pi^2),
wmin = 0: every cell is the record) and records of 255, 256, 257, 1024 and 1025 samples with wmin = 0 (the block and slab edges).

One case more, LATE, has inexact products: the same lattice over [0, 2^20] and full-mantissa frequencies in (0, 3] (tests/_lomb_ref.py).

BOUNDS (u = 2^-53, n = the cell's samples).  The sums and the epilogue are held to the bounds of tests/test_gpu_lomb.py with N := n
(its helpers are imported as they are): (n + 16) u sum|terms| plus the trigonometry allowance, to first order through the epilogue by the
reference's D.  (The device adds per sample lane, (0 + 1) + (2 + 3), then per slab in a pairwise tree, and divides by sum W g at the end:
at most n / 4 + 14 roundings on a sum and as many on sum W g, together within (n + 16) u for n >= 8.)  One allowance is added, derived
and not fitted -- the weight.  With d = t - tau exact and x = a_k d^2, the device's g~ = exp(-fl(a_k fl(d^2))): two roundings in the
exponent, 2 u x, which exp amplifies by x itself -- x <= ln(1 / wmin) = 20.7 where a radius cuts the cell -- one ulp (2 u) of exp, u for
the product with W, and u for the reference's rounding of W g to double: every weight moves by at most T_n = (2 x_n + 4) u of itself.
Through the normalisation w_n = W_n g_n / sum W g, as the taper allowance of tests/test_gpu_lomb_windows.py:
    |dw_n| <= w_n T_n + w_n Tbar,  Tbar = sum w_m T_m,   hence
    C, S, C2, S2: 2 Tbar;    Y, YC, YS: sum w T |yc| + Tbar sum w |yc|;    YY: sum w T yc^2 + Tbar sum w yc^2.
(Weights that underflow carry an absolute error below 2^-1074 each: nothing next to these.)  The device removes the RECORD's mean and the
reference is given that mean to remove, so both sum the same centred signal up to the mean's own rounding, under which every compared
quantity is invariant (the fitted constant absorbs it; the argument of tests/test_gpu_lomb_windows.py).
    amplitude:  (|a| da + |b| db) / A + 4 u A.
    Neff = S1^2 / S2:  dNeff / Neff <= 2 ((n + 16) u + Tbar) + ((n + 17) u + 2 Tbar2) + 3 u,  Tbar2 = sum (W g)^2 T / S2.
    wwz:  (Neff - 3) / 2 [dp / (YY - p) + p (dYY + dp) / (YY - p)^2] + wwz dNeff / (Neff - 3),  dp and dYY those of the epilogue bounds.
NOT compared are cells with fewer than 8 samples, a reference D < 0.01 or Neff within 0.05 of 3: they have to be finite (wwz: not NaN)
with power in [-b, 1 + b], and they may be at most 10 % of a case's non-empty cells (asserted).

MEASURED (MI355X, worst error / bound over all cases): power 0.016, amplitude 0.013, wwz 0.013, a 0.016, b 0.014, c 0.032, neff 0.040 --
the bounds are worst-case in n, the errors a few ulps."""
import functools

import numpy as np
import pytest

from _lomb_ref import LATE_SPAN, LD, wide_freqs
from _wwz_ref import decay, radius, reach, wwz_cell_ref
from test_gpu_lomb import U, _epilogue_bounds, _ratio, _sum_bounds

pytestmark = pytest.mark.gpu
NF, NTAU, NS, SPAN = 70, 9, 5, 375
C_FOSTER = 1.0 / (8.0 * np.pi ** 2)
# case -> (samples, c, wmin, the record's span)
CASES = {"narrow": (1500, C_FOSTER, 1e-9, SPAN), "wide": (3000, 1.0 / (512.0 * np.pi ** 2), 1e-9, SPAN), "whole": (1500, 1.0 / (128.0 * np.pi ** 2), 0.0, SPAN)}
for _n in (255, 256, 257, 1024, 1025):
    CASES[f"edge{_n}"] = (_n, 1.0 / (128.0 * np.pi ** 2), 0.0, 64 if _n < 1000 else 256)       # (four samples per unit, as the others)
# LATE: every product f t inexact (tests/_lomb_ref.py).  t and tau stay multiples of 2^-10 (t - tau is exact) but span [0, 2^20], f are
# full-mantissa doubles in (0, 3]: f t reaches 3e6 turns.  c = 1 / (2^40 pi^2) makes the Gaussian a tenth of the record wide at f = 3 and
# flat at the low frequencies; wmin = 0, so every cell is the record (two slabs).  6 u of trigonometry per term (tests/test_gpu_lomb.py).
CASES["late"] = (1500, 1.0 / (2.0 ** 40 * np.pi ** 2), 0.0, LATE_SPAN)
KEYS = ("power", "amplitude", "wwz", "a", "b", "c", "neff")


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _record(N, offset=0.0, span=SPAN):
    rng = np.random.default_rng(7000 + N)
    t = np.sort(rng.integers(0, span * 1024, N)) / 1024.0
    y = np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(NS)[None, :]) * (1.0 + np.arange(NS))[None, :] + 0.5 * rng.standard_normal((N, NS)) + 0.75 + offset
    W = rng.uniform(0.5, 2.0, N)
    for a in (t, y, W):
        a.setflags(write=False)
    return t, y, W


@functools.lru_cache(maxsize=None)
def _freqs(case=None):
    if case == "late":
        f = wide_freqs(np.random.default_rng(7070), NF)
        f.setflags(write=False)
        return f
    f = np.sort(np.random.default_rng(70).choice(np.arange(16, 193), NF, replace=False)) / 64.0      # [1/4, 3] in steps of 2^-6
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _taus(span=SPAN):
    """From 2 % before to 2 % beyond the record, in multiples of 1/4 (span 375: -7.5, 41.25, ..., 382.5)."""
    tau = np.rint(4 * (-0.02 * span + np.arange(NTAU) * (1.04 * span / (NTAU - 1)))) / 4
    tau.setflags(write=False)
    return tau


def _record_mean(y, W):
    """The record's weighted mean (weights W) as doubles: what the device removes, up to its own rounding."""
    Wl = np.ones(len(y), dtype=LD) if W is None else W.astype(LD)
    return ((Wl[:, None] * y.astype(LD)).sum(axis=0) / Wl.sum()).astype(np.float64)


# ---- reference and bounds ----------------------------------------------------------------------------------------------------------------
def _cell_bounds(ref, ys, ts, trig=4):
    """Bounds of every compared quantity of one cell, all NS signals, from the reference alone."""
    r, n = ref["fit"], ref["count"]
    b = _sum_bounds(r, ts, ys, ref["Wg"], False, trig=trig)
    Wgl = ref["Wgl"]
    w = Wgl / Wgl.sum()
    T = (2 * ref["x"] + 4) * U
    tw = w * T
    Tbar = tw.sum()
    yc = ys.astype(LD) - r["removed"][None, :]
    for k in ("C", "S", "C2", "S2"):
        b[k] = b[k] + 2 * Tbar
    tY = (tw[:, None] * np.abs(yc)).sum(axis=0) + Tbar * (w[:, None] * np.abs(yc)).sum(axis=0)
    for k in ("YC", "YS"):
        b[k] = b[k] + tY[:, None]
    b["Y"] = b["Y"] + tY
    b["YY"] = b["YY"] + (tw[:, None] * yc * yc).sum(axis=0) + Tbar * (w[:, None] * yc * yc).sum(axis=0)
    be = {k: v[0] for k, v in _epilogue_bounds(r, b, True, False, n).items()}
    with np.errstate(all="ignore"):
        dp = _epilogue_bounds(r, b, True, True, n)["power"][0] * 2 / n         # (the psd power is p n / 2)
        dYY = b["YY"] + 2 * np.abs(r["Y"]) * b["Y"]
        A = ref["amplitude"]
        be["amplitude"] = (np.abs(ref["a"]) * be["a"] + np.abs(ref["b"]) * be["b"]) / np.where(A > 0, A, LD(1)) + 4 * U * A
        Tbar2 = (Wgl * Wgl * T).sum() / (Wgl * Wgl).sum()
        neff = ref["neff"]
        dneff = neff * (2 * ((n + 16) * U + Tbar) + ((n + 17) * U + 2 * Tbar2) + 3 * U)
        rest, p = ref["YYf"] - ref["p"], ref["p"]
        dz = (neff - 3) / 2 * (dp / rest + p * (dYY + dp) / (rest * rest)) + ref["wwz"] * dneff / (neff - 3)
        be["wwz"] = dz if neff > 3 else 0 * dz                                 # (Neff <= 3: wwz is exactly 0 on both sides)
    be["neff"] = dneff + 0 * be["power"]
    return be


@functools.lru_cache(maxsize=None)
def _refs(case, with_W, center, offset=0.0):
    """[k][j] -> None (an empty cell) or (reference, bounds), all NS signals; and the counts (NF, NTAU)."""
    N, c, wmin, span = CASES[case]
    t, y, W = _record(N, offset, span)
    W = W if with_W else None
    f, tau = _freqs(case), _taus(span)
    a, r = decay(c, f), radius(f, c, wmin)
    removed = _record_mean(y, W) if center else None
    cells, counts = [], np.zeros((NF, NTAU), dtype=np.int64)
    for k in range(NF):
        row = []
        for j in range(NTAU):
            ref = wwz_cell_ref(y, t, W, f[k], tau[j], a[k], r[k], center=center, removed=removed)
            counts[k, j] = reach(t, tau[j], r[k])[1]
            if ref is None:
                row.append(None)
                continue
            sl = slice(ref["start"], ref["start"] + ref["count"])
            row.append((ref, _cell_bounds(ref, y[sl], t[sl], 6 if case == "late" else 4)))
        cells.append(row)
    return cells, counts


def _compared(ref):
    return ref["count"] >= 8 and not ref["degenerate"] and ref["fit"]["D"][0] >= 0.01 and abs(ref["neff"] - 3) >= 0.05


def _compare(got, cells, ns):
    """got: dict over KEYS of (NF, NTAU, ns) arrays (neff: (NF, NTAU)).  -> the worst error / bound per key."""
    worst = {k: 0.0 for k in KEYS}
    live = skipped = 0
    for k in range(NF):
        for j in range(NTAU):
            vals = {q: (np.asarray(got[q])[k, j] if q == "neff" else np.asarray(got[q]).reshape(NF, NTAU, ns)[k, j]) for q in KEYS}
            if cells[k][j] is None:
                assert all(np.all(v == 0.0) for v in vals.values()), f"cell ({k}, {j}): an empty cell gives exact zeros"
                continue
            ref, be = cells[k][j]
            live += 1
            assert all(np.all(np.isfinite(v)) for q, v in vals.items() if q != "wwz") and not np.any(np.isnan(vals["wwz"])), (k, j)
            if not _compared(ref):
                skipped += 1
                if ref["degenerate"]:                                          # (D <= 2^-40: one or two samples, or collinear columns)
                    assert all(np.all(v == 0.0) for q, v in vals.items() if q != "neff"), (k, j)
                    continue
                bnd = be["power"][:ns].astype(np.float64)
                ok = np.isfinite(bnd)
                assert np.all(vals["power"][ok] >= -bnd[ok]) and np.all(vals["power"][ok] <= 1.0 + bnd[ok]), (k, j)
                continue
            for q in KEYS:
                want, bnd = (ref[q], be[q][0]) if q == "neff" else (ref[q][:ns], be[q][:ns])
                err = np.abs(vals[q].astype(LD) - want)
                ratio = _ratio(np.atleast_1d(err), np.atleast_1d(bnd))
                worst[q] = max(worst[q], ratio)
                assert np.all(err <= bnd), (q, k, j, ratio, ref["count"], float(ref["neff"]))
    assert live > 0 and skipped <= 0.1 * live, f"{skipped} of {live} non-empty cells are not compared"
    print(f"compared {live - skipped} of {live} non-empty cells; worst error / bound:", {k: round(v, 4) for k, v in worst.items()})
    return worst


def _call(L, case, ns, with_W, center, offset=0.0, tau=None, signals=None):
    N, c, wmin, span = CASES[case]
    t, y, W = _record(N, offset, span)
    ys = y[:, signals] if signals is not None else (y[:, :ns] if ns > 1 else y[:, 0])
    R, (a, b, cc) = L.wwz(ys, t, _freqs(case), tau=_taus(span) if tau is None else tau, c=c, wmin=wmin, W=W if with_W else None, center_data=center, coef=True)
    return R, {"power": R.power, "amplitude": R.amplitude, "wwz": R.wwz, "a": a, "b": b, "c": cc, "neff": R.neff}


def _check(L, case, ns, with_W, center, offset=0.0):
    R, got = _call(L, case, ns, with_W, center, offset)
    cells, counts = _refs(case, with_W, center, offset)
    shape = (NF, NTAU) if ns == 1 else (NF, NTAU, ns)
    assert R.power.shape == shape and R.wwz.shape == shape and R.amplitude.shape == shape and R.neff.shape == (NF, NTAU)
    assert np.array_equal(R.freq, _freqs(case)) and np.array_equal(R.time, _taus(CASES[case][3]))
    assert np.array_equal(R.counts, counts), "the samples in reach are numpy's searchsorted on the stated edges"
    assert np.array_equal(R.empty, [[cells[k][j] is None for j in range(NTAU)] for k in range(NF)])
    return R, got, _compare(got, cells, ns)


# ---- 1  every cell against the reference -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,ns,with_W,center", [
    ("narrow", 5, True, True), ("narrow", 1, False, True), ("narrow", 3, True, False),
    ("wide", 5, True, True), ("wide", 1, True, False),
    ("whole", 3, False, True), ("whole", 1, True, True),
    ("edge255", 1, True, True), ("edge256", 3, True, True), ("edge257", 1, True, True), ("edge1024", 1, True, True), ("edge1025", 5, True, True),
])
def test_every_cell_against_the_reference(L, case, ns, with_W, center):
    """1, 3 and 5 signals are the kernels <TT = 4, ts = 1> and <2, 4> with one and two blocks of four; 70 frequencies two tiles."""
    _check(L, case, ns, with_W, center)


def test_every_cell_late_in_a_long_record(L):
    """Every product f t inexact, up to 3e6 turns: the low word of lomb_sincos in the wwz kernels decides."""
    R, got, worst = _check(L, "late", 3, True, True)
    assert not R.empty.any() and R.counts.min() == 1500


# ---- 2  ranges, empty cells, Neff <= 3, the timing record ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["narrow", "wide"])
def test_ranges_empty_cells_and_the_counters(L, case):
    R, got = _call(L, case, 1, True, True)
    cells, counts = _refs(case, True, True)
    tm = L.wwz_last_timing()
    empty = np.array([[cells[k][j] is None for j in range(NTAU)] for k in range(NF)])
    assert np.array_equal(R.counts, counts) and np.array_equal(R.empty, empty)
    if case == "narrow":
        assert empty.sum() > 50 and counts.max() < 400                         # high frequencies at the times outside the record
    else:
        assert counts.max() == 3000 and counts.min() > 0                       # across the stage and the slab more than once
    for q in KEYS:
        assert np.all(np.asarray(got[q])[empty] == 0.0), q
    refs = [cells[k][j][0] for k in range(NF) for j in range(NTAU) if cells[k][j] is not None]
    for r in refs:
        D, scale = r["fit"]["D"][0], (r["fit"]["CC"][0] + r["fit"]["SS"][0] + r["fit"]["C"][0] ** 2 + r["fit"]["S"][0] ** 2)
        assert r["degenerate"] and D <= 2.0 ** -45 * scale ** 2 or not r["degenerate"] and D >= 2.0 ** -35 * scale ** 2, "the inputs stay clear of the threshold"
    assert (tm["nf"], tm["ntau"], tm["tt"], tm["ts"], tm["slab"]) == (NF, NTAU, 4, 1, 1024)
    assert tm["empty"] == int(empty.sum()) and tm["degenerate"] == sum(r["degenerate"] for r in refs)
    assert tm["useful"] == float(counts.sum()) and tm["staged"] >= tm["useful"] and tm["items"] >= 1
    # Neff <= 3: no degrees of freedom left
    neff_ref = np.array([[float(cells[k][j][0]["neff"]) if cells[k][j] is not None else 0.0 for j in range(NTAU)] for k in range(NF)])
    assert np.all(R.wwz[R.neff <= 3.0] == 0.0) and np.all(R.wwz[~empty & (neff_ref <= 2.95)] == 0.0)
    if case == "narrow":
        assert np.any(~empty & (neff_ref <= 2.95))


# ---- 3  bits ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["narrow", "wide"])
def test_the_same_bits_alone_among_others_and_permuted(L, case):
    R, got = _call(L, case, 1, True, True)
    R2, got2 = _call(L, case, 1, True, True)
    for q in KEYS:
        assert np.array_equal(got[q], got2[q]), f"{q}: a repeated call gives the same bits"
    tau = _taus()
    for j in (0, 4, 8):                                                        # one time alone: the kernel <TT = 1>
        _, one = _call(L, case, 1, True, True, tau=tau[j:j + 1])
        for q in KEYS:
            assert np.array_equal(np.asarray(one[q])[:, 0], np.asarray(got[q])[:, j]), (q, j)
    _, two = _call(L, case, 1, True, True, tau=tau[[6, 2]])                    # two: <TT = 2>, out of order
    perm = np.array([3, 8, 0, 5, 1, 7, 2, 6, 4])
    _, pm = _call(L, case, 1, True, True, tau=tau[perm])
    for q in KEYS:
        assert np.array_equal(np.asarray(two[q])[:, 0], np.asarray(got[q])[:, 6]) and np.array_equal(np.asarray(two[q])[:, 1], np.asarray(got[q])[:, 2]), q
        assert np.array_equal(np.asarray(pm[q]), np.asarray(got[q])[:, perm]), f"{q}: a permuted list gives the same columns"
    # a signal alone (<4, 1>) and among five (<2, 4>, its block shared with others or not)
    _, five = _call(L, case, 5, True, True)
    for s in (0, 3, 4):
        _, one = _call(L, case, 1, True, True, signals=s)
        for q in KEYS:
            if q != "neff":
                assert np.array_equal(np.asarray(one[q]), np.asarray(five[q])[:, :, s]), (q, s)
    assert np.array_equal(five["neff"], got["neff"])


# ---- 4  the capability: a resolution that follows the frequency ----------------------------------------------------------------------------------
def test_a_change_of_frequency_is_located_at_both_frequencies(L):
    """A record that is cos 2 pi 1.25 t in its first half and cos 2 pi 2.5 t in its second, plus noise of sigma 1/4: 6000 samples over 375
    units, so that a cell of the highest frequency still has Neff > 9.  At every time the arg-max over f of wwz is the frequency that is
    present there -- with cells of the same 6.4 periods at either frequency: 10.3 units at 1.25, 5.2 at 2.5.  The grid has steps of 1/8,
    about the resolution of a cell whose sigma is one period at f = 1.25 (a finer grid puts the arg-max of a noisy peak on a neighbour;
    twelve seeds of this record were tried on the CPU with Foster's formulas, and all give these peaks).  This shows that ONE call
    resolves both; it does not show that no single window length of lombscargle_spectrogram could (that is not asked for)."""
    rng = np.random.default_rng(5)
    N = 6000
    t = np.sort(rng.integers(0, SPAN * 1024, N)) / 1024.0
    y = np.where(t < SPAN / 2, np.cos(2 * np.pi * 1.25 * t), np.cos(2 * np.pi * 2.5 * t)) + 0.25 * rng.standard_normal(N)
    f = np.arange(2, 25) / 8.0
    tau = SPAN * (np.arange(10) + 0.5) / 10
    R = L.wwz(y, t, f, tau=tau)
    assert R.wwz.shape == (len(f), 10) and not R.empty.any() and np.all(np.isfinite(R.wwz))
    peak = f[np.argmax(R.wwz, axis=0)]
    assert np.all(peak[:5] == 1.25) and np.all(peak[5:] == 2.5), peak
    assert np.all(R.neff > 9)


# ---- 5  a large offset ---------------------------------------------------------------------------------------------------------------------------
def test_a_large_offset_keeps_every_bound(L):
    """y + 10^6: the record's mean is removed before anything is summed, and the bounds -- which do not grow with the offset, but for c,
    which carries 16 u of it -- hold as in the centred case."""
    _check(L, "narrow", 3, True, True, offset=1e6)


# ---- 6  no NaN ---------------------------------------------------------------------------------------------------------------------------------
def test_a_noiseless_sinusoid_gives_no_nan(L):
    N, c, wmin, _ = CASES["narrow"]
    t, _, W = _record(N)
    f, tau = _freqs(), _taus()
    f = np.sort(np.append(f[f != 1.25], 1.25))[:NF]
    y = 3.0 + np.cos(2 * np.pi * 1.25 * t)
    R, (a, b, cc) = L.wwz(y, t, f, tau=tau, c=c, wmin=wmin, W=W, coef=True)
    for v in (R.power, R.amplitude, R.wwz, R.neff, a, b, cc):
        assert not np.any(np.isnan(v))
    k = int(np.flatnonzero(f == 1.25)[0])
    ak, rk = decay(c, 1.25), radius(1.25, c, wmin)
    checked = 0
    for j in range(NTAU):
        ref = wwz_cell_ref(y, t, W, 1.25, tau[j], ak, rk, center=True, removed=_record_mean(y[:, None], W))
        if ref is None or not _compared(ref):
            continue
        sl = slice(ref["start"], ref["start"] + ref["count"])
        bnd = float(_cell_bounds(ref, y[sl, None], t[sl])["power"][0])
        assert abs(R.power[k, j] - 1.0) <= bnd and (R.wwz[k, j] > 1e12 or np.isinf(R.wwz[k, j])), (j, R.power[k, j], bnd)
        checked += 1
    assert checked >= 5
    # a constant signal: power and wwz are 0 everywhere
    R = L.wwz(np.full(N, 7.0), t, f, tau=tau, c=c, wmin=wmin, W=W)
    assert np.all(R.power == 0.0) and np.all(R.wwz == 0.0) and not np.any(np.isnan(R.amplitude))


# ---- 7  errors ---------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_carry_the_librarys_message(L):
    import ctypes as C
    from lpvspectral_jl_amd import _lib
    t, y, W = _record(255)
    y = y[:, 0]
    f, tau = _freqs()[:5], _taus()[:3]

    def raises(message, **kw):
        args = dict(y=y, t=t, f=f, tau=tau, W=W)
        args.update(kw)
        with pytest.raises(ValueError) as e:
            L.wwz(args.pop("y"), args.pop("t"), args.pop("f"), **args)
        assert str(e.value) == _lib.last_error() and message in str(e.value), (message, str(e.value))

    def poke(a, i, v):
        a = np.array(a, dtype=np.float64)
        a[i] = v
        return a
    for bad in (np.nan, np.inf):
        raises("t, y or W holds a value that is not finite", t=poke(t, 100, bad))
        raises("t, y or W holds a value that is not finite", y=poke(y, 7, bad))
        raises("t, y or W holds a value that is not finite", W=poke(W, 254, bad))
        raises("a frequency is not finite", f=poke(f, 2, bad))
        raises("a time tau is not finite", tau=poke(tau, 1, bad))
    raises("frequency 0 is not positive", f=poke(f, 0, 0.0))
    raises("frequency 3 is not positive", f=poke(f, 3, -1.0))
    raises("a weight is negative", W=poke(W, 3, -0.5))
    raises("the decay c must be positive", c=0.0)
    raises("the decay c must be positive", c=-1.0)
    raises("t is not sorted", t=poke(t, 100, t[99] - 0.5))
    raises("need N > 0, Nf > 0, Ntau > 0", f=np.zeros(0))
    raises("need N > 0, Nf > 0, Ntau > 0", tau=np.zeros(0))
    # the radii are an argument of the entry point alone (the binding derives them from wmin)
    out = [np.zeros((1, 3, 5)) for _ in range(3)] + [np.zeros((3, 5))]
    ptr = lambda a: C.c_void_p(np.ascontiguousarray(a).ctypes.data)
    for bad in (np.nan, 0.0, -2.0):
        rad = poke(np.ones(5), 4, bad)
        rc = _lib.lib().lpvs_wwz_f64(ptr(y), 1, ptr(t), len(t), None, ptr(f), 5, ptr(tau), 3, C_FOSTER, ptr(rad), 1, 0, *[ptr(o) for o in out], None, None, None)
        assert rc == _lib.LPVS_EARGUMENT and _lib.last_error() == "wwz: radius 4 is not positive (or not a number)"
    with pytest.raises(ValueError):
        L.wwz(y, t, f, tau=tau, ntau=3)
    with pytest.raises(ValueError):
        L.wwz(y[:-1], t, f, tau=tau)


# ---- 8  the heat map, device inputs, defaults ------------------------------------------------------------------------------------------------------
def test_heatmap_device_inputs_and_defaults(L):
    import torch
    N = CASES["narrow"][0]
    t, y, W = _record(N)
    R = L.wwz(y[:, 0], t, _freqs(), tau=_taus()[1:8], W=W)
    tt, ff, z = L.heatmap(R)
    assert isinstance(R, L.Spectrogram) and np.array_equal(tt, _taus()[1:8]) and np.array_equal(ff, _freqs()[1:]) and z.shape == (NF - 1, 7)
    dev = lambda a: torch.as_tensor(a, device="cuda")
    Rd = L.wwz(dev(y[:, 0].copy()), dev(t), _freqs(), tau=_taus()[1:8], W=dev(W))
    for q in ("power", "wwz", "amplitude", "neff", "counts", "empty"):
        assert np.array_equal(getattr(Rd, q), getattr(R, q)), q
    R = L.wwz(y[:, 0], t, ntau=5)                                              # defaults: default_freqs(t) without its zero, 5 times over the record
    assert np.array_equal(R.time, np.linspace(t[0], t[-1], 5)) and np.array_equal(R.freq, L.default_freqs(t)[1:]) and R.wwz.shape == (len(R.freq), 5)
    assert np.array_equal(R.radius, L.wwz_radius(R.freq)) and np.all(np.isinf(L.wwz_radius(R.freq, wmin=0)))
    assert L.wwz(y[:, 0], t, _freqs()).time.shape == (64,)
