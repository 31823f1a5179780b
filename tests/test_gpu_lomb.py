"""lombscargle on the GPU against the long-double reference of tests/_lomb_ref.py (its own checks: tests/test_lomb_ref_host.py).

INPUTS.  t in multiples of 2^-10 over 40 units, f in multiples of 2^-6 (2^-8 for the grid from a = 37.25 D, 2^-34 for the grid with
residuals): every product f t is exact in double, so the reference's phases are beyond dispute.  Times are random, non-uniform and, at
N = 1000, not sorted.  Weights are drawn from [0.5, 2].
INEXACT PRODUCTS (the cases named "wide"; tests/_lomb_ref.py).  t over [0, 2^20] on multiples of 2^-10 or as full-mantissa doubles, f
full-mantissa doubles in (0, 3]: every product f t is inexact and reaches 3e6 turns, so the low word e = fma(f, t, -p) of
csrc/lomb_device.h: lomb_sincos carries up to 2e-10 turns -- 1e-9 rad, against bounds of 5e-13.  The reference forms the same exact turns.

BOUNDS (u = 2^-53).
  direct sums:     |sum - ref| <= (N + 16) u sum|terms| + 4 u per term of trigonometry -- the bound tests/test_gpu_gram_dense.py holds its
                   sums to.  For the double-angle rows the four ulps of cos and of sin pass through c^2 - s^2 and 2 s c:
                   |d(c^2 - s^2)|, |d(2 s c)| <= 2 (|c| + |s|) 4 u <= 2 sqrt(2) 4 u per term.
                   Inexact products: 6 u in place of the 4 u.  r = (p - rint(p)) + e now rounds once, |r| <= 1/2, so the phase moves by
                   at most 2 pi 2^-55 <= 1.6 u on top of the sincospi.
  transform sums:  |sum - ref| <= 1e-12 sum|terms| -- what tests/test_gpu_nufft.py holds the same spreading to -- plus, for the grid with
                   frequency residuals, the dropped second-order term (residual phase)^2 / 2 sum|weights|; the double-angle family
                   applies the residuals twice over, so its phase is twice as large.
  centred data:    the device reports the weighted means it removed (held to (N + 16) u sum w|y|, a sum like the others), and the
                   reference centres with THOSE, so that both sides sum the same centred signal and no allowance for the mean is needed.
  power, a, b, c:  the sums' bounds passed through the epilogue to first order (1 % is added for the higher orders), every quotient
                   by the REFERENCE's D, plus the epilogue's own roundings (16 u of the magnitudes that are added).  No constant is
                   fitted to what the device gives.  The inputs are such that the reference's D >= 0.01 at every frequency it does not
                   call degenerate, and <= 2^-45 where it does (asserted)."""
import functools
import os

import numpy as np
import pytest

from _lomb_ref import LD, block_residual_phase, late_times, lomb_ref, wide_freqs, wide_grid

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _record(N, ns, seed=0, rec=None):
    """rec = "lattice" / "full": times over [0, 2^20] on multiples of 2^-10 / as full-mantissa doubles (tests/_lomb_ref.py)."""
    rng = np.random.default_rng(1000 * N + 10 * ns + seed)
    if rec:
        t = late_times(rng, N, rec == "lattice")
    else:
        t = rng.integers(0, 40 * 1024, N) / 1024.0
    if N != 1000 and not rec:
        t = np.sort(t)
    y = np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(ns)[None, :]) * (1.0 + np.arange(ns))[None, :] + 0.5 * rng.standard_normal((N, ns)) + 0.75
    W = rng.uniform(0.5, 2.0, N)
    for a in (t, y, W):
        a.setflags(write=False)
    return t, y, W


@functools.lru_cache(maxsize=None)
def _irregular(Nf):
    rng = np.random.default_rng(Nf)
    f = np.sort(rng.choice(np.arange(1, 193), Nf, replace=False)) / 64.0      # distinct multiples of 2^-6 in (0, 3]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _grid(kind, Nf=200):
    D = 1.0 / 64.0
    if kind == "zero":
        f = D * np.arange(Nf)
    elif kind == "step":
        f = D * np.arange(1, Nf + 1)
    elif kind == "offset":
        f = 37.25 * D + D * np.arange(Nf)
    else:                                                                      # "residual": interior frequencies moved by -1, 0, 1 times 2^-34
        j = np.random.default_rng(7).integers(-1, 2, Nf).astype(np.float64)
        j[0] = j[-1] = 0.0
        f = D * np.arange(1, Nf + 1) + j * 2.0 ** -34
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _wide(kind, Nf=200):
    """Full-mantissa frequencies in (0, 3] (tests/_lomb_ref.py): "wide-irregular", and the progressions "wide-zero" (from 0) and
    "wide-offset" (from a = 37.25 D) of a step that is no binary fraction."""
    f = wide_freqs(np.random.default_rng(50 + Nf), Nf) if kind == "wide-irregular" else wide_grid(0.0 if kind == "wide-zero" else 37.25, Nf)
    f.setflags(write=False)
    return f


def _freqs(fkey):
    if fkey[0].startswith("wide"):
        return _wide(*fkey)
    return _irregular(fkey[1]) if fkey[0] == "irregular" else _grid(fkey[0])


@functools.lru_cache(maxsize=None)
def _ref(N, ns, fkey, fit_mean=True, center=True, normalization="standard", removed=None, rec=None):
    """removed: the means the device removed, as a tuple (the cache's key: the device gives the same bits every time)."""
    t, y, W = _record(N, ns, rec=rec)
    f = _freqs(fkey)
    return lomb_ref(y, t, f, W=W, fit_mean=fit_mean, center_data=center, normalization=normalization, removed=None if removed is None else np.array(removed))


# ---- bounds --------------------------------------------------------------------------------------------------------------------------------
def _sum_bounds(r, t, y, W, transform, eps_phase=0.0, trig=4):
    """Bounds of every raw sum, same keys and shapes as the reference's (r: centred with the device's means).  trig: the ulps of
    trigonometry per term of the direct sums, 4 where every product f t is exact and 6 where it is not (the module's docstring)."""
    N = len(t)
    w = (W / W.sum()).astype(LD)
    yc = y.astype(LD) - r["removed"][None, :]
    sw, swy, swyy = LD(1), (w[:, None] * np.abs(yc)).sum(axis=0), (w[:, None] * yc * yc).sum(axis=0)
    b = {}
    if transform:
        for k, ph in (("C", eps_phase), ("S", eps_phase), ("C2", 2 * eps_phase), ("S2", 2 * eps_phase)):
            b[k] = 1e-12 * r["abs_" + k] + 0.5 * ph ** 2 * sw
        for k in ("YC", "YS"):
            b[k] = 1e-12 * r["abs_" + k] + 0.5 * eps_phase ** 2 * swy[:, None]
    else:
        for k in ("C", "S"):
            b[k] = (N + 16) * U * r["abs_" + k] + trig * U * sw
        for k in ("C2", "S2"):
            b[k] = (N + 16) * U * r["abs_" + k] + 2 * np.sqrt(2.0) * trig * U * sw
        for k in ("YC", "YS"):
            b[k] = (N + 16) * U * r["abs_" + k] + trig * U * swy[:, None]
    b["Y"] = (N + 16) * U * swy
    b["YY"] = (N + 16) * U * swyy
    b["mean"] = (N + 16) * U * r["abs_mean"]
    b["removed"] = 0 * swy                                                    # the reference removed the device's own means
    return b


def _epilogue_bounds(r, b, fit_mean, psd, N):
    """First-order bounds of power, a, b, c (Nf, ns) from the sums' bounds b, by the reference's D."""
    with np.errstate(all="ignore"):                                           # (degenerate frequencies divide by D = 0; they are not compared)
        return _epilogue_bounds_(r, b, fit_mean, psd, N)


def _epilogue_bounds_(r, b, fit_mean, psd, N):
    C, S = np.abs(r["C"])[:, None], np.abs(r["S"])[:, None]
    dC, dS, dC2, dS2 = b["C"][:, None], b["S"][:, None], b["C2"][:, None], b["S2"][:, None]
    Y, dY, dYY = np.abs(r["Y"])[None, :], b["Y"][None, :], b["YY"][None, :]
    YC, YS = r["YCf"], r["YSf"]                                               # after the floating-mean terms
    CC, SS, CS, D = r["CC"][:, None], r["SS"][:, None], r["CS"][:, None], r["D"][:, None]
    dYC, dYS = b["YC"].T, b["YS"].T
    dCC, dSS, dCS = dC2 / 2, dC2 / 2, dS2 / 2
    if fit_mean:
        dCC, dSS, dCS = dCC + 2 * C * dC, dSS + 2 * S * dS, dCS + C * dS + S * dC
        dYC, dYS, dYY = dYC + Y * dC + C * dY, dYS + Y * dS + S * dY, dYY + 2 * Y * dY
    # the epilogue's own roundings: 16 u of the magnitudes that are added
    mD = np.abs(CC * SS) + CS * CS + (C * C + S * S if fit_mean else 0)
    dD = np.abs(SS) * dCC + np.abs(CC) * dSS + 2 * np.abs(CS) * dCS + 16 * U * mD
    pa, pb = SS * YC - CS * YS, CC * YS - CS * YC                             # a D, b D
    mNum = np.abs(SS) * YC * YC + np.abs(CC) * YS * YS + 2 * np.abs(CS * YC * YS)
    dNum = YC * YC * dSS + YS * YS * dCC + 2 * np.abs(YC * YS) * dCS + 2 * np.abs(pa) * dYC + 2 * np.abs(pb) * dYS + 16 * U * mNum
    a, bb, p = np.abs(r["a"]), np.abs(r["b"]), np.abs(r["p"])
    dp = (dNum + p * dD) / D
    da = (np.abs(YC) * dSS + np.abs(SS) * dYC + np.abs(YS) * dCS + np.abs(CS) * dYS + 16 * U * (np.abs(SS * YC) + np.abs(CS * YS)) + a * dD) / D
    db = (np.abs(YS) * dCC + np.abs(CC) * dYS + np.abs(YC) * dCS + np.abs(CS) * dYC + 16 * U * (np.abs(CC * YS) + np.abs(CS * YC)) + bb * dD) / D
    dc = b["removed"][None, :] + 0 * a
    if fit_mean:
        dc = dc + dY + a * dC + C * da + bb * dS + S * db + 16 * U * (np.abs(r["removed"])[None, :] + Y + a * C + bb * S)
    if psd:
        dpow = dp * N / 2
    else:
        YYf = r["YYf"][None, :]
        dpow = dp / YYf + p * dYY / (YYf * YYf) + 4 * U * p / YYf
    return {k: 1.01 * v for k, v in (("power", dpow), ("a", da), ("b", db), ("c", dc))}


def _ratio(err, bound):
    return float(np.max(err / np.where(bound > 0, bound, LD(1)), initial=0.0))


def _check(L, N, ns, fkey, path, fit_mean=True, center=True, normalization="standard", eps_phase=0.0, rec=None):
    t, y, W = _record(N, ns, rec=rec)
    f = _freqs(fkey)
    P, (a, b, c), sums = L.lombscargle(y if ns > 1 else y[:, 0], t, f, W=W, fit_mean=fit_mean, center_data=center, normalization=normalization, path=path,
                                       coef=True, return_sums=True)
    tm = L.lombscargle_last_timing()
    r = _ref(N, ns, fkey, fit_mean, center, normalization, tuple(sums["mean"]) if center else None, rec)
    deg = r["degenerate"]
    assert np.all((r["D"][~deg] >= 0.01)) and np.all(r["D"][deg] <= 2.0 ** -45), "the inputs are to stay clear of the degenerate threshold"
    assert tm["path"] == path and tm["degenerate"] == int(deg.sum())
    bs = _sum_bounds(r, t, y, W, path == "nufft", eps_phase, 6 if rec else 4)
    for k in ("mean", "C", "S", "C2", "S2", "YC", "YS", "Y", "YY"):
        err = np.abs(sums[k].astype(LD) - r[k])
        print(k, "worst error / bound:", _ratio(err, bs[k]))
        assert np.all(err <= bs[k]), (k, _ratio(err, bs[k]))
    got = {"power": P.power, "a": a, "b": b, "c": c}
    be = _epilogue_bounds(r, bs, fit_mean, normalization == "psd", N)
    for k, g in got.items():
        g = np.asarray(g).reshape(len(f), ns)
        assert np.all(g[deg] == 0.0), f"{k}: degenerate frequencies give exact zeros"
        err = np.abs(g.astype(LD) - r[k])[~deg]
        print(k, "worst error / bound:", _ratio(err, be[k][~deg]))
        assert np.all(err <= be[k][~deg]), (k, _ratio(err, be[k][~deg]))
    if normalization == "standard" and fit_mean:
        assert np.all(P.power >= 0.0) and np.all(P.power <= 1.0 + 1e-12)
    return tm


# ---- direct path -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 3])
@pytest.mark.parametrize("Nf", [1, 7, 65])
@pytest.mark.parametrize("N", [1, 255, 1000, 4097])
def test_direct_sums_power_and_coefficients(L, N, Nf, ns):
    """N = 1: every frequency is degenerate; 4097 samples are five slabs, 65 frequencies two tiles, three signals one block of four.
    Centring and the floating mean alternate over the cases so that every combination meets every shape class."""
    case = (N + Nf + ns) % 4
    tm = _check(L, N, ns, ("irregular", Nf), "direct", fit_mean=case < 2, center=case % 2 == 0, normalization="psd" if (N + Nf) % 3 == 0 else "standard")
    assert tm["blocks"] == (0, 0) and tm["nf"] == 0 and tm["slabs"] == {1: 1, 255: 1, 1000: 1, 4097: 5}[N]


def test_direct_takes_the_zero_frequency_of_a_progression_as_degenerate(L):
    tm = _check(L, 1000, 1, ("zero",), "direct")
    assert tm["degenerate"] == 1


# ---- transform path ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [None, 64])
@pytest.mark.parametrize("kind", ["zero", "step", "offset"])
def test_transform_sums_power_and_coefficients(L, monkeypatch, kind, block):
    """200 frequencies in one block, and with LPVS_LOMB_BLOCK=64 in four per family: pre-phase on all but the first (on all four when
    the grid does not start at 0), a ragged last block of 8."""
    if block is None:
        monkeypatch.delenv("LPVS_LOMB_BLOCK", raising=False)
    else:
        monkeypatch.setenv("LPVS_LOMB_BLOCK", str(block))
    tm = _check(L, 4097, 3, (kind,), "nufft", normalization="psd" if kind == "step" else "standard")
    assert tm["blocks"] == ((1, 1) if block is None else (4, 4)) and tm["nf"] == (1024 if block is None else 256)
    assert tm["degenerate"] == (1 if kind == "zero" else 0) and tm["slabs"] == 0 and not tm["twin"]


@pytest.mark.parametrize("block", [None, 64])
def test_transform_takes_frequency_residuals_to_first_order(L, monkeypatch, block):
    """Residuals of 2^-34: a phase of 2 pi 2^-34 40 = 1.5e-8, 10^4 times the bound if the first-order term were missing or had the wrong
    sign; the dropped second-order term is 1.1e-16."""
    if block is None:
        monkeypatch.delenv("LPVS_LOMB_BLOCK", raising=False)
    else:
        monkeypatch.setenv("LPVS_LOMB_BLOCK", str(block))
    tm = _check(L, 4097, 1, ("residual",), "nufft", fit_mean=False, center=False, eps_phase=2 * np.pi * 2.0 ** -33 * 40.0)
    assert tm["twin"] and tm["blocks"] == ((1, 1) if block is None else (4, 4))


# ---- inexact products ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", ["lattice", "full"])
def test_direct_sums_of_inexact_products(L, rec):
    """N = 4097 (five slabs), 65 frequencies (two tiles), three signals; every f t inexact, up to 3e6 turns."""
    tm = _check(L, 4097, 3, ("wide-irregular", 65), "direct", rec=rec)
    assert tm["blocks"] == (0, 0) and tm["nf"] == 0 and tm["slabs"] == 5 and tm["degenerate"] == 0


@pytest.mark.parametrize("block", [None, 64])
@pytest.mark.parametrize("kind", ["wide-zero", "wide-offset"])
def test_transform_sums_of_inexact_products(L, monkeypatch, kind, block):
    """200 frequencies a + k D of a step that is no binary fraction, from a = 0 and from a = 37.25 D, t to 2^20: the pre-phase of the
    blocks' bases (lomb_prephase_kernel: lomb_sincos on inexact products), the coordinates (nu_phase_turns of 2 pi D t = 8e4 rad) and the
    natural rounding residuals of the grid, taken to first order (twin)."""
    if block is None:
        monkeypatch.delenv("LPVS_LOMB_BLOCK", raising=False)
    else:
        monkeypatch.setenv("LPVS_LOMB_BLOCK", str(block))
    t = _record(4097, 3, rec="lattice")[0]
    eps_phase = block_residual_phase(_wide(kind), t, block)
    assert 0.0 < eps_phase <= 2e-7                                           # (csrc/lomb_plan.h: twice the admitted 1e-7 at the most)
    tm = _check(L, 4097, 3, (kind,), "nufft", eps_phase=eps_phase, rec="lattice")
    assert tm["blocks"] == ((1, 1) if block is None else (4, 4)) and tm["nf"] == (1024 if block is None else 256)
    assert tm["degenerate"] == (1 if kind == "wide-zero" else 0) and tm["slabs"] == 0 and tm["twin"]


def test_a_constant_signal_has_standard_power_zero(L):
    """Unequal weights: the weighted mean is not the constant to the last bit, and without centring YY - Y^2 is a rounding residue.  Both
    count as YY = 0 (csrc/lomb_plan.h: lomb_yy_noise: (1016 u)^2 R = 9e-26 centred, 3 1016 u YY = 2.5e-12 not centred).  A sinusoid of
    amplitude 1e-6 on the constant (variance 5e-13) is a signal for the centred fit; without centring YY - Y^2 cannot resolve it, and one of
    amplitude 1e-3 is."""
    t, y, W = _record(1000, 1)
    f = _irregular(65)
    const = np.full(1000, 2.7)
    for center, amplitude in ((True, 1e-6), (False, 1e-3)):
        assert np.all(L.lombscargle(const, t, f, W=W, center_data=center).power == 0.0), center
        Pw = L.lombscargle(const + amplitude * np.cos(2 * np.pi * f[30] * t), t, f, W=W, center_data=center)
        assert int(np.argmax(Pw.power)) == 30 and Pw.power[30] > 0.999, center
    assert np.all(L.lombscargle(const, t, f, W=W, center_data=False, fit_mean=False, normalization="psd").power > 0)   # psd: no quotient by YY
    assert np.all(lomb_ref(const, t, f, W=W, center_data=False)["power"] == 0) and np.all(lomb_ref(const, t, f, W=W)["power"] == 0)


# ---- further cases -----------------------------------------------------------------------------------------------------------------------
def _bits(L, y, t, f, W, path, **kw):
    P, (a, b, c) = L.lombscargle(y, t, f, W=W, path=path, coef=True, **kw)
    return [np.asarray(x).tobytes() for x in (P.power, a, b, c)]


@pytest.mark.parametrize("path,block", [("direct", None), ("nufft", None), ("nufft", 64)])
def test_same_bits_twice_per_column_and_from_device_tensors(L, monkeypatch, path, block):
    import torch
    if block is None:
        monkeypatch.delenv("LPVS_LOMB_BLOCK", raising=False)
    else:
        monkeypatch.setenv("LPVS_LOMB_BLOCK", str(block))
    t, y, W = _record(4097, 3)
    f = _grid("offset")
    P, (a, b, c) = L.lombscargle(y, t, f, W=W, path=path, coef=True)
    first = [P.power, a, b, c]
    again = L.lombscargle(y, t, f, W=W, path=path, coef=True)
    for x, z in zip(first, [again[0].power, *again[1]]):
        assert x.shape == (200, 3) and np.array_equal(x, z)
    for q in range(3):                                                        # a column of the call = the call of that signal alone
        Pq, cq = L.lombscargle(y[:, q], t, f, W=W, path=path, coef=True)
        for x, z in zip(first, [Pq.power, *cq]):
            assert z.shape == (200,) and np.array_equal(x[:, q], z), q
    dev = L.lombscargle(torch.tensor(y, device="cuda"), torch.tensor(t, device="cuda"), f, W=torch.tensor(W, device="cuda"), path=path, coef=True)
    for x, z in zip(first, [dev[0].power, *dev[1]]):
        assert np.array_equal(x, z)


def test_auto_reports_the_path_of_the_plan(L, monkeypatch):
    """csrc/lomb_plan.h: the transforms from 2^18 samples, 512 frequencies and N Nf = 2^29 on, for admitted grids."""
    monkeypatch.delenv("LPVS_LOMB_BLOCK", raising=False)
    for N, f, want in ((4097, _grid("step"), "direct"), (4097, _irregular(65), "direct")):
        t, y, W = _record(N, 1)
        P = L.lombscargle(y[:, 0], t, f, W=W)
        assert L.lombscargle_last_timing()["path"] == want and P.power.shape == (len(f),) and np.array_equal(P.freq, f)
    rng = np.random.default_rng(5)
    t = np.sort(rng.integers(0, 1 << 30, 1 << 18)) / 1024.0                  # 2^18 samples over 2^20 units
    y = np.cos(2 * np.pi * 0.25 * t) + rng.standard_normal(1 << 18)
    for Nf, want in ((2048, "nufft"), (2047, "direct")):
        f = np.arange(1, Nf + 1) / 4096.0
        P = L.lombscargle(y, t, f)
        tm = L.lombscargle_last_timing()
        assert tm["path"] == want and tm["degenerate"] == 0
        assert np.array_equal(P.power, L.lombscargle(y, t, f, path=want).power)   # auto is that path, to the bit
        assert int(np.argmax(P.power)) == 1023                               # f = 1/4
    t, y, W = _record(255, 1)
    P = L.lombscargle(y[:, 0], t)                                             # f = default_freqs(t)
    assert np.array_equal(P.freq, L.default_freqs(t)) and P.power[0] == 0.0
    assert np.array_equal(L.lombscargle(y[:, 0].astype(np.float32), t, P.freq).power, L.lombscargle(y[:, 0].astype(np.float32).astype(np.float64), t, P.freq).power)


def test_bad_inputs_raise_value_errors(L):
    t, y, W = _record(255, 1)
    f = _irregular(7)
    tn = t.copy(); tn[17] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        L.lombscargle(y[:, 0], tn, f)
    yi = y[:, 0].copy(); yi[3] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        L.lombscargle(yi, t, f)
    Wn = W.copy(); Wn[5] = -0.25
    with pytest.raises(ValueError, match="negative"):
        L.lombscargle(y[:, 0], t, f, W=Wn)
    with pytest.raises(ValueError, match="sum to"):
        L.lombscargle(y[:, 0], t, f, W=np.zeros(255))
    with pytest.raises(ValueError, match="not finite"):
        L.lombscargle(y[:, 0], t, np.array([0.5, np.nan]))
    with pytest.raises(ValueError, match="progression"):
        L.lombscargle(y[:, 0], t, f, path="nufft")
    with pytest.raises(ValueError):
        L.lombscargle(y[:, 0], t, f, path="fft")
    with pytest.raises(ValueError):
        L.lombscargle(y[:, 0], t, f, normalization="density")
    assert os.environ.get("LPVS_EXPERIMENTS") == "1"                          # (the block knob of the cases above is read only with it)
