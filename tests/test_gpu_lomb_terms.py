"""lombscargle(..., nterms=K) on the GPU against the long-double reference of tests/_lomb_terms_ref.py (its own checks:
tests/test_lomb_terms_ref_host.py).

INPUTS.  Those of tests/test_gpu_lomb.py: t in multiples of 2^-10 over 40 units (N = 1000: not sorted, four stages of 256 with the last
partial; N = 2501: three slabs, the last partial), weights in [0.5, 2], 70 distinct frequencies in multiples of 2^-6 in [4/64, 3] (two
tiles, the second partial), ns in {1, 3, 5}.  Every product f t is exact in double.  The grid starts at 4/64 because at f = 1/64 the six-term
design is nearly singular over 40 units (smallest pivot 0.008); on these inputs the reference's smallest pivot is >= 0.3 for every K <= 6.
Asserted: pivots >= 0.01 at every frequency the reference does not call degenerate, <= 2^-45 where it does.
One case more has INEXACT products (tests/_lomb_ref.py): t over [0, 2^20], on the 2^-10 lattice and as full-mantissa doubles, f
full-mantissa doubles in (0, 3]; f t reaches 3e6 turns and the low word of lomb_sincos decides.

BOUNDS (u = 2^-53); nothing is fitted to what the device returns, every term comes from the reference.
  sums:   |sum - ref| <= (N + 16) u sum|terms| + e_m sum|weights| for a row of harmonic m, e_m = m 4 sqrt(2) u + 3 (m - 1) u: z_1 carries
          the four ulps of cos and of sin (modulus 4 sqrt(2) u), and every rotation z_m = z_{m-1} z_1 adds the moduli of the errors of
          its factors and its own roundings (3 u).  Y, YY and the means: (N + 16) u sum|terms|.  The reference is centred with the
          means the device reports, so both sides sum the same centred signal.
  A, b:   the sums' bounds through A = (C_|h-j| +- C_{h+j}) / 2, (S_{h+j} +- S_|h-j|) / 2, A -= g g^T, b -= Y g, plus 4 u (|A_pre| + |g||g|^T)
          and 4 u (|b_pre| + |Y||g|) for forming them.
  theta:  |d theta| <= 1.01 |A^-1| (|dA||theta| + |db| + gamma (|L| D |L|^T) |theta|), gamma = (3n + 1) u / (1 - (3n + 1) u): the backward
          error of an L D L^T solve (Higham, Accuracy and Stability, Th. 10.4 with 10.3's constant); 1 % for the higher orders.
  p:      |dp| <= |db|^T |theta| + |b|^T |d theta| + (n + 2) u |b|^T |theta|.
  power, c: from dp, dYY, dY, dg, d theta as _epilogue_bounds of tests/test_gpu_lomb.py does for one term (its 4 u and 16 u for the
          epilogue's own roundings, its 1 %)."""
import functools

import numpy as np
import pytest

from _lomb_ref import LD, late_times, lomb_ref, wide_freqs
from _lomb_terms_ref import ldl_solve, lomb_terms_ref
from test_lomb_terms_ref_host import planted

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
WORST = {}                                                                    # quantity -> worst error / bound seen in this session (printed)


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _record(N, ns, seed=0):
    rng = np.random.default_rng(1000 * N + 10 * ns + seed)
    t = rng.integers(0, 40 * 1024, N) / 1024.0
    if N != 1000:
        t = np.sort(t)
    y = np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(ns)[None, :]) * (1.0 + np.arange(ns))[None, :] + 0.5 * rng.standard_normal((N, ns)) + 0.75
    W = rng.uniform(0.5, 2.0, N)
    for a in (t, y, W):
        a.setflags(write=False)
    return t, y, W


@functools.lru_cache(maxsize=None)
def _freqs(Nf=70):
    rng = np.random.default_rng(Nf)
    f = np.sort(rng.choice(np.arange(4, 193), Nf, replace=False)) / 64.0      # distinct multiples of 2^-6 in [4/64, 3]
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _uniform():
    rng = np.random.default_rng(512)
    t = np.arange(512) / 16.0
    y = np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(2)[None, :]) + 0.3 * np.cos(2 * np.pi * 2.5 * t[:, None]) + 0.5 * rng.standard_normal((512, 2)) + 0.75
    W = rng.uniform(0.5, 2.0, 512)
    for a in (t, y, W):
        a.setflags(write=False)
    return t, y, W


def _call(L, y, t, f, K, W, fit_mean=True, center=True, normalization="standard"):
    """(P, (a, b, c), sums, timing); one term goes through the new entry too (the public function keeps g4's entry for it)."""
    if K == 1:
        out = L.api._lombscargle_terms(y, t, f, W, fit_mean, center, normalization, 0, True, True, 1)
    else:
        out = L.lombscargle(y, t, f, W=W, fit_mean=fit_mean, center_data=center, normalization=normalization, coef=True, return_sums=True, nterms=K)
    return (*out, L.lombscargle_terms_last_timing())


# ---- bounds --------------------------------------------------------------------------------------------------------------------------------
def _sum_bounds(r, t, y, W, trig=4):
    """trig: the ulps of cos and of sin of the first harmonic, 4 where every product f t is exact, 6 where it is not."""
    N, K = len(t), r["K"]
    w = (W / W.sum()).astype(LD)
    yc = y.reshape(N, -1).astype(LD) - r["removed"][None, :]
    swy, swyy = (w[:, None] * np.abs(yc)).sum(axis=0), (w[:, None] * yc * yc).sum(axis=0)
    e = np.array([m * trig * np.sqrt(2.0) * U + 3 * (m - 1) * U for m in range(1, 2 * K + 1)])
    b = {"C": (N + 16) * U * r["abs_C"] + e[:, None], "S": (N + 16) * U * r["abs_S"] + e[:, None]}            # sum|weights| = 1
    for k in ("YC", "YS"):
        b[k] = (N + 16) * U * r["abs_" + k] + e[None, :K, None] * swy[:, None, None]
    b["Y"], b["YY"], b["mean"] = (N + 16) * U * swy, (N + 16) * U * swyy, (N + 16) * U * r["abs_mean"]
    return b


def _fit_bounds(r, bs, fit_mean, psd, N):
    with np.errstate(all="ignore"):                                           # (degenerate frequencies are not compared)
        return _fit_bounds_(r, bs, fit_mean, psd, N)


def _fit_bounds_(r, bs, fit_mean, psd, N):
    K = r["K"]
    n, Nf = 2 * K, r["g"].shape[0]
    zero = np.zeros((1, Nf), dtype=LD)
    dC, dS = np.concatenate([zero, bs["C"]]), np.concatenate([zero, bs["S"]])  # harmonics 0 .. 2K
    dA = np.zeros((Nf, n, n), dtype=LD)
    for h in range(1, K + 1):
        for j in range(1, K + 1):
            dA[:, 2 * h - 2, 2 * j - 2] = dA[:, 2 * h - 1, 2 * j - 1] = (dC[abs(h - j)] + dC[h + j]) / 2
            dA[:, 2 * h - 2, 2 * j - 1] = dA[:, 2 * j - 1, 2 * h - 2] = (dS[h + j] + dS[abs(h - j)]) / 2
    dg = np.stack([bs["C"][:K], bs["S"][:K]], axis=1).reshape(n, Nf).T         # (Nf, n)
    db = np.stack([bs["YC"], bs["YS"]], axis=2).reshape(-1, n, Nf).transpose(2, 0, 1)   # (Nf, ns, n)
    g, Y, dY = np.abs(r["g"]), np.abs(r["Y"]), bs["Y"]
    dA = dA + 4 * U * np.abs(r["A_pre"])
    db = db + 4 * U * np.abs(r["b_pre"])
    dYY = bs["YY"]
    if fit_mean:
        gg = g[:, :, None] * g[:, None, :]
        dA = dA + g[:, :, None] * dg[:, None, :] + dg[:, :, None] * g[:, None, :] + 4 * U * gg
        db = db + Y[None, :, None] * dg[:, None, :] + dY[None, :, None] * g[:, None, :] + 4 * U * Y[None, :, None] * g[:, None, :]
        dYY = dYY + 2 * Y * dY
    th, b = np.abs(r["theta"]), np.abs(r["b"])
    Lm, d = np.abs(r["L"]), r["pivots_used"]
    Ainv = np.abs(ldl_solve(r["L"], d, np.broadcast_to(np.eye(n, dtype=LD), (Nf, n, n))))
    LDL = np.einsum("kiq,kq,kjq->kij", Lm, d, Lm)
    gamma = (3 * n + 1) * U / (1 - (3 * n + 1) * U)
    rhs = np.einsum("kij,kcj->kci", dA, th) + db + gamma * np.einsum("kij,kcj->kci", LDL, th)
    dth = 1.01 * np.einsum("kij,kcj->kci", Ainv, rhs)
    dp = (db * th).sum(axis=2) + (b * dth).sum(axis=2) + (n + 2) * U * (b * th).sum(axis=2)
    p = np.abs(r["p"])
    if psd:
        dpow = dp * N / 2
    else:
        YYf = r["YYf"][None, :]
        dpow = dp / YYf + p * dYY[None, :] / (YYf * YYf) + 4 * U * p / YYf
    dc = np.zeros_like(p)
    if fit_mean:
        dc = dY[None, :] + (th * dg[:, None, :]).sum(axis=2) + (g[:, None, :] * dth).sum(axis=2) + \
            16 * U * (np.abs(r["removed"])[None, :] + Y[None, :] + (g[:, None, :] * th).sum(axis=2))
    return {"power": 1.01 * dpow, "a": dth[:, :, 0::2].transpose(2, 0, 1), "b": dth[:, :, 1::2].transpose(2, 0, 1), "c": 1.01 * dc}


def _ratio(name, err, bound):
    v = float(np.max(err / np.where(bound > 0, bound, LD(1)), initial=0.0))
    WORST[name] = max(WORST.get(name, 0.0), v)
    return v


def _check(L, y, t, W, f, K, fit_mean=True, center=True, normalization="standard", trig=4):
    N = len(t)
    ns = 1 if y.ndim == 1 else y.shape[1]
    P, (a, b, c), sums, tm = _call(L, y, t, f, K, W, fit_mean, center, normalization)
    r = lomb_terms_ref(y, t, f, K, W=W, fit_mean=fit_mean, center_data=center, normalization=normalization, removed=sums["mean"] if center else None)
    deg = r["degenerate"]
    assert np.all(r["worst_pivot"][~deg] >= 0.01) and np.all(r["worst_pivot"][deg] <= 2.0 ** -45), "the inputs are to stay clear of the degenerate threshold"
    assert tm["nterms"] == K and tm["degenerate"] == int(deg.sum())
    assert sums["C"].shape == sums["S"].shape == (2 * K, len(f)) and sums["YC"].shape == sums["YS"].shape == (ns, K, len(f))
    bs = _sum_bounds(r, t, y, W, trig)
    for k in ("mean", "C", "S", "YC", "YS", "Y", "YY"):
        err = np.abs(sums[k].astype(LD) - r[k])
        print(f"K = {K} {k}: worst error / bound {_ratio(k, err, bs[k]):.3f}")
        assert np.all(err <= bs[k]), (k, _ratio(k, err, bs[k]))
    be = _fit_bounds(r, bs, fit_mean, normalization == "psd", N)
    shape = (len(f),) if y.ndim == 1 else (len(f), ns)
    assert P.power.shape == c.shape == shape and a.shape == b.shape == (K, *shape)
    got = {"power": np.asarray(P.power).reshape(len(f), ns), "a": np.asarray(a).reshape(K, len(f), ns), "b": np.asarray(b).reshape(K, len(f), ns),
           "c": np.asarray(c).reshape(len(f), ns)}
    want = {"power": r["power"], "a": r["a"], "b": r["b_h"], "c": r["c"]}
    for k, gv in got.items():
        assert np.all(gv[..., deg, :] == 0.0), f"{k}: degenerate frequencies give exact zeros"
        err = np.abs(gv.astype(LD) - want[k])[..., ~deg, :]
        bound = be[k][..., ~deg, :]
        print(f"K = {K} {k}: worst error / bound {_ratio(k, err, bound):.3f}")
        assert np.all(err <= bound), (k, _ratio(k, err, bound))
    if normalization == "standard" and fit_mean:
        assert np.all(P.power >= 0.0) and np.all(P.power <= 1.0 + 1e-12)
    return tm, r, got, be


# ---- 1. every instantiation -----------------------------------------------------------------------------------------------------------------
TS = {2: 4, 3: 4, 4: 4, 5: 2, 6: 2}                                           # signals per thread of a multi-signal call


@pytest.mark.parametrize("ns", [1, 3, 5])
@pytest.mark.parametrize("K", [2, 3, 4, 5, 6])
def test_sums_power_and_coefficients_of_every_instantiation(L, K, ns):
    t, y, W = _record(1000, ns)
    tm, _, _, _ = _check(L, y if ns > 1 else y[:, 0], t, W, _freqs(), K)
    ts = 1 if ns == 1 else TS[K]
    assert (tm["ts"], tm["accumulators"], tm["slabs"]) == (ts, 4 * K + 2 * K * ts, 1)


@pytest.mark.parametrize("K", [2, 6])
def test_three_slabs_the_last_partial(L, K):
    t, y, W = _record(2501, 3)
    tm, _, _, _ = _check(L, y, t, W, _freqs(), K)
    assert (tm["ts"], tm["accumulators"], tm["slabs"]) == (TS[K], 4 * K + 2 * K * TS[K], 3)


@functools.lru_cache(maxsize=None)
def _late(rec, N=2501, ns=3, Nf=70):
    """tests/_lomb_ref.py: times over [0, 2^20] (rec = "lattice": multiples of 2^-10; "full": full-mantissa doubles) and full-mantissa
    frequencies in (0, 3]: every product f t is inexact, up to 3e6 turns."""
    rng = np.random.default_rng(7000 + N + ns + (rec == "full"))
    t = late_times(rng, N, rec == "lattice")
    f = wide_freqs(rng, Nf)
    y = np.cos(2 * np.pi * f[40] * t[:, None] + np.arange(ns)[None, :]) * (1.0 + np.arange(ns))[None, :] + 0.5 * rng.standard_normal((N, ns)) + 0.75
    W = rng.uniform(0.5, 2.0, N)
    for a in (t, y, W, f):
        a.setflags(write=False)
    return t, y, W, f


@pytest.mark.parametrize("rec", ["lattice", "full"])
def test_three_harmonics_of_inexact_products(L, rec):
    """The low word e of lomb_sincos in lomb_terms_kernel: 2e-10 turns at f t = 3e6, times m in the m-th harmonic.  6 u of trigonometry in
    place of 4 u: r = (p - rint(p)) + e rounds once, |r| <= 1/2, a phase of at most 2 pi 2^-55 <= 1.6 u."""
    t, y, W, f = _late(rec)
    tm, _, _, _ = _check(L, y, t, W, f, 3, trig=6)
    assert (tm["ts"], tm["accumulators"], tm["slabs"], tm["degenerate"]) == (TS[3], 4 * 3 + 2 * 3 * TS[3], 3, 0)


@pytest.mark.parametrize("normalization", ["standard", "psd"])
@pytest.mark.parametrize("fit_mean,center", [(True, True), (True, False), (False, True), (False, False)])
def test_floating_mean_centring_and_normalisation(L, fit_mean, center, normalization):
    t, y, W = _record(1000, 3)
    _check(L, y, t, W, _freqs(), 3, fit_mean=fit_mean, center=center, normalization=normalization)


# ---- 2., 3. one term ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 3])
def test_one_term_through_the_new_entry_agrees_with_lombscargle(L, ns):
    import test_gpu_lomb as g4                                                # the single-term bounds, as that test holds them
    t, y, W = _record(1000, ns)
    f = _freqs()
    ya = y if ns > 1 else y[:, 0]
    tm, r, got, be = _check(L, ya, t, W, f, 1)
    assert (tm["ts"], tm["accumulators"]) == ((1, 6) if ns == 1 else (4, 12))
    P1, (a1, b1, c1), s1 = L.lombscargle(ya, t, f, W=W, path="direct", coef=True, return_sums=True)
    sums = _call(L, ya, t, f, 1, W)[2]
    for k in ("mean", "Y", "YY"):                                             # the same kernels produce them
        assert sums[k].tobytes() == s1[k].tobytes(), k
    r1 = lomb_ref(y, t, f, W=W, removed=np.array(s1["mean"]))
    b1e = g4._epilogue_bounds(r1, g4._sum_bounds(r1, t, y, W, False), True, False, len(t))
    for k, v, idx in (("power", P1.power, None), ("a", a1, 0), ("b", b1, 0), ("c", c1, None)):
        mine, bound = (got[k], be[k]) if idx is None else (got[k][idx], be[k][idx])
        assert np.all(np.abs(mine.astype(LD) - np.asarray(v).reshape(len(f), ns).astype(LD)) <= bound + b1e[k]), k


def test_the_default_is_untouched(L):
    t, y, W = _record(1000, 3)
    f = _freqs()
    one = L.lombscargle(y, t, f, W=W, coef=True, return_sums=True)
    L.lombscargle(y, t, f, W=W, nterms=2)                                     # (a call of the new entry in between changes nothing)
    two = L.lombscargle(y, t, f, W=W, coef=True, return_sums=True, nterms=1)
    assert L.lombscargle_last_timing()["path"] == "direct"
    assert one[0].power.tobytes() == two[0].power.tobytes()
    for x, z in zip(one[1], two[1]):
        assert x.tobytes() == z.tobytes()
    assert sorted(one[2]) == sorted(two[2]) == ["C", "C2", "S", "S2", "Y", "YC", "YS", "YY", "mean"]
    for k in one[2]:
        assert np.asarray(one[2][k]).tobytes() == np.asarray(two[2][k]).tobytes(), k
    assert L.lombscargle(y[:, 0], t, f).power.tobytes() == L.lombscargle(y[:, 0], t, f, nterms=1).power.tobytes()


# ---- 4. independence ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5])
def test_a_column_has_the_same_bits_alone_and_two_calls_agree(L, K):
    t, y, W = _record(1000, 5)
    f = _freqs()
    P, (a, b, c), s, _ = _call(L, y, t, f, K, W)
    P2, (a2, b2, c2), s2, _ = _call(L, y, t, f, K, W)
    for x, z in ((P.power, P2.power), (a, a2), (b, b2), (c, c2), *((s[k], s2[k]) for k in s)):
        assert np.asarray(x).tobytes() == np.asarray(z).tobytes()
    for q in range(5):
        Pq, (aq, bq, cq), sq, tq = _call(L, y[:, q], t, f, K, W)
        assert tq["ts"] == 1
        assert np.array_equal(P.power[:, q], Pq.power) and np.array_equal(a[:, :, q], aq) and np.array_equal(b[:, :, q], bq) and np.array_equal(c[:, q], cq), q
        assert np.array_equal(s["C"], sq["C"]) and np.array_equal(s["S"], sq["S"]) and np.array_equal(s["YC"][q], sq["YC"][0]) and np.array_equal(s["YS"][q], sq["YS"][0])
        assert s["Y"][q] == sq["Y"][0] and s["YY"][q] == sq["YY"][0] and s["mean"][q] == sq["mean"][0]


# ---- 5. degenerate frequencies -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fit_mean", [True, False])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_degenerate_frequencies_of_a_uniform_record(L, K, fit_mean):
    t, y, W = _uniform()
    f = np.array([0.0, 2.0, 4.0, 8.0, 1.25])
    tm, r, got, _ = _check(L, y, t, W, f, K, fit_mean=fit_mean)
    want = {1: {0.0, 8.0}, 2: {0.0, 4.0, 8.0}, 3: {0.0, 4.0, 8.0}, 4: {0.0, 2.0, 4.0, 8.0}}[K]
    assert set(f[r["degenerate"]]) == want and tm["degenerate"] == len(want)
    assert np.all(got["power"][~r["degenerate"]] > 0)                       # (the reference's pivots here: <= 2e-19 where degenerate, >= 0.48 elsewhere)


# ---- 6. a planted signal ---------------------------------------------------------------------------------------------------------------------------
def test_a_planted_record_of_three_harmonics(L):
    t, _, W = _record(1000, 1)
    y = planted(t)
    f = np.array([1.0, 1.25, 2.5])
    _, r, got, be = _check(L, y, t, W, f, 3)
    assert abs(got["power"][1, 0] - 1.0) <= float(be["power"][1, 0]) + 1e-15
    want = [(1.0, 0.0), (0.5 * np.sin(0.3), 0.5 * np.cos(0.3)), (-0.25, 0.0)]
    for h, (ah, bh) in enumerate(want):
        assert abs(got["a"][h, 1, 0] - ah) <= float(be["a"][h, 1, 0]) + 1e-15 and abs(got["b"][h, 1, 0] - bh) <= float(be["b"][h, 1, 0]) + 1e-15, h
    assert abs(got["c"][1, 0] - 0.75) <= float(be["c"][1, 0]) + 1e-15
    P2 = L.lombscargle(y, t, f, W=W, nterms=2).power
    assert P2[1] < 0.96 and L.lombscargle(y, t, f, W=W).power[1] < P2[1]


# ---- 7. a constant signal ----------------------------------------------------------------------------------------------------------------------
def test_a_constant_signal_has_standard_power_zero(L):
    t, _, W = _record(1000, 1)
    const = np.full(1000, 2.7)
    for center in (True, False):
        assert np.all(L.lombscargle(const, t, _freqs(), W=W, center_data=center, nterms=2).power == 0.0), center
    assert L.lombscargle_terms_last_timing()["degenerate"] == 0
    assert np.all(lomb_terms_ref(const, t, _freqs(), 2, W=W)["power"] == 0) and np.all(lomb_terms_ref(const, t, _freqs(), 2, W=W, center_data=False)["power"] == 0)


# ---- 8. errors -----------------------------------------------------------------------------------------------------------------------------------
def test_bad_inputs_raise_value_errors(L):
    t, y, W = _record(1000, 1)
    f = _freqs()
    for K in (0, 7):
        with pytest.raises(ValueError, match="nterms"):
            L.lombscargle(y[:, 0], t, f, nterms=K)
        with pytest.raises(ValueError, match="nterms must be 1 .. 6"):       # ... and the library's own refusal
            L.api._lombscargle_terms(y[:, 0], t, f, None, True, True, "standard", 0, False, False, K)
    with pytest.raises(ValueError, match="not implemented for several terms"):
        L.lombscargle(y[:, 0], t, np.arange(1, 71) / 64.0, path="nufft", nterms=2)
    yn = y[:, 0].copy(); yn[3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        L.lombscargle(yn, t, f, nterms=2)
    Wn = W.copy(); Wn[5] = -0.25
    with pytest.raises(ValueError, match="negative"):
        L.lombscargle(y[:, 0], t, f, W=Wn, nterms=2)
    for path in ("auto", "direct"):
        assert L.lombscargle(y[:, 0], t, f, W=W, path=path, nterms=2).power.shape == (70,)


def test_three_samples_cannot_carry_two_terms_and_a_mean(L):
    """Five unknowns, three samples: in exact arithmetic the third pivot is 0 at every frequency; in double it is a rounding residue (at most
    2e-15 on this record, worked in numpy), 500 times below the threshold 2^-40."""
    f = _freqs()
    P, (a, b, c) = L.lombscargle(np.array([1.0, -2.0, 0.5]), np.array([0.0, 0.25, 0.625]), f, nterms=2, coef=True)
    assert L.lombscargle_terms_last_timing()["degenerate"] == len(f)
    assert not P.power.any() and not a.any() and not b.any() and not c.any() and a.shape == (2, 70)


def test_worst_ratios_are_reported(L):
    """(Runs last: the worst error / bound of every quantity over the cases above, for DESIGN.md 4.15.)"""
    print("worst error / bound of this session:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())
