"""lombscargle_bootstrap on the GPU (csrc/lomb_boot.hip; include/lpvspectral.h g6) against the long-double reference of tests/_lomb_ref.py
evaluated on the resampled signals y[pi_b], the indices pi_b from this file's own statement of the stream (Python integers on
tests/_cnormal_ref.uniform_words), not from the package.

INPUTS, as in tests/test_gpu_lomb.py: t in multiples of 2^-10 over 40 units, 70 distinct frequencies in multiples of 2^-6 in (0, 3] -- two
tiles of frequencies, the second partial -- so that every product f t is exact; W uniform in [0.5, 2]; y = 0.5 randn + 0.75, the "tone"
records with 0.6 cos(2 pi 1.25 t + 0.3) added.  N = 301 (odd: half of the last pair of the stream, one partial stage of samples) and
N = two slabs + 453 of the plan's slab (read from last_timing); B = 37 (no multiple of either TS); seed 5.

One case more, on the long record: t over [0, 2^20] (on the 2^-10 lattice, and as full-mantissa doubles) and full-mantissa frequencies in
(0, 3] (tests/_lomb_ref.py): every product f t is inexact, and the trigonometry allowance is 6 u.

TIES.  On these records two powers of a column never share their bits, and the only tie is the all-zero column of a constant signal.
Section 6 plants them: f = (f0, f0), every frequency twice, makes every resample's maximum a tie of the indices k and k + len(f0) --
len(f0) = 70: partners in other threads and tiles; 256 (multiples of 2^-6 up to 4): partners in the same thread's stride of the epilogue;
200: the higher partner in a LOWER thread, which the tree's tie clause has to undo.

BOUNDS (u = 2^-53): those tests/test_gpu_lomb.py derives for direct sums -- every raw sum within (N + 16) u sum|terms| + 4 u per term of
trigonometry -- passed through the epilogue to first order by the REFERENCE's D (its _sum_bounds / _epilogue_bounds, imported).  The
reference is centred with the means the device reports (held to (N + 16) u sum w|y*|), as there.  Precondition, asserted: the reference's
D >= 0.01 off the degenerate set.  The reductions (maximum, argmax), the independence of B, row0, chunks and power_out, and the
repeatability are exact: bit for bit."""
import functools
import math

import numpy as np
import pytest

from _cnormal_ref import uniform_words
from _lomb_ref import LD, late_times, lomb_ref, wide_freqs
from test_gpu_lomb import _epilogue_bounds, _irregular, _ratio, _sum_bounds

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
B, SEED, NF = 37, 5, 70
SLAB = 1024                                                                    # asserted against last_timing below
N_SMALL, N_LONG = 301, 2 * SLAB + 453


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _record(N, tone=False, rec=None):
    """rec = "lattice" / "full": times over [0, 2^20] on multiples of 2^-10 / as full-mantissa doubles (tests/_lomb_ref.py)."""
    rng = np.random.default_rng(77 + N)
    t = late_times(rng, N, rec == "lattice") if rec else np.sort(rng.integers(0, 40 * 1024, N) / 1024.0)
    y = 0.5 * rng.standard_normal(N) + 0.75
    W = rng.uniform(0.5, 2.0, N)
    if tone:
        y = y + 0.6 * np.cos(2 * np.pi * 1.25 * t + 0.3)
    for a in (t, y, W):
        a.setflags(write=False)
    return t, y, W


@functools.lru_cache(maxsize=None)
def _f(rec=None):
    """The 70 frequencies: multiples of 2^-6, or with rec full-mantissa doubles in (0, 3] (every product f t inexact)."""
    if not rec:
        return _irregular(NF)
    f = wide_freqs(np.random.default_rng(770), NF)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def _indices(N, nb, seed=SEED, row0=0):
    """pi_b(i), b = row0 .. row0 + nb - 1: sample 2p takes (w0 << 32) | w1, sample 2p + 1 takes (w2 << 32) | w3; pi = (u N) >> 64."""
    i = np.arange(N)
    w0, w1, w2, w3 = (w.astype(object) for w in uniform_words(seed, (row0 + np.arange(nb))[:, None], (i >> 1)[None, :]))
    u = np.where((i & 1).astype(bool)[None, :], w2 * (1 << 32) + w3, w0 * (1 << 32) + w1)
    idx = np.array((u * N) // (1 << 64), dtype=np.int64)
    assert idx.shape == (nb, N) and idx.min() >= 0 and idx.max() < N
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def _ref(N, tone, weighted, fit_mean, center, normalization, removed, nb=B, seed=SEED, rec=None):
    """The reference on the nb resampled signals (N x nb); removed: the device's means as a tuple, or None (the reference's own)."""
    t, y, W = _record(N, tone, rec)
    ys = y[_indices(N, nb, seed)].T
    return lomb_ref(ys, t, _f(rec), W=W if weighted else None, fit_mean=fit_mean, center_data=center, normalization=normalization,
                    removed=None if removed is None else np.array(removed))


def _boot(L, N, tone=False, weighted=True, nb=B, rec=None, **kw):
    t, y, W = _record(N, tone, rec)
    kw.setdefault("seed", SEED)
    kw.setdefault("f", _f(rec))
    return L.lombscargle_bootstrap(y, t, W=W if weighted else None, B=nb, return_argmax=True, return_means=True, return_power=True, **kw)


def _check_numerics(L, N, weighted, fit_mean, center, normalization, want_ts=16, rec=None):
    t, y, W = _record(N, rec=rec)
    M, am, means, P = _boot(L, N, weighted=weighted, rec=rec, fit_mean=fit_mean, center_data=center, normalization=normalization)
    tm = L.lombscargle_bootstrap_last_timing()
    assert tm["resamples"] == B and tm["ts"] == want_ts and tm["slab"] == SLAB and tm["slabs"] == math.ceil(N / SLAB) and tm["degenerate"] == 0
    assert P.shape == (NF, B) and M.shape == am.shape == means.shape == (B,)
    r = _ref(N, False, weighted, fit_mean, center, normalization, tuple(means) if center else None, rec=rec)
    deg = r["degenerate"]
    assert not deg.any() and np.all(r["D"] >= 0.01), "the inputs are to stay clear of the degenerate threshold"
    ys = y[_indices(N, B)].T
    bs = _sum_bounds(r, t, ys, W if weighted else np.ones(N), False, trig=6 if rec else 4)
    err = np.abs(means.astype(LD) - r["mean"])
    print("mean: worst error / bound:", _ratio(err, bs["mean"]))
    assert np.all(err <= bs["mean"])
    be = _epilogue_bounds(r, bs, fit_mean, normalization == "psd", N)["power"]
    err = np.abs(P.astype(LD) - r["power"])
    print("power: worst error / bound:", _ratio(err, be), "largest power", float(P.max()))
    assert np.all(err <= be), _ratio(err, be)
    assert np.all(be < 1e-9 * np.maximum(1, np.abs(r["power"]).max())), "the bound is a rounding bound"
    if normalization == "standard" and fit_mean:
        assert np.all(P >= 0.0) and np.all(P <= 1.0 + 1e-12)
    return M, am, means, P


# ---- 1. numerics ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("normalization", ["standard", "psd"])
@pytest.mark.parametrize("fit_mean,center", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("N", [N_SMALL, N_LONG])
def test_every_column_is_the_estimate_of_its_resample(L, monkeypatch, N, fit_mean, center, normalization, weighted):
    monkeypatch.delenv("LPVS_LOMB_BOOT_TS", raising=False)
    monkeypatch.delenv("LPVS_LOMB_BOOT_MB", raising=False)
    _check_numerics(L, N, weighted, fit_mean, center, normalization)


@pytest.mark.parametrize("rec", ["lattice", "full"])
def test_every_column_of_a_record_with_inexact_products(L, monkeypatch, rec):
    """t over [0, 2^20], f full-mantissa doubles in (0, 3]: f t reaches 3e6 turns and the low word of lomb_sincos in lomb_boot_kernel
    decides; three slabs, every column against the reference on its resampled indices (6 u of trigonometry per term in place of 4 u,
    tests/test_gpu_lomb.py)."""
    monkeypatch.delenv("LPVS_LOMB_BOOT_TS", raising=False)
    monkeypatch.delenv("LPVS_LOMB_BOOT_MB", raising=False)
    _check_numerics(L, N_LONG, True, True, True, "standard", rec=rec)


# ---- 2. the reduction, exact -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalization", ["standard", "psd"])
@pytest.mark.parametrize("N", [N_SMALL, N_LONG])
def test_maximum_and_argmax_are_those_of_the_devices_own_column(L, monkeypatch, N, normalization):
    monkeypatch.delenv("LPVS_LOMB_BOOT_TS", raising=False)
    monkeypatch.delenv("LPVS_LOMB_BOOT_MB", raising=False)
    t, y, W = _record(N)
    M, am, means, P = _boot(L, N, normalization=normalization)
    assert np.array_equal(M, P.max(axis=0)) and np.array_equal(am, P.argmax(axis=0))       # (numpy's argmax: the first of equal values)
    M2, am2 = L.lombscargle_bootstrap(y, t, _irregular(NF), W=W, B=B, seed=SEED, normalization=normalization, return_argmax=True)   # power_out = NULL
    assert M2.tobytes() == M.tobytes() and np.array_equal(am2, am)
    assert np.array_equal(L.lombscargle_bootstrap(y, t, _irregular(NF), W=W, B=B, seed=SEED, normalization=normalization), M)


# ---- 3. independence and reproducibility ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,small_mb", [(N_SMALL, "0.01"), (N_LONG, "0.06")])
def test_same_bits_twice_alone_and_cut_into_chunks(L, monkeypatch, N, small_mb):
    monkeypatch.delenv("LPVS_LOMB_BOOT_TS", raising=False)
    monkeypatch.delenv("LPVS_LOMB_BOOT_MB", raising=False)
    first = _boot(L, N)
    assert L.lombscargle_bootstrap_last_timing()["chunks"] == 1
    for a, b in zip(first, _boot(L, N)):
        assert a.tobytes() == b.tobytes()
    M, am, means, P = first
    for b in (0, 15, 16, 36):                                                  # first and last row of a block of 16, the last of the call
        Mb, ab, mb, Pb = _boot(L, N, nb=1, row0=b)
        assert Pb[:, 0].tobytes() == P[:, b].tobytes() and Mb[0] == M[b] and ab[0] == am[b] and mb[0] == means[b], b
    half = _boot(L, N, nb=20, row0=17)                                         # another B, another row0: the rows 17 .. 36
    for a, b in zip(half, (M[17:], am[17:], means[17:], P[:, 17:])):
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
    # 1120 (N = 301) and 3360 (three slabs) bytes of partial sums per resample: 9 and 18 fit, one block of 16 per chunk, 16 + 16 + 5
    monkeypatch.setenv("LPVS_LOMB_BOOT_MB", small_mb)
    cut = _boot(L, N)
    assert L.lombscargle_bootstrap_last_timing()["chunks"] == 3
    for a, b in zip(first, cut):
        assert a.tobytes() == b.tobytes()
    monkeypatch.delenv("LPVS_LOMB_BOOT_MB")
    other = _boot(L, N, seed=6)                                                # another seed: other indices
    assert not np.array_equal(other[0], M) and not np.array_equal(other[2], means)


@pytest.mark.parametrize("N", [N_SMALL, N_LONG])
def test_the_other_instantiation_agrees_within_the_bound(L, monkeypatch, N):
    monkeypatch.delenv("LPVS_LOMB_BOOT_MB", raising=False)
    monkeypatch.setenv("LPVS_LOMB_BOOT_TS", "8")
    M8, am8, means8, P8 = _check_numerics(L, N, True, True, True, "standard", want_ts=8)    # 37 = 4 blocks of 8 + 5
    monkeypatch.delenv("LPVS_LOMB_BOOT_TS")
    M, am, means, P = _boot(L, N)
    assert L.lombscargle_bootstrap_last_timing()["ts"] == 16
    assert means8.tobytes() == means.tobytes()                                 # the moments do not depend on TS
    assert np.array_equal(M8, P8.max(axis=0)) and np.array_equal(am8, P8.argmax(axis=0))
    monkeypatch.setenv("LPVS_LOMB_BOOT_TS", "8")
    monkeypatch.setenv("LPVS_LOMB_BOOT_MB", "0.01" if N == N_SMALL else "0.06")
    cut = _boot(L, N)                                                          # 9 / 18 fit: chunks of 8 / 16
    assert L.lombscargle_bootstrap_last_timing()["chunks"] == (5 if N == N_SMALL else 3)
    assert cut[3].tobytes() == P8.tobytes() and cut[0].tobytes() == M8.tobytes()


# ---- 4. edges ---------------------------------------------------------------------------------------------------------------------------------
def test_the_zero_frequency_is_degenerate_once_and_gives_zeros(L):
    t, y, W = _record(N_SMALL)
    f = np.concatenate([_irregular(NF)[:5], [0.0], _irregular(NF)[5:]])
    M, am, P = L.lombscargle_bootstrap(y, t, f, W=W, B=B, seed=SEED, return_argmax=True, return_power=True)
    assert L.lombscargle_bootstrap_last_timing()["degenerate"] == 1
    assert np.all(P[5] == 0.0) and np.all(am != 5) and np.all(M > 0)
    rest = _boot(L, N_SMALL)
    assert np.array_equal(np.delete(P, 5, axis=0), rest[3])                   # a frequency's sums do not depend on its place in a tile


def test_a_constant_signal_has_maxima_zero(L):
    t, y, W = _record(N_SMALL)
    const = np.full(N_SMALL, 2.7)
    for center in (True, False):
        M, am, P = L.lombscargle_bootstrap(const, t, _irregular(NF), W=W, B=B, seed=SEED, center_data=center, return_argmax=True, return_power=True)
        assert np.all(P == 0.0) and np.all(M == 0.0) and np.all(am == 0), center
    assert L.false_alarm_probability(0.0, const, t, _irregular(NF), W=W, method="bootstrap", B=B, seed=SEED) == 1.0
    assert L.false_alarm_probability(1e-300, const, t, _irregular(NF), W=W, method="bootstrap", B=B, seed=SEED) == 0.0


def test_one_resample_one_frequency_one_sample(L):
    t, y, W = _record(N_SMALL)
    f = _irregular(NF)
    full = _boot(L, N_SMALL)
    M, am, means, P = _boot(L, N_SMALL, nb=1)                                  # B = 1
    assert P.shape == (NF, 1) and P[:, 0].tobytes() == full[3][:, 0].tobytes() and M[0] == full[0][0]
    M, am, means, P = _boot(L, N_SMALL, f=f[40:41])                            # Nf = 1
    assert P.shape == (1, B) and np.array_equal(M, P[0]) and np.all(am == 0) and np.array_equal(P[0], full[3][40])
    M, am, means, P = L.lombscargle_bootstrap(y[:1], t[:1], f, B=B, seed=SEED, return_argmax=True, return_means=True, return_power=True)   # N = 1, fit_mean
    assert L.lombscargle_bootstrap_last_timing()["degenerate"] == NF
    assert np.all(P == 0.0) and np.all(M == 0.0) and np.all(am == 0) and np.all(means == y[0])


def test_bad_inputs_raise_what_lombscargle_raises(L):
    from lpvspectral_jl_amd._lib import lib, check, out_ptr
    t, y, W = _record(N_SMALL)
    f = _irregular(7)
    tn = t.copy(); tn[17] = np.nan
    yi = y.copy(); yi[3] = np.inf
    Wn = W.copy(); Wn[5] = -0.25
    Wi = W.copy(); Wi[300] = np.inf
    for args, kw, match in (((y, tn, f), {}, "not finite"), ((yi, t, f), {}, "not finite"), ((y, t, f), {"W": Wi}, "not finite"), ((y, t, f), {"W": Wn}, "negative"),
                            ((y, t, f), {"W": np.zeros(N_SMALL)}, "sum to"), ((y, t, np.array([0.5, np.nan])), {}, "not finite")):
        with pytest.raises(ValueError, match=match) as mine:
            L.lombscargle_bootstrap(*args, B=4, **kw)
        with pytest.raises(ValueError, match=match) as theirs:               # the same wording as lombscargle
            L.lombscargle(*args, **kw)
        assert str(mine.value) == str(theirs.value)
    for kw in ({"B": 0}, {"B": -3}, {"B": 4, "row0": -1}):
        with pytest.raises(ValueError, match="need N > 0"):
            L.lombscargle_bootstrap(y, t, f, **kw)
    with pytest.raises(ValueError):
        L.lombscargle_bootstrap(y[:0], t[:0], f, B=4)                          # N < 1
    with pytest.raises(ValueError):
        L.lombscargle_bootstrap(y, t, f[:0], B=4)                              # Nf < 1
    with pytest.raises(ValueError):
        L.lombscargle_bootstrap(y, t, f, B=4, normalization="density")
    with pytest.raises(ValueError):
        L.lombscargle_bootstrap(np.stack([y, y], axis=1), t, f, B=4)           # one signal
    with pytest.raises(NotImplementedError, match="2\\^40"):
        L.lombscargle_bootstrap(y, t, f, B=4, row0=(1 << 40) - 3)
    assert L.lombscargle_bootstrap(y, t, f, B=4, row0=(1 << 40) - 4).shape == (4,)
    # sizes no test can allocate: refused by the plan before any memory is touched (the arrays passed are the small ones)
    out = np.zeros(4)

    def raw(N, Nf, nb):
        check(lib().lpvs_lombscargle_bootstrap_f64(out_ptr(y), out_ptr(t), N, None, out_ptr(f), Nf, nb, SEED, 0, 1, 1, 0, 0, out_ptr(out), None, None, None))
    with pytest.raises(NotImplementedError, match="2\\^31 or more"):
        raw(1 << 31, 7, 4)
    with pytest.raises(NotImplementedError, match="too many"):
        raw(N_SMALL, (1 << 24) + 1, 4)
    with pytest.raises(NotImplementedError, match="more than one call takes"):
        raw(N_SMALL, 7, 1 << 31)
    with pytest.raises(NotImplementedError):                                    # ... as lombscargle refuses a grid beyond 2^24
        check(lib().lpvs_lombscargle_f64(out_ptr(y), 1, out_ptr(t), N_SMALL, None, out_ptr(f), (1 << 24) + 1, 1, 1, 0, 1, 0, out_ptr(out), None, None))


# ---- 5. the estimate --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalization", ["standard", "psd"])
@pytest.mark.parametrize("tone", [False, True])
@pytest.mark.parametrize("N", [301, 1000])
def test_the_false_alarm_count_is_that_of_the_long_double_reference(L, monkeypatch, N, tone, normalization):
    monkeypatch.delenv("LPVS_LOMB_BOOT_TS", raising=False)
    monkeypatch.delenv("LPVS_LOMB_BOOT_MB", raising=False)
    nb = 64
    t, y, W = _record(N, tone)
    f = _irregular(NF)
    z0 = float(L.lombscargle(y, t, f, W=W, normalization=normalization).power.max())
    M, am = L.lombscargle_bootstrap(y, t, f, W=W, B=nb, seed=SEED, normalization=normalization, return_argmax=True)
    r = _ref(N, tone, True, True, True, normalization, None, nb=nb)            # the reference's own centring: nothing of the device in it
    Mref = r["power"].max(axis=0)
    gap = float(np.min(np.abs(Mref - z0)) / z0)
    top2 = np.sort(r["power"], axis=0)[-2:]
    print("N", N, "tone", tone, normalization, "z0", z0, "count", int(np.sum(Mref >= z0)), "closest maximum (relative)", gap,
          "two largest powers apart by at least", float(np.min(top2[1] - top2[0]) / np.max(top2[1])))
    assert gap > 1e-6, "a condition on the inputs: no reference maximum within 1e-6 of the observed peak"
    count = int(np.sum(M >= z0))
    assert count == int(np.sum(Mref >= z0))
    assert np.array_equal(am, np.argmax(r["power"], axis=0))
    assert L.false_alarm_probability(z0, y, t, f, W=W, method="bootstrap", maxima=M, normalization=normalization) == count / nb
    assert L.false_alarm_probability(z0, y, t, f, W=W, method="bootstrap", B=nb, seed=SEED, normalization=normalization) == count / nb
    if tone:
        assert count == 0                                                      # the tone stands far above every resample's maximum
    Ms = np.sort(M)
    for p in (0.5, 0.1, 0.01, 1.0):
        k = min(max(math.ceil((1.0 - p) * nb), 1), nb)
        assert L.false_alarm_level(p, y, t, f, W=W, method="bootstrap", maxima=M, normalization=normalization) == Ms[k - 1], p
    assert L.false_alarm_level(0.1, y, t, f, W=W, method="bootstrap", B=nb, seed=SEED, normalization=normalization) == Ms[57]   # ceil(0.9 64) = 58


# ---- 6. planted ties: every frequency twice -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", [70, 200, 256])
@pytest.mark.parametrize("normalization", ["standard", "psd"])
def test_duplicated_frequencies_tie_and_the_lower_index_wins(L, monkeypatch, n0, normalization):
    """f = (f0, f0): every power occurs twice, bit for bit, so EVERY resample's maximum is a tie of the indices k and k + n0, and only the
    rule -- the lower index -- says which is reported.  n0 = 70: the partners sit in different threads and tiles of the sums and in
    different threads of the epilogue; n0 = 256: in the same thread's stride of the epilogue, 256 apart; n0 = 200: for k >= 56 the
    partner k + 200 is the SECOND frequency of thread k - 56, so a lower thread brings the higher index into the tree and the tree's
    own tie clause has to hand the maximum to thread k's index."""
    monkeypatch.delenv("LPVS_LOMB_BOOT_TS", raising=False)
    monkeypatch.delenv("LPVS_LOMB_BOOT_MB", raising=False)
    t, y, W = _record(N_SMALL)
    f0 = _irregular(n0) if n0 <= 192 else np.arange(1, n0 + 1) / 64.0          # multiples of 2^-6: every product f t is exact
    assert len(np.unique(f0)) == n0
    kw = dict(W=W, B=B, seed=SEED, normalization=normalization, return_argmax=True, return_power=True)
    M, am, P = L.lombscargle_bootstrap(y, t, np.concatenate([f0, f0]), **kw)
    M0, am0, P0 = L.lombscargle_bootstrap(y, t, f0, **kw)
    assert P.shape == (2 * n0, B) and P[:n0].tobytes() == P[n0:].tobytes()
    assert np.all(am < n0) and np.array_equal(am, P[:n0].argmax(axis=0))
    assert M.tobytes() == M0.tobytes() and np.array_equal(am, am0) and P[:n0].tobytes() == P0.tobytes()
    assert len(set(am.tolist())) > 1                                           # (the ties are met at more than one index)
    # without the columns (power_out = NULL): the same reduction
    M2, am2 = L.lombscargle_bootstrap(y, t, np.concatenate([f0, f0]), W=W, B=B, seed=SEED, normalization=normalization, return_argmax=True)
    assert M2.tobytes() == M.tobytes() and np.array_equal(am2, am)
