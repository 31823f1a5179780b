"""The references of CLEAN (tests/_clean_ref.py) checked on the host before the device is held to them (include/lpvspectral.h g11):
the float64 model of the loop recovers planted lines and makes the picks of the same loop in long double; every case the GPU runs is
unambiguous; what the loop removes from the residual is what it put into the components; and the rules -- inadmissible bins, ties, a
count of zero, the tol stop, the empty status.  CPU only.

CONSERVATION, the bound.  Entry k of D - R - sum_p [C_p Wn_{k-p} + conj(C_p) Wn_{k+p}] is a sum of the roundings of the loop.  A pick
touches an entry with four products, three additions and one subtraction per component (re, im): at most 4 u relative to the moduli
of what it adds, and C_p itself is a sum of at most `picks` values.  The loop's roundings are relative to intermediate residuals, which
are bounded by the sum of the moduli of all terms; so, per entry, |residue| <= (picks + 2) 4 u sum|terms| with
sum|terms| = |R_k| + sum_p |C_p| (|Wn_{k-p}| + |Wn_{k+p}|)."""
import functools

import numpy as np
import pytest

import _clean_ref as ref

U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _planted(seed):
    t, y, df, Nf = ref.planted_record(seed)
    case = dict(t=t, y=y[:, None], W=None, df=df, Nf=Nf)
    D, Wn = ref.host_spectra(case)
    m = ref.clean_model(D[0], Wn, 0.5, 300, 1e-6)
    ld = ref.clean_loop_ld(D[0], Wn, 0.5, 300, 1e-6)
    return D[0], Wn, m, ld


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_planted_lines_are_recovered(seed):
    D, Wn, m, ld = _planted(seed)
    C = ref.to_complex(*m["C"])
    amp = 2 * np.abs(C)
    others = np.delete(amp, [40, 93])
    print(f"seed {seed}: 2|C40| = {amp[40]:.6f}, 2|C93| = {amp[93]:.6f}, phases {np.angle(C[40]):.6f}, {np.angle(C[93]):.6f}, "
          f"largest other {others.max():.4f}, iterations {m['iterations']}, status {m['status']}, smallest gap {ld['gaps'].min():.3g}")
    assert abs(amp[40] - 1.0) <= 0.003 and abs(amp[93] - 0.6) <= 0.001
    assert abs(np.angle(C[40]) - 0.7) <= 1e-3 and abs(np.angle(C[93]) + 1.1) <= 1e-3
    assert others.max() <= 0.05
    # the model makes the long-double loop's picks, and its C and R are within 1e-15 of it
    assert m["iterations"] == ld["iterations"] and m["status"] == ld["status"]
    assert np.array_equal(m["picks"], ld["picks"])
    assert ld["gaps"].min() >= 2.0 ** -30
    for key in ("C", "R"):
        for a, b in zip(m[key], ld[key]):
            d = np.abs(a.astype(ref.LD) - b).max()
            print(f"seed {seed}: max |{key} - {key}_ld| = {float(d):.3g}")
            assert d < 1e-15


@pytest.mark.parametrize("name", sorted(ref.LOOP_CASES))
def test_every_gpu_case_is_unambiguous(name):
    """A condition on the INPUTS: in the long-double run, the best admissible P is ahead of the second best by a relative 2^-30 at every
    iteration (a signal with a single admissible bin has nothing to be confused with)."""
    case = ref.loop_case(name)
    D, Wn = ref.host_spectra(case)
    for c in range(case["ns"]):
        ld = ref.clean_loop_ld(D[c], Wn, case["gain"], case["niter"], case["tol"])
        if ld["admissible"].sum() < 2 or len(ld["gaps"]) == 0:
            continue
        print(f"{name}[{c}]: {ld['iterations']} iterations, status {ld['status']}, smallest gap {ld['gaps'].min():.3g}")
        assert ld["gaps"].min() >= 2.0 ** -30


@pytest.mark.parametrize("name", ["planted", "nf255", "nf1030", "nf257"])
def test_the_loop_conserves_the_dirty_spectrum(name):
    case = ref.loop_case(name)
    D, Wn = ref.host_spectra(case)
    m = ref.clean_model(D[0], Wn, case["gain"], case["niter"], case["tol"])
    residue, mag = ref.conservation(D[0], Wn, m["R"], m["C"])
    bound = (m["iterations"] + 2) * 4 * U * mag
    print(f"{name}: {m['iterations']} picks, max residue {float(residue.max()):.3g}, max |D| {np.abs(D[0]).max():.3g}, smallest bound {float(bound.min()):.3g}")
    assert np.all(residue <= bound)


def test_inadmissible_bins_of_a_uniform_record():
    """t = 0 .. 63 (step 1), df = 1/8, Nf = 7: Wn_2p = 1 where 2 p / 8 is an integer -- p = 0 and 4 -- the aliases of the zero frequency.  A line
    planted at the alias p = 4 (f = 1/2, the Nyquist frequency) is never picked, though it is the largest bin."""
    t = np.arange(64.0)
    y = 3.0 * np.cos(2 * np.pi * 0.5 * t) + np.cos(2 * np.pi * 0.125 * t + 0.3)
    D, Wn = ref.host_spectra(dict(t=t, y=y[:, None], W=None, df=0.125, Nf=7))
    m = ref.clean_model(D[0], Wn, 0.5, 20, 0.0)
    assert list(np.nonzero(~m["admissible"])[0]) == [0, 4]
    assert np.argmax(np.abs(D[0])) == 4
    assert 4 not in m["picks"] and 0 not in m["picks"] and m["picks"][0] == 1
    assert m["iterations"] == 20 and m["status"] == ref.NITER


def test_a_tie_goes_to_the_lowest_index():
    Wn = np.zeros(9, dtype=np.complex128)
    Wn[0] = 1.0                                                              # the window of a perfect sampling: every p > 0 is admissible
    D = np.array([9.0, 1.0, 2.0 + 1.0j, 1.0 - 2.0j, -2.0 - 1.0j])           # bins 2, 3, 4 share P = 5; bin 0 is the largest, and inadmissible
    m = ref.clean_model(D, Wn, 1.0, 3, 0.0)
    assert list(m["picks"]) == [2, 3, 4]
    ld = ref.clean_loop_ld(D, Wn, 1.0, 3, 0.0)
    assert list(ld["picks"]) == [2, 3, 4] and ld["gaps"][0] == 0.0


def test_no_iterations_returns_the_dirty_spectrum():
    D, Wn, _, _ = _planted(0)
    m = ref.clean_model(D, Wn, 0.5, 0, 0.0)
    assert np.array_equal(ref.to_complex(*m["R"]).view(np.uint8), D.view(np.uint8))
    assert not np.any(m["C"][0]) and not np.any(m["C"][1])
    assert m["iterations"] == 0 and m["status"] == ref.NITER and len(m["picks"]) == 0


def test_the_tol_stop_and_its_count():
    """With the window of a perfect sampling and gain g every pick multiplies its bin by 1 - g: lines of moduli 1 and 1/2 with g = 1/2 and
    tol = 1/8 are picked as 1, then (1/2, 1/2: the tie to the lower bin 1), 1/2, then (1/4, 1/4, 1/4) ... until the peak is <= 1/8."""
    Wn = np.zeros(9, dtype=np.complex128)
    Wn[0] = 1.0
    D = np.array([0.0, 1.0, 0.0, 0.5j, 0.0])
    m = ref.clean_model(D, Wn, 0.5, 100, 0.125)
    # peaks: 1 (bin 1), 1/2 (bin 1), 1/2 (bin 3), 1/4 (bin 1), 1/4 (bin 3), then 1/8 <= tol * 1: stop
    assert list(m["picks"][:5]) == [1, 1, 3, 1, 3] and m["iterations"] == 5 and m["status"] == ref.TOL
    assert np.all(m["picks"][5:] == -1)
    assert ref.clean_model(D, Wn, 0.5, 4, 0.125)["status"] == ref.NITER
    assert ref.clean_model(D, Wn, 0.5, 7, 0.0)["iterations"] == 7           # tol = 0 never stops


def test_the_empty_status():
    case = ref.loop_case("uniform")
    D, Wn = ref.host_spectra(case)
    m = ref.clean_model(D[0], Wn, 0.5, 300, 0.0)
    assert not m["admissible"].any()
    assert m["iterations"] == 0 and m["status"] == ref.EMPTY
    assert np.array_equal(ref.to_complex(*m["R"]).view(np.uint8), D[0].view(np.uint8))


def test_sigma_is_the_half_power_width_of_the_main_lobe():
    """|Wn|^2 = 1, 0.8, 0.4: the crossing of 1/2 lies 3/4 of the way from m = 1 to m = 2."""
    Wn = np.sqrt(np.array([1.0, 0.8, 0.4, 0.1, 0.0])).astype(np.complex128)
    P = Wn.real * Wn.real
    want = ((1.0 + (P[1] - 0.5) / (P[1] - P[2])) * 0.25) / np.sqrt(2 * np.log(2.0))
    assert abs(ref.clean_sigma(Wn, 0.25) - want) <= 4 * U * want


# ---- planted spectra: the closed forms the GPU's loop is held to (tests/test_gpu_clean.py) ----------------------------------------------------
def _planted_runs(Nf):
    D = ref.planted_spectra(Nf)
    return [ref.delta_oracle(D[c], 0.5, 2 * (Nf - 1) + 1, 0.0) for c in range(4)]


@pytest.mark.parametrize("Nf", [n for n in ref.PLANTED_NF if n <= ref.MODEL_NF_MOST] + [257, 1030])
def test_the_delta_window_oracle_equals_the_model(Nf):
    """Byte for byte on all four planted patterns, with the iteration count the GPU test uses."""
    D, Wn = ref.planted_spectra(Nf), ref.delta_window(Nf)
    for c, o in enumerate(_planted_runs(Nf)):
        m = ref.clean_model(D[c], Wn, 0.5, 2 * (Nf - 1) + 1, 0.0)
        assert not m["admissible"][0] and m["admissible"][1:].all() and m["den"][0] == 0.0 and np.all(m["den"][1:] == 1.0)
        assert ref.same_result(o, ref.model_as_complex(m)) is None, (Nf, c, ref.same_result(o, ref.model_as_complex(m)))


@pytest.mark.parametrize("Nf", [2, 257, 1030, 4096, 8193])
def test_equal_peaks_are_picked_in_index_order(Nf):
    """All P equal: the picks walk the admissible bins in increasing index, round after round, each pick halving its bin; pattern 2 takes
    its bins of modulus 5 three times (25, 25/4, 25/16 > 1) before any other; an all-zero spectrum picks bin 1 with value 0 every time."""
    K, n = Nf - 1, 2 * (Nf - 1) + 1
    runs = _planted_runs(Nf)
    D = ref.planted_spectra(Nf)
    i = np.arange(n)
    for c in (0, 1):
        o = runs[c]
        assert np.array_equal(o["picks"], 1 + i % K) and o["iterations"] == n and o["status"] == ref.NITER
        want = 0.5 ** (1 + i // K) * D[c][1 + i % K]
        assert o["pick_values"].tobytes() == want.astype(np.complex128).tobytes()
        assert np.array_equal(o["R"][2:], D[c][2:] / 4) and o["R"][1] == D[c][1] / 8 and o["R"][0] == D[c][0] and o["C"][0] == 0
    big = np.arange(1, Nf, 64)
    assert np.array_equal(runs[2]["picks"][:min(n, 3 * len(big))], np.tile(big, 3)[:n])
    if n > 3 * len(big):
        rest = np.setdiff1d(np.arange(1, Nf), big)
        assert np.array_equal(runs[2]["picks"][3 * len(big):][:len(rest)], rest[:n - 3 * len(big)])
    assert np.all(runs[3]["picks"] == 1) and not runs[3]["pick_values"].any() and not runs[3]["R"].any() and not runs[3]["C"].any()
    assert all(r["admissible"] == K for r in runs)


@pytest.mark.parametrize("Nf", [2, 257, 1030])
def test_the_stop_at_equality(Nf):
    """bP <= thr WITH equality: all bins 5, tol = 2^-3: thr = 25 / 64, and each bin is picked at 25, 25/4 and 25/16 -- 3 (Nf - 1) picks --
    before every P equals thr; with gain 1 a pick zeroes its bin and the loop stops after Nf - 1.  tol = 0 never stops: the picks beyond
    Nf - 1 fall on bin 1 with value 0."""
    K = Nf - 1
    D, Wn = ref.planted_spectra(Nf)[0], ref.delta_window(Nf)
    for kw, iters, status in ((dict(gain=0.5, niter=3 * K + 7, tol=2.0 ** -3), 3 * K, ref.TOL), (dict(gain=1.0, niter=3 * K + 7, tol=2.0 ** -3), K, ref.TOL),
                              (dict(gain=1.0, niter=Nf + 5, tol=0.0), Nf + 5, ref.NITER)):
        o, m = ref.delta_oracle(D, **kw), ref.model_as_complex(ref.clean_model(D, Wn, **kw))
        assert ref.same_result(o, m) is None
        assert (o["iterations"], o["status"]) == (iters, status), (kw, o["iterations"], o["status"])
        assert np.all(o["picks"][iters:] == -1)
    assert np.all(o["picks"][K:] == 1) and not o["pick_values"][K:].any() and len(o["picks"][K:]) == 6
    assert ref.clean_model(ref.planted_spectra(257)[0], ref.delta_window(257), 0.5, 800, 2.0 ** -3)["iterations"] == 768


def test_peaks_that_overflow_tie_at_infinity():
    D = np.full(8, complex(1e200, 0.0))
    o, m = ref.delta_oracle(D, 0.5, 20, 0.0), ref.clean_model(D, ref.delta_window(8), 0.5, 20, 0.0)
    assert ref.same_result(o, ref.model_as_complex(m)) is None
    assert np.all(o["picks"] == 1) and o["iterations"] == 20 and o["status"] == ref.NITER
    assert np.array_equal(o["pick_values"], 1e200 * 0.5 ** np.arange(1, 21)) and np.all(np.isfinite(o["R"].view(np.float64))) and np.all(o["R"][2:] == 1e200)
    assert float(o["R"][1].real) * float(o["R"][1].real) == np.inf                                       # ... still +inf at the last pick: every one was decided by the index


@pytest.mark.parametrize("Nf", [257, 1030])
def test_sidelobes_after_a_tie_of_every_bin(Nf):
    """The inputs of the sidelobe case: every admissible bin ties at iteration 0, nothing overflows, and the update pass is not trivial
    (the picks are not those of the delta window)."""
    Wn = ref.sidelobe_window(Nf)
    for c in (0, 1):
        D = ref.planted_spectra(Nf)[c]
        ld = ref.clean_loop_ld(D, Wn, 0.5, 300, 0.0)
        m = ref.clean_model(D, Wn, 0.5, 300, 0.0)
        assert ld["gaps"][0] == 0.0 and m["picks"][0] == 1 and m["admissible"].sum() == Nf - 1 and m["den"][1] == 1.0 - 2.0 ** -8
        assert m["iterations"] == 300 and all(np.isfinite(a).all() for a in m["R"] + m["C"])
        assert not np.array_equal(m["picks"], ref.delta_oracle(D, 0.5, 300, 0.0)["picks"])


def test_the_cut_is_found_by_search_and_decides_admission():
    at, above, below = ref.cut_doubles()
    den = lambda w: np.float64(1.0) - np.float64(w) * np.float64(w)            # noqa: E731
    assert den(above) > ref.MIN_DEN > den(below) and den(above) - ref.MIN_DEN <= 2.0 ** -52 and ref.MIN_DEN - den(below) <= 2.0 ** -52      # (neighbouring squares: 2^-52 apart)
    assert at is None or (den(at) == ref.MIN_DEN and below > at > above)
    D, Wn, found = ref.cut_case()
    assert found == (at is not None)
    for c in range(2):
        m = ref.clean_model(D[c], Wn, 0.5, 60, 0.0)
        assert list(np.flatnonzero(~m["admissible"])) == [0] + sorted(ref.CUT_BINS["below"])
        assert np.abs(D[c]).argmax() in ref.CUT_BINS["below"] and not set(ref.CUT_BINS["below"]) & set(m["picks"].tolist())
        assert m["picks"][0] == ref.CUT_BINS["above"][2] and m["picks"][1] == ref.CUT_BINS["at"][2]       # the first picks sit just above and AT the cut
        assert m["iterations"] == 60 and all(np.isfinite(a).all() for a in m["R"] + m["C"])
        waves = lambda bins: sorted((p % 256) >> 6 for p in bins)             # noqa: E731
        assert all(len(set(waves(b))) == 3 for b in ref.CUT_BINS.values())
