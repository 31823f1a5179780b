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
