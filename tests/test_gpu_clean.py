"""CLEAN on the GPU (include/lpvspectral.h g11; csrc/clean.hip, csrc/clean_plan.h) against the references of tests/_clean_ref.py (their
own checks: tests/test_clean_ref_host.py).

INPUTS.  The exact-phase family of tests/_bls_ref.py: t in multiples of 2^-10, df = 2^-6, so every product (m df) t is exact in double
and the reference's phases are beyond dispute.  Every such record carries noise, so two bins with bit-equal P never meet, no den lies
near the cut 2^-20 and the stop never meets equality: on those inputs the tie rule decides nothing.
PLANTED (tests/_clean_ref.py: planted_spectra, delta_window, sidelobe_window, cut_case).  clean_loop takes any finite D and Wn, so what the
records never produce is planted: on the delta window Wn = (1, 0, ...) four spectra per call -- all bins 5; the Gaussian integers of
modulus 5 in turn (equal P, different bits); modulus 5 at the bins 1 + 64 j only (the same lane of every wave and stride); zero -- at
Nf = 256 w - 1 for EVERY wave count w = 1 .. 16 and at 2, 3, 65, 8192, 8193, with 2 (Nf - 1) + 1 iterations; the stop at equality; peaks
of +inf; dyadic sidelobes; den exactly at the cut and one double to either side.  All arithmetic on these is exact, so the expected
result is a closed form, stated by delta_oracle without the model; the model is compared too up to Nf = 1030.  The restoration's
compaction gets every bin, no bin, the ends of its chunks of 256, and parts that are zero, negative zero or imaginary alone.
BOUNDS (u = 2^-53).
  sums, direct path   |sum - ref| <= (N + 16) u sum|terms| + 4 u per term of trigonometry, the bound tests/test_gpu_lomb.py holds the same
                      kernels to; transform path: its 1e-12 sum|terms|.  The device centres with its own weighted means, which it does
                      not report here; they are sums like the others, within (N + 16) u sum w|y| of the reference's, and a change of the
                      mean by d moves D_k by d Wn_k, |Wn_k| <= 1: that allowance is added to the bound of D.
  the loop            none: picks, pick values, C, R, iterations and status equal the float64 model's through .view(uint8), fed with the
                      device's own D and Wn.
  conservation        (picks + 2) 4 u sum|terms| per entry (derived in tests/test_clean_ref_host.py).
  restoration         (ncomp + 2) 4 u sum|terms| per entry against the long-double gather: per component two products and an addition
                      into the sum, the beam's exp and its rounded argument."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _clean_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
KNOB = "LPVS_CLEAN_RESIDUAL"
LAST_LDS = 8192                                                               # csrc/clean_plan.h: 16 Nf <= 128 KiB


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------
SUM_SHAPES = [(1, 2, 1), (257, 257, 3), (1500, 1030, 1), (257, 1030, 3), (1500, 2, 3), (1, 257, 1)]


@functools.lru_cache(maxsize=None)
def _sum_ref(N, Nf, ns, weighted):
    t, y, W = ref.exact_record(7 * N + Nf + ns, N, ns)
    return (t, y, W if weighted else None) + ref.sums_ld(y, t, 2.0 ** -6, Nf, W=W if weighted else None)


@pytest.mark.parametrize("path", ["direct", "nufft"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("N,Nf,ns", SUM_SHAPES)
def test_dirty_spectrum_and_window_against_long_double_sums(L, N, Nf, ns, weighted, path):
    t, y, W, (Dre, Dim), (Wre, Wim), (aDre, aDim), (aWre, aWim), swyc, swy = _sum_ref(N, Nf, ns, weighted)
    D, Wn = L.dirty_spectrum(y, t, df=2.0 ** -6, Nf=Nf, W=W, path=path)
    assert L.clean_last_timing()["path"] == path
    assert D.shape == (ns, Nf) and Wn.shape == (2 * Nf - 1,) and D.dtype == Wn.dtype == np.complex128
    mean_allowance = (N + 16) * U * swy[:, None]
    if path == "direct":
        bW = [(N + 16) * U * a + 4 * U for a in (aWre, aWim)]
        bD = [(N + 16) * U * a + 4 * U * swyc[:, None] + mean_allowance for a in (aDre, aDim)]
    else:
        bW = [1e-12 * a for a in (aWre, aWim)]
        bD = [1e-12 * a + mean_allowance for a in (aDre, aDim)]
    for name, got, want, bound in (("Re Wn", Wn.real, Wre, bW[0]), ("Im Wn", Wn.imag, Wim, bW[1]), ("Re D", D.real, Dre, bD[0]), ("Im D", D.imag, Dim, bD[1])):
        err = np.abs(got.astype(ref.LD) - want)
        worst = float(np.max(err / np.maximum(bound, np.finfo(np.float64).tiny)))
        print(f"N={N} Nf={Nf} ns={ns} W={weighted} {path}: {name} max err {float(err.max()):.3g}, worst err / bound {worst:.3g}")
        assert np.all(err <= bound), name


# ---- the loop, bit for bit ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _device_spectra(name):
    import lpvspectral_jl_amd as L
    case = ref.loop_case(name)
    D, Wn = L.dirty_spectrum(case["y"], case["t"], df=case["df"], Nf=case["Nf"], W=case["W"], path="direct")
    for a in (D, Wn):
        a.setflags(write=False)
    return case, D, Wn


@functools.lru_cache(maxsize=None)
def _model(name, c):
    case, D, Wn = _device_spectra(name)
    return ref.clean_model(D[c], Wn, case["gain"], case["niter"], case["tol"])


def _compare_with_model(name, out, signals=None):
    case, D, Wn = _device_spectra(name)
    R, Cc, picks, pv, iters, status = out
    for i, c in enumerate(range(case["ns"]) if signals is None else signals):
        m = _model(name, c)
        mpv = ref.to_complex(*m["pick_values"])
        differ = np.flatnonzero((picks[i] != m["picks"]) | (_bits(pv[i]).reshape(-1, 16) != _bits(mpv).reshape(-1, 16)).any(axis=1))
        first = int(differ[0]) if len(differ) else None
        assert first is None, (f"{name}[{c}]: the first differing iteration is {first}: the device picked bin {picks[i][first]} with {pv[i][first]!r}, "
                               f"the model bin {m['picks'][first]} with {mpv[first]!r}")
        assert iters[i] == m["iterations"] and status[i] == m["status"], (name, c, iters[i], status[i], m["iterations"], m["status"])
        assert _same(Cc[i], ref.to_complex(*m["C"])), f"{name}[{c}]: C differs from the model"
        assert _same(R[i], ref.to_complex(*m["R"])), f"{name}[{c}]: R differs from the model"


@pytest.mark.parametrize("name", sorted(ref.LOOP_CASES))
def test_loop_equals_the_model_bit_for_bit(L, monkeypatch, name):
    case, D, Wn = _device_spectra(name)
    monkeypatch.delenv(KNOB, raising=False)
    out = L.clean_loop(D, Wn, gain=case["gain"], niter=case["niter"], tol=case["tol"])
    tm = L.clean_last_timing()
    assert tm["residual"] == ("lds" if case["Nf"] <= LAST_LDS else "global"), tm
    assert tm["lds_bytes"] == 1024 + (16 * case["Nf"] if case["Nf"] <= LAST_LDS else 0)
    assert tm["threads"] == min(1024, max(64, -(-(-(-case["Nf"] // 4)) // 64) * 64))
    assert tm["admissible"] == int(_model(name, 0)["admissible"].sum())
    _compare_with_model(name, out)
    print(f"{name}: iterations {list(out[4])}, status {list(out[5])}, residual {tm['residual']}, {tm['threads']} threads, loop {tm['loop_ms']:.3f} ms")
    if name == "uniform":
        assert list(out[5]) == [ref.EMPTY] and tm["admissible"] == 0
    if name == "nf3":
        assert list(out[5]) == [ref.TOL] * 3
    # the knob forces the residual into global memory: the same bits
    monkeypatch.setenv(KNOB, "global")
    forced = L.clean_loop(D, Wn, gain=case["gain"], niter=case["niter"], tol=case["tol"])
    tf = L.clean_last_timing()
    assert tf["residual"] == "global" and tf["lds_bytes"] == 1024 and tf["threads"] == tm["threads"]
    for a, b, what in zip(out, forced, ("R", "C", "picks", "pick_values", "iterations", "status")):
        assert _same(a, b), f"{name}: {what} with the residual in global memory differs from the run in LDS"


@pytest.mark.parametrize("name", ["planted", "nf255", "nf1030"])
def test_device_outputs_conserve_the_dirty_spectrum(L, name):
    case, D, Wn = _device_spectra(name)
    R, Cc, picks, pv, iters, status = L.clean_loop(D, Wn, gain=case["gain"], niter=case["niter"], tol=case["tol"])
    for c in range(case["ns"]):
        residue, mag = ref.conservation(D[c], Wn, R[c], Cc[c])
        bound = (int(iters[c]) + 2) * 4 * U * mag
        print(f"{name}[{c}]: {iters[c]} picks, max residue {float(residue.max()):.3g}, smallest bound {float(bound.min()):.3g}")
        assert np.all(residue <= bound)


@pytest.mark.parametrize("name", ["planted", "nf257", "nf1030"])
def test_restoration_against_the_long_double_gather(L, name):
    case, D, Wn = _device_spectra(name)
    R, Cc, *_ = L.clean_loop(D, Wn, gain=case["gain"], niter=case["niter"], tol=case["tol"])
    sigma = L.clean_sigma(Wn, case["df"])
    assert sigma == ref.clean_sigma(Wn, case["df"]) and sigma > 0
    S = L.clean_restore(R, Cc, case["df"], sigma)
    for c in range(case["ns"]):
        (sre, sim), mag, ncomp = ref.restore_ld(R[c], Cc[c], case["df"], sigma)
        bound = (ncomp + 2) * 4 * U * mag
        err = np.maximum(np.abs(S[c].real.astype(ref.LD) - sre), np.abs(S[c].imag.astype(ref.LD) - sim))
        print(f"{name}[{c}]: {ncomp} components, sigma {sigma:.6g}, max err {float(err.max()):.3g}, worst err / bound {float((err / bound).max()):.3g}")
        assert np.all(err <= bound)


# ---- planted spectra: ties, the stop at equality, the cut (module docstring, PLANTED) ----------------------------------------------------------
def _plan_threads(Nf):
    return min(1024, max(64, -(-(-(-Nf // 4)) // 64) * 64))


def _as_result(out, i, admissible):
    R, Cc, picks, pv, iters, status = out
    return dict(R=R[i], C=Cc[i], picks=picks[i], pick_values=pv[i], iterations=int(iters[i]), status=int(status[i]), admissible=admissible)


def _explain(got, want):
    """Where a device result leaves the expected one: the key, and for the picks the first differing iteration."""
    key = ref.same_result(got, want)
    if key is None:
        return None
    differ = np.flatnonzero((got["picks"] != want["picks"]) | (_bits(got["pick_values"]).reshape(-1, 16) != _bits(want["pick_values"]).reshape(-1, 16)).any(axis=1))
    if len(differ):
        i = int(differ[0])
        return f"{key}: first at iteration {i}: the device picked bin {got['picks'][i]} with {got['pick_values'][i]!r}, expected bin {want['picks'][i]} with {want['pick_values'][i]!r}"
    return f"{key}: {got[key]!r} against {want[key]!r}" if key in ("iterations", "status", "admissible") else key


@functools.lru_cache(maxsize=None)
def _expected(kind, Nf, gain, niter, tol):
    """Per signal (oracle or None, model or None) of a planted case; kind: "delta", "sidelobes", "cut"."""
    if kind == "cut":
        D, Wn, _ = ref.cut_case()
    else:
        D, Wn = ref.planted_spectra(Nf), (ref.delta_window(Nf) if kind == "delta" else ref.sidelobe_window(Nf))
    out = []
    for c in range(len(D)):
        oracle = ref.delta_oracle(D[c], gain, niter, tol) if kind == "delta" else None
        model = ref.model_as_complex(ref.clean_model(D[c], Wn, gain, niter, tol)) if Nf <= ref.MODEL_NF_MOST else None
        out.append((oracle, model))
    return D, Wn, out


def _run_planted(L, monkeypatch, kind, Nf, gain, niter, tol, signals=None):
    """One call of the loop on a planted case, held to the oracle and to the model byte for byte, in LDS and (Nf <= 8192) in global memory."""
    D, Wn, want = _expected(kind, Nf, gain, niter, tol)
    sel = list(range(len(D))) if signals is None else list(signals)
    monkeypatch.delenv(KNOB, raising=False)
    out = L.clean_loop(D[sel], Wn, gain=gain, niter=niter, tol=tol)
    tm = L.clean_last_timing()
    assert tm["threads"] == _plan_threads(Nf), tm
    assert tm["residual"] == ("lds" if Nf <= LAST_LDS else "global") and tm["lds_bytes"] == 1024 + (16 * Nf if Nf <= LAST_LDS else 0), tm
    print(f"{kind} Nf={Nf} gain={gain} niter={niter} tol={tol}: threads {tm['threads']} ({tm['threads'] // 64} waves), residual {tm['residual']}, "
          f"admissible {tm['admissible']}, iterations {list(out[4])}, status {list(out[5])}, loop {tm['loop_ms']:.3f} ms")
    for i, c in enumerate(sel):
        got = _as_result(out, i, tm["admissible"])
        for what, w in zip(("oracle", "model"), want[c]):
            if w is not None:
                why = _explain(got, w)
                assert why is None, f"{kind} Nf={Nf} signal {c} against the {what}: {why}"
    if Nf <= LAST_LDS:
        monkeypatch.setenv(KNOB, "global")
        forced = L.clean_loop(D[sel], Wn, gain=gain, niter=niter, tol=tol)
        tf = L.clean_last_timing()
        assert tf["residual"] == "global" and tf["lds_bytes"] == 1024 and tf["threads"] == tm["threads"]
        for a, b, what in zip(out, forced, ("R", "C", "picks", "pick_values", "iterations", "status")):
            assert _same(a, b), f"{kind} Nf={Nf}: {what} with the residual in global memory differs from the run in LDS"
        monkeypatch.delenv(KNOB)
    return out, tm


@pytest.mark.parametrize("Nf", ref.PLANTED_NF)
def test_planted_ties_go_to_the_lowest_index_at_every_wave_count(L, monkeypatch, Nf):
    """Nf = 256 w - 1: 64 w threads, w = 1 .. 16 (asserted and printed), the last stride ragged; the edges 2, 3, 65, 8192, 8193.  Four
    signals per call: all bins equal, equal P with different bits, equal P in the same lane of every wave and stride, zero."""
    out, tm = _run_planted(L, monkeypatch, "delta", Nf, 0.5, 2 * (Nf - 1) + 1, 0.0)
    assert tm["admissible"] == Nf - 1
    picks, pv = out[2], out[3]
    i = np.arange(2 * (Nf - 1) + 1)
    assert np.array_equal(picks[0], 1 + i % (Nf - 1)) and np.array_equal(picks[1], 1 + i % (Nf - 1))       # the closed form, without any reference
    assert np.all(picks[3] == 1) and not pv[3].any()
    assert list(out[4]) == [len(i)] * 4 and list(out[5]) == [ref.NITER] * 4


def test_every_wave_count_is_among_the_planted_shapes():
    assert sorted({_plan_threads(Nf) for Nf in ref.PLANTED_NF}) == [64 * w for w in range(1, 17)]


@pytest.mark.parametrize("Nf", [2, 257, 1030, 8193])
def test_the_stop_meets_equality(L, monkeypatch, Nf):
    """All bins 5 on the delta window, tol = 2^-3: the threshold 25 / 64 is met exactly after three picks of every bin (gain 1/2) or
    by the zeros one pick of every bin leaves (gain 1).  tol = 0 goes on: bin 1 with value 0."""
    K = Nf - 1
    out, _ = _run_planted(L, monkeypatch, "delta", Nf, 0.5, 3 * K + 7, 2.0 ** -3, signals=[0])
    assert (int(out[4][0]), int(out[5][0])) == (3 * K, ref.TOL) and np.all(out[2][0][3 * K:] == -1)
    out, _ = _run_planted(L, monkeypatch, "delta", Nf, 1.0, 3 * K + 7, 2.0 ** -3, signals=[0])
    assert (int(out[4][0]), int(out[5][0])) == (K, ref.TOL) and not out[0][0][1:].any()
    out, _ = _run_planted(L, monkeypatch, "delta", Nf, 1.0, Nf + 5, 0.0, signals=[0])
    assert (int(out[4][0]), int(out[5][0])) == (Nf + 5, ref.NITER) and np.all(out[2][0][K:] == 1) and not out[3][0][K:].any()


def test_peaks_that_overflow_tie_at_infinity(L, monkeypatch):
    """D_k = 1e200: every P is +inf and stays so through 20 halvings; +inf == +inf is a tie, bin 1 wins it 20 times and no NaN arises."""
    monkeypatch.delenv(KNOB, raising=False)
    D, Wn = np.full((1, 8), complex(1e200, 0.0)), ref.delta_window(8)
    out = L.clean_loop(D, Wn, gain=0.5, niter=20, tol=0.0)
    tm = L.clean_last_timing()
    for want in (ref.delta_oracle(D[0], 0.5, 20, 0.0), ref.model_as_complex(ref.clean_model(D[0], Wn, 0.5, 20, 0.0))):
        assert _explain(_as_result(out, 0, tm["admissible"]), want) is None, _explain(_as_result(out, 0, tm["admissible"]), want)
    assert np.all(out[2][0] == 1) and np.all(np.isfinite(out[0].view(np.float64))) and np.all(np.isfinite(out[3].view(np.float64)))


@pytest.mark.parametrize("Nf", [257, 1030])
def test_sidelobes_after_a_tie_of_every_bin(L, monkeypatch, Nf):
    """Wn_0 = 1 with dyadic sidelobes at 1, 2 and 5: iteration 0 is a tie of every admissible bin, and every later search runs on what
    the update pass left.  Against the model."""
    out, tm = _run_planted(L, monkeypatch, "sidelobes", Nf, 0.5, 300, 0.0, signals=[0, 1])
    assert tm["admissible"] == Nf - 1 and out[2][0][0] == 1 and out[2][1][0] == 1 and list(out[4]) == [300, 300]


def test_the_cut_admits_equality_and_nothing_below(L, monkeypatch):
    """Wn_2p at den == 2^-20 exactly, one double above and one below (found by search: tests/_clean_ref.py cut_doubles), each in three
    waves.  The bins below the cut hold the largest |D| and are never picked; the count and every byte are the model's."""
    D, Wn, found = ref.cut_case()
    out, tm = _run_planted(L, monkeypatch, "cut", ref.CUT_NF, 0.5, 60, 0.0)
    assert tm["admissible"] == ref.CUT_NF - 1 - len(ref.CUT_BINS["below"])
    for c in range(2):
        assert not set(ref.CUT_BINS["below"]) & set(out[2][c].tolist())
        assert out[2][c][0] == ref.CUT_BINS["above"][2] and out[2][c][1] == ref.CUT_BINS["at"][2]
    if not found:
        from _guards import precondition_not_met
        precondition_not_met("no double gives den == 2^-20 exactly: the leg AT the cut ran on the double just above it")


# ---- restoration on planted components --------------------------------------------------------------------------------------------------------
def _restore_cases(Nf=1030):
    """name -> (C [4][Nf], the number of components of every signal).  R: Gaussian integers; df = 1/64, sigma = 3 df."""
    rng = np.random.default_rng(41)
    z = lambda *shape: rng.integers(1, 5, shape) * rng.choice([-1.0, 1.0], shape) + 1j * (rng.integers(1, 5, shape) * rng.choice([-1.0, 1.0], shape))     # noqa: E731
    every, none = z(4, Nf), np.zeros((4, Nf), dtype=np.complex128)
    few = np.zeros((4, Nf), dtype=np.complex128)
    at = [0, 255, 256, 511, 512, Nf - 1]                                       # the first and last lane of the chunks of 256, the ragged last chunk
    few[:, at] = z(4, len(at))
    signs = np.zeros((4, Nf), dtype=np.complex128)
    imag = np.arange(3, Nf, 7)                                                 # re = +0.0 or -0.0, im != 0: components
    signs[:, imag] = 1j * z(4, len(imag)).imag
    signs.real[:, imag[::2]] = -0.0
    zeros = np.setdiff1d(np.arange(Nf), imag)                                  # +-0.0 in both parts: -0.0 != 0.0 is false -- no components
    signs.real[:, zeros[::2]] = -0.0
    signs.imag[:, zeros[::3]] = -0.0
    assert np.signbit(signs.real[:, zeros[::2]]).all() and np.signbit(signs.imag[:, zeros[::3]]).all()
    return {"every": (every, Nf), "none": (none, 0), "few": (few, len(at)), "signs": (signs, len(imag))}, z(4, Nf)


@pytest.mark.parametrize("name", ["every", "none", "few", "signs"])
def test_restoration_of_planted_components(L, name):
    """The ordered compaction (ballots over chunks of 256) at its edges: every bin a component, none, components at the ends of the
    chunks only, and parts that are zero, negative zero or imaginary alone."""
    cases, R = _restore_cases()
    Cc, planted = cases[name]
    df, sigma = 2.0 ** -6, 3 * 2.0 ** -6
    S = L.clean_restore(R, Cc, df, sigma)
    if name == "none":
        assert _same(S, R)
    for c in range(4):
        (sre, sim), mag, ncomp = ref.restore_ld(R[c], Cc[c], df, sigma)
        assert ncomp == planted
        bound = (ncomp + 2) * 4 * U * mag
        err = np.maximum(np.abs(S[c].real.astype(ref.LD) - sre), np.abs(S[c].imag.astype(ref.LD) - sim))
        print(f"{name}[{c}]: {ncomp} components, max err {float(err.max()):.3g}, worst err / bound {float((err / bound).max()):.3g}")
        assert np.all(err <= bound)


# ---- clean: the three stages in one call -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["planted", "nf1030", "nf8193", "nf257-zero"])
def test_clean_equals_the_three_stages(L, name):
    case = ref.loop_case(name)
    kw = dict(df=case["df"], Nf=case["Nf"], W=case["W"])
    r = L.clean(case["y"], case["t"], gain=case["gain"], niter=case["niter"], tol=case["tol"], center_time=False, **kw)
    tm = L.clean_last_timing()
    assert tm["residual"] == ("lds" if case["Nf"] <= LAST_LDS else "global") and tm["sigma"] == r.sigma
    D, Wn = L.dirty_spectrum(case["y"], case["t"], **kw)
    R, Cc, picks, pv, iters, status = L.clean_loop(D, Wn, gain=case["gain"], niter=case["niter"], tol=case["tol"])
    sigma = L.clean_sigma(Wn, case["df"])
    S = L.clean_restore(R, Cc, case["df"], sigma)
    assert r.sigma == sigma
    assert _same(r.window, Wn) and _same(r.picks, picks) and _same(r.pick_values, pv)
    for got, want, what in ((r.dirty, D, "dirty"), (r.residual, R, "residual"), (r.components, Cc, "components"), (r.spectrum, S, "spectrum")):
        assert _same(got, want.T), what
    assert list(np.atleast_1d(r.iterations)) == list(iters)
    assert list(r.status) == [{0: "niter", 1: "tol", 2: "empty"}[int(v)] for v in status]
    assert _same(r.power, (S.real ** 2 + S.imag ** 2).T) and _same(r.amplitude, 2.0 * np.abs(Cc).T)
    assert np.array_equal(r.freq, np.arange(case["Nf"]) * case["df"])


def test_clean_of_one_signal_and_the_planted_lines(L):
    """A vector in, vectors out; the planted amplitudes and phases (tests/test_clean_ref_host.py holds the model to the same figures);
    center_time moves the epoch of the phases to the mean time."""
    t, y, df, Nf = ref.planted_record(0)
    r = L.clean(y, t, df=df, Nf=Nf, niter=300, tol=1e-6, center_time=False)
    assert r.dirty.shape == (Nf,) and r.window.shape == (2 * Nf - 1,) and r.picks.shape == (300,) and isinstance(r.iterations, int) and isinstance(r.status, str)
    assert abs(r.amplitude[40] - 1.0) <= 0.003 and abs(r.amplitude[93] - 0.6) <= 0.001
    assert abs(np.angle(r.components[40]) - 0.7) <= 1e-3 and abs(np.angle(r.components[93]) + 1.1) <= 1e-3
    assert np.delete(r.amplitude, [40, 93]).max() <= 0.05
    assert np.argmax(r.power) == 40
    rc = L.clean(y, t, df=df, Nf=Nf, niter=300, tol=1e-6)                   # center_time=True
    shift = 2 * np.pi * (40 * df) * np.mean(t)
    assert abs(np.angle(rc.components[40] * np.exp(-1j * (0.7 + shift)))) <= 1e-3 and abs(rc.amplitude[40] - 1.0) <= 0.003


# ---- reproducibility ------------------------------------------------------------------------------------------------------------------------
def test_two_calls_and_a_signal_alone_give_the_same_bits(L):
    case = ref.loop_case("nf1030")
    kw = dict(df=case["df"], Nf=case["Nf"], W=case["W"], gain=case["gain"], niter=case["niter"], tol=case["tol"], center_time=False)
    a = L.clean(case["y"], case["t"], **kw)
    b = L.clean(case["y"], case["t"], **kw)
    one = L.clean(case["y"][:, 1], case["t"], **kw)
    for key in ("dirty", "window", "residual", "components", "picks", "pick_values", "spectrum", "power", "amplitude"):
        assert _same(getattr(a, key), getattr(b, key)), key
        if key == "window":
            assert _same(one.window, a.window)
        elif key in ("picks", "pick_values"):
            assert _same(getattr(one, key), getattr(a, key)[1]), key
        else:
            assert _same(getattr(one, key), getattr(a, key)[:, 1]), key
    assert list(a.iterations) == list(b.iterations) and a.status == b.status and a.sigma == b.sigma == one.sigma
    assert one.iterations == a.iterations[1] and one.status == a.status[1]


# ---- device-pointer outputs -------------------------------------------------------------------------------------------------------------------
def test_device_pointer_outputs_equal_host_outputs(L):
    import torch
    from lpvspectral_jl_amd._lib import check, lib, out_ptr
    case = ref.loop_case("nf257-one")
    t, y, W, df, Nf, ns, niter = case["t"], np.asfortranarray(case["y"]), case["W"], case["df"], case["Nf"], case["ns"], 5
    D, Wn = L.dirty_spectrum(y, t, df=df, Nf=Nf, W=W)
    R, Cc, picks, pv, iters, status = L.clean_loop(D, Wn, gain=0.5, niter=niter)
    sigma = L.clean_sigma(Wn, df)
    S = L.clean_restore(R, Cc, df, sigma)
    dev = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device="cuda")     # noqa: E731
    ptr = lambda x: C.c_void_p(x.data_ptr())                                                     # noqa: E731
    dD, dWn, dR, dC, dpv, dS = dev(ns, Nf, 2), dev(2 * Nf - 1, 2), dev(ns, Nf, 2), dev(ns, Nf, 2), dev(ns, niter, 2), dev(ns, Nf, 2)
    torch.cuda.synchronize()
    check(lib().lpvs_dirty_spectrum_f64(out_ptr(y), ns, out_ptr(t), len(t), out_ptr(W), df, Nf, 1, 0, 0, ptr(dD), ptr(dWn)))
    hp, hi, hs = np.zeros((ns, niter), dtype=np.int32), np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    check(lib().lpvs_clean_loop_f64(ptr(dD), ns, Nf, ptr(dWn), 0.5, niter, 0.0, 0, ptr(dR), ptr(dC), out_ptr(hp), ptr(dpv), out_ptr(hi), out_ptr(hs)))
    check(lib().lpvs_clean_restore_f64(ptr(dR), ptr(dC), ns, Nf, df, sigma, 0, ptr(dS)))
    torch.cuda.synchronize()
    host = lambda x: torch.view_as_complex(x).cpu().numpy()                                      # noqa: E731
    for got, want, what in ((dD, D, "D"), (dWn, Wn, "Wn"), (dR, R, "R"), (dC, Cc, "C"), (dpv, pv, "pick values"), (dS, S, "S")):
        assert _same(host(got), want), what
    assert _same(hp, picks) and _same(hi, iters) and _same(hs, status)
    # complex128 device tensors through the Python layer
    R2, C2, p2, *_ = L.clean_loop(torch.view_as_complex(dD), torch.view_as_complex(dWn), gain=0.5, niter=niter)
    assert _same(R2, R) and _same(C2, Cc) and _same(p2, picks)


# ---- what a reused device block held ------------------------------------------------------------------------------------------------------------
def test_no_result_depends_on_what_a_reused_block_held(L, monkeypatch):
    from test_gpu_pool_fill import same_bytes_whatever_the_block_held
    case = ref.loop_case("nf257-one")

    def run(L, monkeypatch):
        r = L.clean(case["y"], case["t"], df=case["df"], Nf=case["Nf"], W=case["W"], gain=0.5, niter=40, tol=0.0)
        tm = L.clean_last_timing()
        assert tm["residual"] == "lds" and tm["path"] in ("direct", "nufft")
        return r, tm
    same_bytes_whatever_the_block_held(run, L, monkeypatch)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_their_messages_and_status_codes(L):
    """ValueError is LPVS_EARGUMENT and NotImplementedError LPVS_EUNSUPPORTED (lpvspectral.jl_amd/_lib.py: check)."""
    t, y, W = ref.exact_record(3, 300, 1)
    y = y[:, 0]
    D, Wn = L.dirty_spectrum(y, t, df=2.0 ** -6, Nf=64, W=W)
    for entry, who in ((L.dirty_spectrum, "dirty_spectrum"), (L.clean, "clean")):
        kw = dict(df=2.0 ** -6, Nf=64)
        bad = y.copy(); bad[17] = np.inf
        with pytest.raises(ValueError, match=rf"{who}: t, y or W holds a value that is not finite"):
            entry(bad, t, **kw)
        neg = W.copy(); neg[5] = -1.0
        with pytest.raises(ValueError, match=rf"{who}: a weight is negative"):
            entry(y, t, W=neg, **kw)
        with pytest.raises(ValueError, match=rf"{who}: the weights sum to 0"):
            entry(y, t, W=np.zeros(len(t)), **kw)
        for df, text in ((0.0, "0.000000"), (-0.5, "-0.500000"), (np.inf, "inf"), (np.nan, "nan")):
            with pytest.raises(ValueError, match=rf"{who}: df must be positive and finite, got {text}"):
                entry(y, t, df=df, Nf=64)
        with pytest.raises(ValueError, match=r"y has 300 samples, t has 299"):
            entry(y, t[:-1], **kw)
    with pytest.raises(ValueError, match=r"dirty_spectrum: Nf must be at least 2, got 1"):
        L.dirty_spectrum(y, t, df=2.0 ** -6, Nf=1)
    with pytest.raises(NotImplementedError, match=r"dirty_spectrum: 1048577 frequencies are more than 2\^20"):
        L.dirty_spectrum(y, t, df=2.0 ** -6, Nf=(1 << 20) + 1)
    with pytest.raises(ValueError, match=r"path: unknown value 'fft'"):
        L.dirty_spectrum(y, t, df=2.0 ** -6, Nf=64, path="fft")
    # a NaN in D or in Wn: the family's flag word
    for which in (0, 1):
        Db, Wb = D.copy(), Wn.copy()
        (Db if which == 0 else Wb)[3] = complex(0.0, np.nan)
        with pytest.raises(ValueError, match=r"clean: D or Wn holds a value that is not finite"):
            L.clean_loop(Db, Wb)
    # every refusal of the plan (csrc/clean_plan.h; tests/test_clean_plan.py holds the same messages on the host)
    plan_refusals = [
        (dict(niter=-1), ValueError, r"clean: niter must not be negative, got -1"),
        (dict(niter=(1 << 24) + 1), NotImplementedError, r"clean: 16777217 iterations are more than 2\^24"),
        (dict(gain=0.0), ValueError, r"clean: gain must lie in \(0, 2\), got 0.000000"),
        (dict(gain=2.0), ValueError, r"clean: gain must lie in \(0, 2\), got 2.000000"),
        (dict(gain=np.nan), ValueError, r"clean: gain must lie in \(0, 2\), got nan"),
        (dict(tol=-0.25), ValueError, r"clean: tol must lie in \[0, 1\), got -0.250000"),
        (dict(tol=1.0), ValueError, r"clean: tol must lie in \[0, 1\), got 1.000000"),
    ]
    for kw, exc, msg in plan_refusals:
        with pytest.raises(exc, match=msg):
            L.clean_loop(D, Wn, **kw)
        with pytest.raises(exc, match=msg):
            L.clean(y, t, df=2.0 ** -6, Nf=64, **kw)
    with pytest.raises(ValueError, match=r"clean: Nf must be at least 2, got 1"):
        L.clean_loop(D[:1], Wn[:1])
    with pytest.raises(ValueError, match=r"clean: Nf must be at least 2, got 1"):
        L.clean(y, t, df=2.0 ** -6, Nf=1)
    with pytest.raises(NotImplementedError, match=r"clean: 1048577 frequencies are more than 2\^20"):
        L.clean(y, t, df=2.0 ** -6, Nf=(1 << 20) + 1, niter=1)
    with pytest.raises(ValueError, match=r"clean_restore: sigma must be positive and finite, got 0"):
        L.clean_restore(D, D, 2.0 ** -6, 0.0)
    with pytest.raises(ValueError, match=r"clean_restore: df must be positive and finite, got 0.000000"):
        L.clean_restore(D, D, 0.0, 1.0)
    with pytest.raises(ValueError, match=r"Wn: shape \(126,\), needed \(127,\)"):
        L.clean_loop(D, Wn[:-1])
