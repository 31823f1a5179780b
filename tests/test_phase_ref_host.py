"""tests/_phase_ref.py held to what does not depend on it, and the proof that the GPU cases built on it put weight on the low words of the
device's phases; CPU only.

    a  exact_turns_angular against fractions.Fraction with a 100-digit pi, |w x| near 1e3, 3e6, 2^30 and 2^40 rad, both signs: 1e-18 turns
    b  the exact-phase Gram / evaluation references against oracle.gram_phase_ld and _eval_ref.evaluate_ld at the existing small-phase
       cases, to what the latter's own errors allow; their disagreement at 3e6 rad is printed (it is why the new references exist);
       the fast Gram product (gram_of) against the plain long-double product
    c  THE MUTATION TABLE.  For every GPU case that uses these references, or the inexact-product inputs of tests/_lomb_ref.py, the numpy
       restatement of the phase formation its kernels use -- lomb_sincos; nu_phase_turns; the p + d form of nudft.hip -- is run on the
       case's own inputs: faithful, and with one low word dropped or negated.  What is measured is the largest error of one term's
       trigonometry against the phase of the real product (for a transform: of its highest mode), not the summation.  The faithful
       restatement has to stay within the case's per-term bound -- 1e-12 + q for the structured forms and predict, 6 u for the Lomb
       direct sums, 1e-12 + (residual phase)^2 / 2 for the Lomb transforms -- and every mutation has to exceed it at least ten times.
       A low word that is identically zero on a case's inputs (the low words of the step on the dyadic grid, where the issue's point is
       eps = 0 exactly; of the rotation's a, a double) cannot matter there: the table says "zero", and every word is required to reach
       its factor of ten in at least one case of its family.

Mutation factors measured here on the CPU (error of the mutated restatement / bound, "drop"; "negate" is twice that; the GPU ratios of the
same cases are in DESIGN.md 4.3.1, 4.12 and 4.11):

    lomb_sincos, e             direct sums 2.2e6 (lattice and full-mantissa times; nterms, spectrogram, bootstrap and wwz alike: f t = 3e6 turns
                               against 6 u); the transforms' pre-phase 1.8e2 (base 37.25 D) .. 1.5e3 (bases of the blocks of 64)
    nu_phase_turns, tl         Gram 3e6 rad: 7.3e2 (24 x 3), 8.9e2 (20 x 8), residual cases 4.0e2 .. 7.2e2; 2^30 rad: 2.0e5; windows 6.0e4;
                               predict 2.6e2 .. 2.7e2 (3e6 rad), 8.5e4 (2^30 rad); predict's rotation 29 and 3.7e3; Lomb transforms 5.9e2 .. 4.8e3
    nu_phase_turns, D_lo       Gram 3e6 rad: 3.4e2 (24 x 3), 2.2e2 (20 x 8), residual cases 42 .. 3.3e2; windows 2.7e4; predict 1.1e2;
                               Lomb transforms 1.4e2 .. 2.0e3; zero on the dyadic grids
    nudft, FMA error of wh x   Gram 3e6 rad: 5.1e2 .. 5.5e2; 2^30 rad: 1.4e5; Fourier 4e7 rad: 7.9e3; windows 3.4e4
    nudft, wl                  Gram 3e6 rad: 2.2e2 .. 4.6e2; Fourier 3.7e3 .. 6.1e3; windows 2.6e4; zero on the dyadic grid
    nudft, d (the correction)  Gram 3e6 rad: 7.0e2 .. 9.3e2; 2^30 rad: 1.4e5; Fourier 1.1e4 .. 1.4e4; windows 5.8e4
The faithful restatements sit at 7e-7 .. 0.1 of their bounds (nudft 7e-7 .. 7e-3, nu_phase_turns 0.012 .. 0.10, the rounding of its turns
times the highest mode) and lomb_sincos at 0.26 of 6 u (the rounding of r).  All of these are CPU figures."""
from fractions import Fraction

import numpy as np
import pytest

import _eval_ref as E
import _gram_ref as R
import _lomb_ref as LR
import _phase_ref as PR

LD = PR.LD
U = 2.0 ** -53
TWO_PI = PR.TWO_PI_LD


# ---- a ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mag", [1e3, 3e6, 2.0 ** 30, 2.0 ** 40, 1.3e14], ids=["1e3", "3e6", "2^30", "2^40", "1.3e14"])
def test_exact_turns_against_rational_arithmetic(mag):
    rng = np.random.default_rng(int(np.log2(mag)))
    w = rng.uniform(0.5, 6.3, 12)
    x = rng.uniform(0.5, 1.0, 25) * (mag / w.max()) * rng.choice([-1.0, 1.0], 25)     # 300 pairs, both signs
    u = PR.exact_turns_angular(w, x)
    assert u.dtype == LD and u.shape == (12, 25) and np.all(np.abs(u) <= 0.5) and np.abs(w[:, None] * x[None, :]).max() > 0.5 * mag
    worst = Fraction(0)
    for i in range(12):
        for j in range(25):
            hi = float(u[i, j])
            d = Fraction(hi) + Fraction(float(u[i, j] - LD(hi))) - PR.turns_fraction(w[i], x[j])
            worst = max(worst, abs(d - round(d)))
    print(f"|w x| ~ {mag:.3g} rad: worst |exact_turns_angular - rational| = {float(worst):.2e} turns")
    assert worst <= Fraction(1, 10 ** 18)


def test_the_chunks_of_one_over_two_pi():
    c = PR.INV_TWO_PI_CHUNKS
    assert len(c) == 6 and all(v * 2.0 ** (24 * (i + 1)) == int(v * 2.0 ** (24 * (i + 1))) < 2 ** 24 for i, v in enumerate(c))   # 24-bit integers
    assert abs(sum(Fraction(v) for v in c) - 1 / (2 * PR.PI_Q)) < Fraction(1, 2 ** 144)
    assert abs(Fraction(float(TWO_PI)) + Fraction(float(TWO_PI - LD(float(TWO_PI)))) - 2 * PR.PI_Q) < Fraction(1, 2 ** 61)


# ---- b ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.STRUCT_LPV_CASES, ids=[c[0] for c in R.STRUCT_LPV_CASES])
def test_lpv_gram_reference_agrees_with_the_oracle_at_small_phases(oracle, case):
    """oracle.gram_phase_ld rounds w x to a long double (2^-64 |w x| of phase, twice per product of two columns), sums N products in long
    double (2^-64 each) and rounds the entry to a double: (2^-63 max|w x| + (N + 16) 2^-64 + 2^-53) C is what it can be off by."""
    _, Nf, Nv, N = case
    y, X, V, w = R.struct_lpv_inputs(case)
    K = oracle.basis_activation(V, Nv)
    G, b, C, s = PR.lpv_gram_exact(X, w, K, y)
    Go = oracle.gram_phase_ld(X, w, K)
    j = np.arange(2 * Nf * Nv) % Nv
    allow = (2.0 ** -63 * np.abs(w).max() * np.abs(X).max() + (N + 16) * 2.0 ** -64 + U) * C[np.ix_(j, j)]
    r = float((np.abs(G - Go.astype(LD)) / allow).max())
    print(f"{case[0]}: exact-phase Gram against oracle.gram_phase_ld, worst ratio to the oracle's own error {r:.3f}")
    assert r <= 1.0
    Phi = oracle.lpv_regressor(X, V, w, Nv)                                        # b: against the f64 regressor (its phase is rounded: u |w x|)
    allow_b = (U * np.abs(w).max() * np.abs(X).max() + 4 * U) * s[j]
    assert np.all(np.abs(b - Phi.astype(LD).T @ y.astype(LD)) <= allow_b)


@pytest.mark.parametrize("case", R.STRUCT_FOURIER_CASES, ids=[c[0] for c in R.STRUCT_FOURIER_CASES])
def test_fourier_gram_reference_agrees_with_the_oracle_at_small_phases(oracle, case):
    _, Nf, zero, weighted, N = case
    y, t, f, W = R.struct_fourier_inputs(case)
    w = 6.283185307179586 * f
    G, b, sG, sb = PR.fourier_gram_exact(t, w, y, zero, W)
    Go = oracle.gram_phase_ld(t, w, None, zero, W)
    allow = (2.0 ** -63 * w.max() * t.max() + (N + 16) * 2.0 ** -64 + U) * sG
    r = float(np.abs(G - Go.astype(LD)).max() / allow)
    print(f"{case[0]}: exact-phase Gram against oracle.gram_phase_ld, worst ratio to the oracle's own error {r:.3f}")
    assert G.shape == Go.shape and r <= 1.0
    A, zf = oracle.get_fourier_regressor(t, f)
    Wy = (np.ones(N) if W is None else W).astype(LD) * y.astype(LD)
    assert bool(zf) == zero and np.all(np.abs(b - A.astype(LD).T @ Wy) <= (U * w.max() * t.max() + 4 * U) * sb)


def test_the_oracles_long_double_product_cannot_referee_large_phases(oracle):
    """On record: at the benchmark's scale (3e6 rad) oracle.gram_phase_ld is off by more than the new cases' whole bound."""
    case = R.PHASE_LPV["bench-24x3"]
    Y, X, V, w = R.phase_lpv_inputs(case)
    K = oracle.basis_activation(V, case[2])
    G, _, C, _ = PR.lpv_gram_exact(X, w, K)
    j = np.arange(G.shape[0]) % case[2]
    r = float((np.abs(G - oracle.gram_phase_ld(X, w, K).astype(LD)) / (1e-12 * C[np.ix_(j, j)])).max())
    lo = float(np.abs(PR.exact_turns_angular(w[-1:], X[:2]) - PR._wrap(w[-1].astype(LD) * X[:2].astype(LD) / TWO_PI)).max())
    print(f"bench-24x3 (|w x| = 3.1e6 rad): |exact-phase Gram - oracle.gram_phase_ld| is {r:.4f} of 1e-12 C; one long-double product is off by {lo:.1e} turns")
    assert 1e-4 <= r <= 0.5                                                       # (2^-63 |w x| = 3.4e-13: visible, and itself no referee)


def test_fast_gram_product_against_the_plain_long_double_product(oracle):
    case = R.PHASE_LPV["bench-24x3-multi"]
    Y, X, V, w = R.phase_lpv_inputs(case)
    K = oracle.basis_activation(V, case[2])
    G, b, C, s = PR.lpv_gram_exact(X, w, K, Y)
    Gp, bp, _, _ = PR.lpv_gram_exact(X, w, K, Y, plain=True)
    j = np.arange(G.shape[0]) % case[2]
    assert b.shape == bp.shape == (G.shape[0], 3)
    assert np.all(np.abs(G - Gp) <= 2.0 ** -52 * C[np.ix_(j, j)]) and np.all(np.abs(b - bp) <= 2.0 ** -52 * s[j])
    y, t, f, W = R.phase_fourier_inputs(R.STRUCT_FOURIER_CASES[3])                # zero frequency and weights
    G, b, sG, sb = PR.fourier_gram_exact(t, 6.283185307179586 * f, y, True, W)
    Gp, bp, _, _ = PR.fourier_gram_exact(t, 6.283185307179586 * f, y, True, W, plain=True)
    assert G.shape == (79, 79) and np.abs(G - Gp).max() <= 2.0 ** -52 * sG and np.abs(b - bp).max() <= 2.0 ** -52 * sb


def test_evaluation_reference_agrees_with_the_rounded_phase_reference_at_small_phases():
    """_eval_ref.evaluate_ld rounds the phase to a double: u |w x| per term, nothing else differs."""
    rng = np.random.default_rng(5)
    Nf, nb, M = 24, 3, 500
    w, x = 2 * np.pi * np.arange(1, Nf + 1) / 7.0, rng.uniform(-50.0, 50.0, M)
    P = rng.standard_normal((Nf * nb, 2)) + 1j * rng.standard_normal((Nf * nb, 2))
    K = np.abs(rng.standard_normal((M, nb))).astype(LD)
    yh, S = PR.evaluate_exact(P, w, x, K, 0.25)
    yo, So = E.evaluate_ld(P, w, x, K, 0.25)
    assert np.array_equal(S, So) and np.all(np.abs(yh - yo) <= (U * np.abs(w).max() * np.abs(x).max() + 2.0 ** -60) * S)


# ---- c ------------------------------------------------------------------------------------------------------------------------------------
def _trig_err(turns, exact_turns):
    """Largest |e^{i phase} - e^{i exact phase}| = 2 |sin(pi (turns - exact))| over the array (long double)."""
    return float(np.abs(2 * np.sin(TWO_PI / 2 * PR._wrap(turns.astype(LD) - exact_turns))).max())


def _lomb_rows(name, f, t, bound):
    exact = PR.lomb_turns_exact(f, t)
    return [(name, "lomb_sincos", "e", bound, _trig_err(PR.lomb_turns(f, t), exact),
             {m: _trig_err(PR.lomb_turns(f, t, "e:" + m), exact) for m in ("drop", "neg")}, False)]


def _nu_rows(name, what, D_hi, D_lo, x, modes, bound, words=("tl", "D_lo")):
    """nu_phase_turns of (D_hi + D_lo) x; the error of mode ``modes`` is that many times the error of the turns."""
    exact = PR.dd_turns_exact([D_hi], [D_lo], x)[0]
    def err(mut):
        return float(np.abs(2 * np.sin(TWO_PI / 2 * modes * PR._wrap(PR.nu_turns(D_hi, D_lo, x, mut).astype(LD) - exact))).max())
    zero = {"tl": False, "D_lo": D_lo == 0.0}
    return [(name, what, wd, bound, err(None), {m: err(f"{wd}:{m}") for m in ("drop", "neg")}, zero[wd]) for wd in words]


def _nudft_rows(name, tb, x, bound):
    """Slot 8 a + b of nudft.hip: the product of the anchor's and the offset's corrected sincos against e^{i (om_anchor + om_step) x}."""
    (ah, al), (sh, sl) = (v[::8] for v in tb["om"]), tb["step"]
    exact = PR.dd_turns_exact(ah, al, x)[:, None, :] + PR.dd_turns_exact(sh, sl, x)[None, :, :]
    ze = np.cos(TWO_PI * exact) + 1j * np.sin(TWO_PI * exact)
    def err(mut):
        ca, sa = PR.nudft_trig(ah, al, x, mut)
        cb, sb = PR.nudft_trig(sh, sl, x, mut)
        z = (ca + 1j * sa)[:, None, :] * (cb + 1j * sb)[None, :, :]
        return float(np.abs(z - ze).max())
    base = err(None)
    zero = {"fe": False, "wl": not (np.any(al) or np.any(sl)), "d": False}
    return [(name, "nudft", wd, bound, base, {m: err(f"{wd}:{m}") for m in ("drop", "neg")}, zero[wd]) for wd in ("fe", "wl", "d")]


def _gram_rows(name, w, x, nufft=True, nudft=True):
    xmax = float(np.abs(x).max())
    bound = float(1e-12 + PR.second_order(w, x))
    tb = PR.ap_slot_tables(w, xmax)
    rows = _nudft_rows(name, tb, x, bound) if nudft else []
    if nufft:
        rows += _nu_rows(name, "nu_phase_turns", tb["step"][0][1], tb["step"][1][1], x, len(tb["om"][0]) - 1, bound)
    return rows


def _all_rows():
    import test_gpu_lomb as TL
    import test_gpu_lomb_bootstrap as TB
    import test_gpu_lomb_terms as TT
    import test_gpu_lomb_windows as TW
    import test_gpu_wwz as TZ
    rows = []
    # the structured Gram, LPV and Fourier, the window engine
    for case in R.PHASE_LPV_CASES:
        Y, X, V, w = R.phase_lpv_inputs(case)
        rows += _gram_rows("gram " + case[0], w, X, nufft=case[0] != "resid-split")
    for case in R.STRUCT_FOURIER_CASES:
        y, t, f, W = R.phase_fourier_inputs(case)
        rows += _gram_rows("gram " + case[0], 6.283185307179586 * f, t, nufft=False)
    n, nwin, Nf, t, f, Y = R.phase_window_inputs()
    rows += _gram_rows("windows", 6.283185307179586 * f, t)
    # predict, type-2: modes 0 .. Nf - 1 of the step, and the rotation by the first frequency (a double: no low word of its own)
    for cid in (c[0] for c in R.PHASE_PREDICT_CASES):
        Y, X, V, w = R.phase_lpv_inputs(R.PHASE_LPV[cid])
        bound = float(1e-12 + PR.second_order(w, X))
        tb = PR.ap_slot_tables(w, float(np.abs(X).max()))
        rows += _nu_rows(cid, "nu_phase_turns", tb["step"][0][1], tb["step"][1][1], X, len(w) - 1, bound)
        rows += _nu_rows(cid, "rotation", w[0], 0.0, X, 1, bound, words=("tl",))
    # the Lomb-Scargle family: direct sums, 6 u per term
    for rec in ("lattice", "full"):
        rows += _lomb_rows("lomb direct " + rec, TL._wide("wide-irregular", 65), TL._record(4097, 3, rec=rec)[0], 6 * U)
        t, y, W, f = TT._late(rec)
        rows += _lomb_rows("lomb nterms " + rec, f, t, 6 * U)
        rows += _lomb_rows("lomb bootstrap " + rec, TB._f(rec), TB._record(TB.N_LONG, rec=rec)[0], 6 * U)
    rows += _lomb_rows("lomb spectrogram late", TW._freqs(late=True), TW._record(late=True)[0], 6 * U)
    rows += _lomb_rows("wwz late", TZ._freqs("late"), TZ._record(TZ.CASES["late"][0], 0.0, TZ.CASES["late"][3])[0], 6 * U)
    # the Lomb transforms: the pre-phase of the blocks' bases (lomb_sincos) and the coordinates of the step 2 pi D (family 2: 4 pi D)
    t = TL._record(4097, 3, rec="lattice")[0]
    for kind in ("wide-zero", "wide-offset"):
        for block in (None, 64):
            f = TL._wide(kind)
            L = len(f) if block is None else block
            name = f"lomb transform {kind} block {L}"
            ph = LR.block_residual_phase(f, t, block)
            bases = f[::L][f[::L] != 0.0]
            if len(bases):
                rows += _lomb_rows(name, bases, t, 1e-12 + 0.5 * ph ** 2)
            D = (Fraction(float(f[-1])) - Fraction(float(f[0]))) / (len(f) - 1)
            for fam in (1, 2):
                hi, lo = PR._dd(2 * PR.PI_Q * D * fam)
                rows += _nu_rows(name + f" family {fam}", "nu_phase_turns", hi, lo, t, L - 1, 1e-12 + 0.5 * (fam * ph) ** 2)
    return rows


def test_mutation_table():
    rows = _all_rows()
    reached = {}
    print()
    print(f"{'case':46s} {'formation':15s} {'word':5s} {'bound':>9s} {'faithful':>9s} {'drop':>9s} {'negate':>9s}")
    failures = []
    for name, what, word, bound, faithful, mutated, zero in rows:
        fd, fn = mutated["drop"] / bound, mutated["neg"] / bound
        tag = "  zero" if zero else ""
        print(f"{name:46s} {what:15s} {word:5s} {bound:9.2e} {faithful / bound:9.2e} {fd:9.2e} {fn:9.2e}{tag}")
        if faithful > bound:
            failures.append((name, what, word, "faithful", faithful / bound))
        if zero:
            assert mutated["drop"] == faithful and mutated["neg"] == faithful, (name, word)      # the word is identically zero here
            continue
        reached[(what, word)] = max(reached.get((what, word), 0.0), min(fd, fn))
        if min(fd, fn) < 10.0:
            failures.append((name, what, word, "mutation", min(fd, fn)))
    assert not failures, failures
    assert set(reached) == {("lomb_sincos", "e"), ("nu_phase_turns", "tl"), ("nu_phase_turns", "D_lo"), ("rotation", "tl"), ("nudft", "fe"), ("nudft", "wl"),
                            ("nudft", "d")} and all(v >= 10.0 for v in reached.values()), reached
