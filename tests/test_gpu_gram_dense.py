"""Every instance of the dense Gram kernel (csrc/gram.hip: gram_kernel<MODE, BK>, MODE = KR / KRS / PANEL, BK = 32 / 16 / 8 samples per stage),
its two reduce / expand chains and its right-hand-side kernels, entry by entry against a long-double Gram (oracle.gram_ld) of the regressor the
device itself evaluates.  GPU only.

Bound (tests/_gram_ref.py, derived there): |G - G_ref| <= (N + 16) 2^-53 S and |b - b_ref| <= (N + 16) 2^-53 s for EVERY entry, S and s the
sums of the absolute values of the terms.  Each case asserts which instance ran: the form and the samples per stage (timing()["gram_form"],
["gram_stage"]), the number of sample chunks (["gram_ksplit"]) and tiles x chunks x rows per chunk (["gram_issued_flops"]) against the host
mirror of the plan; more than one tile column everywhere.  G is exactly symmetric; pad rows and columns of the handle's np x np Gram and the pad
entries of b are zero (include/lpvspectral.h: lpvs_problem_device_gram_f64).

Nv = 1 (nb = 1, which also selects gram_kernel<0,16>) has no finite regressor -- gamma = 1 / 0 in the reference itself, test_gram_ref_host.py --
so those two cases assert the instance and that the NaN arrives everywhere; the nb = 1 tile geometry (65 + 129 frequencies per tile) therefore has
no value check.  gram_kernel<0,16> and <0,8> are held to the bound at nb = 320 and nb = 640, where the activation rows push two 32-sample
(16-sample) images past 160 KiB.

The structured forms (ap, ap-nufft) are held, entry by entry, to a long-double Gram with long-double phases at the scale of the activation pair
(second to last section), and, where the low words of their phases decide (|w x| from 3e6 to 2^30 rad), G and b to a long-double Gram whose phases
are those of the real products (last section).  Every test prints its worst ratio to the bound; DESIGN 4.3.1 tabulates them."""
import numpy as np
import pytest

import _gram_ref as R
import _phase_ref as PR
from _guards import precondition_not_met

pytestmark = pytest.mark.gpu

LPV = {c[0]: c for c in R.LPV_CASES}
FOURIER = {c[0]: c for c in R.FOURIER_CASES}


def _full(p):
    """The handle's np x np Gram and [ns][np] right-hand sides as they sit on the device (pad rows included)."""
    Gt, bt = p.device_gram()
    return Gt.cpu().numpy().copy(), bt.cpu().numpy().copy()


def _assert_instance(tm, form, stage, pl, N, name):
    assert tm["gram_form"] == form, (name, tm["gram_form"])
    assert tm["gram_stage"] == stage, (name, tm["gram_stage"])
    assert pl["tile_cols"] >= 2, (name, pl)
    assert tm["gram_ksplit"] == pl["ksplit"], (name, tm["gram_ksplit"], pl)
    assert tm["gram_issued_flops"] == pl["issued"], (name, tm["gram_issued_flops"], pl)      # tiles x 128 x 256 x 2 x (chunks x rows per chunk)
    if N == 1500:
        assert pl["ksplit"] * pl["rows_per_chunk"] == 1536, pl                               # 36 zero pad rows
        assert pl["ksplit"] == 3 or name == "krs-65x19", pl      # (192 tiles fill whole rounds of 256 workgroups equally at 1, 2, 3 chunks: one chunk of 1536)
    if N == 333:
        assert (pl["ksplit"], pl["rows_per_chunk"]) == (1, 384), pl                          # one chunk, 51 pad rows


def _assert_entries(G, b, Gf, bf, ref, N, name):
    """ref = (G_ref, S, b_ref [n] or [n][ns], s); b likewise; Gf, bf the padded device arrays."""
    G_ref, S, b_ref, s = ref
    n = G.shape[0]
    if not (S.min() > 1e-200 and s.min() > 1e-200):
        precondition_not_met(f"{name}: a scale of the bound underflows (min S {S.min():.3g}, min s {s.min():.3g})")
    rg, rb = np.abs(G - G_ref) / R.bound(N, S), np.abs(b - b_ref) / R.bound(N, s)
    print(f"{name}: N = {N}, n = {n}: worst |G - G_ref| / bound {rg.max():.4f} over {rg.size} entries, worst |b - b_ref| / bound {rb.max():.4f} over {rb.size}")
    assert np.all(rg <= 1.0), (name, "G", int(np.sum(rg > 1)), np.unravel_index(np.argmax(rg), rg.shape), float(rg.max()))
    assert np.all(rb <= 1.0), (name, "b", int(np.sum(rb > 1)), int(np.argmax(rb.reshape(n, -1).max(axis=1))), float(rb.max()))
    assert np.array_equal(G, G.T), name
    assert np.array_equal(Gf[:n, :n], G) and not Gf[n:, :].any() and not Gf[:, n:].any(), name
    assert np.array_equal(bf[:, :n].T.reshape(b.shape), b) and not bf[:, n:].any(), name
    return float(rg.max()), float(rb.max())


# ---------------------------------------------------------------------------------------------------------------- LPV: KRS and KR
class _LpvShared:
    """References and device results of the LPV cases, computed on first use and shared by the tests of this module (a reference is never
    modified); released when the module is done."""

    def __init__(self, L, oracle):
        self.L, self.oracle, self._ref, self._run = L, oracle, {}, {}

    def ref(self, case):
        """(device regressor, (G_ref, S, b_ref, s) or None for Nv = 1)"""
        key = (case[1], case[2], case[3], case[7])
        if key not in self._ref:
            y, X, V, w = R.lpv_inputs(case)
            Phi = self.L.lpv_regressor(X, V, w, case[2], normalize=case[7], permuted=True)   # the device's own trig and activation tables
            self._ref[key] = (Phi, self.oracle.gram_ld(Phi, y)) if case[2] > 1 else (Phi, None)
        return self._ref[key]

    def run(self, case):
        """(G, b, padded G, padded b, timing) of the case"""
        if case[0] not in self._run:
            y, X, V, w = R.lpv_inputs(case)
            with self.L.default_options(gram_form=case[4]):
                with self.L.Problem.lpv(y, X, V, w, case[2], normalize=case[7]) as p:
                    self._run[case[0]] = p.get_gram() + _full(p) + (p.timing(),)
        return self._run[case[0]]


@pytest.fixture(scope="module")
def lpv(L, oracle):
    shared = _LpvShared(L, oracle)
    yield shared
    shared._ref.clear()
    shared._run.clear()


@pytest.mark.parametrize("cid", [c for c in R.LPV_IDS if LPV[c][2] > 1])
def test_lpv_gram_instance_entry_by_entry(lpv, cid):
    case = LPV[cid]
    _, Nf, Nv, N, _, form, stage, _, _ = case
    G, b, Gf, bf, tm = lpv.run(case)
    _assert_instance(tm, form, stage, R.plan(form, 2 * Nf * Nv, N, Nf, Nv), N, cid)
    _assert_entries(G, b, Gf, bf, lpv.ref(case)[1], N, cid)


@pytest.mark.parametrize("cid,permuted", [("kr-1x320", True), ("kr-1x640", False), ("kr-auto-3x50", True)])
def test_lpv_regressor_beyond_127_basis_functions(L, oracle, cid, permuted):
    """The materialised regressor stages 64 basis functions at a time (blockIdx.z), so its LDS image does not grow with nb: nb = 50 (one
    chunk), 320 (five) and 640 (ten) -- the sizes where gram_kernel<0,16> and <0,8> live, and where one image of all nb activations would pass
    the 64 KiB a launch gets by default -- against the CPU oracle at the 4e-15 of tests/test_gpu_random.py, both column orders."""
    case = LPV[cid]
    y, X, V, w = R.lpv_inputs(case)
    Phi = L.lpv_regressor(X, V, w, case[2], case[7], False, permuted)
    Po = oracle.lpv_regressor(X, V, w, case[2], case[7], False, permuted)
    assert Phi.shape == Po.shape == (case[3], 2 * case[1] * case[2]) and np.isfinite(Phi).all()
    assert np.abs(Phi - Po).max() <= 4e-15 * max(1.0, np.abs(Po).max()), np.abs(Phi - Po).max()
    assert np.count_nonzero(Phi) > 0.5 * Phi.size


@pytest.mark.parametrize("cid", [c for c in R.LPV_IDS if LPV[c][2] == 1])
def test_single_basis_function_runs_the_16_sample_kr_instance(lpv, cid):
    """nb = 1: 65 + 129 frequencies per tile, two 32-sample images need 196 KiB -> gram_kernel<0,16>; asking for krs runs kr too
    (gram_krs_fits needs nb >= 2).  The regressor is NaN as the reference's is, and the NaN reaches every entry; no value of this tile geometry
    is checked."""
    case = LPV[cid]
    G, b, Gf, bf, tm = lpv.run(case)
    _assert_instance(tm, "kr", 16, R.plan("kr", 2 * case[1], case[3]), case[3], cid)
    Phi = lpv.ref(case)[0]
    assert np.isnan(Phi).all() and np.isnan(G).all() and np.isnan(b).all()
    n = G.shape[0]
    assert not Gf[n:, :].any() and not Gf[:, n:].any() and not bf[:, n:].any()


def test_one_k_shortcut_agrees_with_krs_and_shares_its_rhs(lpv):
    """2 nb == 16 through kr (one activation read per k-step) and through krs at the same two shapes: both inside the same bound (asserted per case
    above, repeated here side by side), and -- one right-hand-side kernel serves both -- the same b bit for bit."""
    for a, c in (("kr-20x8", "krs-20x8"), ("kr-17x8", "krs-17x8")):
        Ga, ba, _, _, tma = lpv.run(LPV[a])
        Gc, bc, _, _, tmc = lpv.run(LPV[c])
        assert (tma["gram_form"], tmc["gram_form"]) == ("kr", "krs")
        assert np.array_equal(ba, bc), a
        G_ref, S, _, _ = lpv.ref(LPV[a])[1]
        ra, rc = R.worst_ratio(Ga, G_ref, 1500, S), R.worst_ratio(Gc, G_ref, 1500, S)
        print(f"{a}: worst ratio to the bound, kr (one_k) {ra:.4f}, krs {rc:.4f}; largest |kr - krs| / bound {R.worst_ratio(Ga, Gc, 1500, S):.4f}")
        assert ra <= 1.0 and rc <= 1.0 and not np.array_equal(Ga, Gc)          # (two groupings of the four factors: not the same bits)


@pytest.mark.parametrize("cid", ["krs-66x5", "kr-22x7", "krs-8x20"])
def test_two_builds_of_one_lpv_problem_are_bit_identical(L, lpv, cid):
    """The chunk slabs are summed in fixed order: no float atomics, no dependence on which workgroup finishes first."""
    case = LPV[cid]
    G, b, Gf, bf, _ = lpv.run(case)
    y, X, V, w = R.lpv_inputs(case)
    with L.default_options(gram_form=case[4]):
        with L.Problem.lpv(y, X, V, w, case[2], normalize=case[7]) as p:
            G2, b2 = p.get_gram()
    assert np.array_equal(G, G2) and np.array_equal(b, b2)


def test_multi_signal_rhs_on_the_side_stream(L, oracle, lpv):
    """Problem.lpv_multi, three signals, KRS (70, 2): launch_rhs_kr once per signal underneath the Gram kernel; every b_q entry by entry."""
    case = LPV["krs-70x2"]
    _, Nf, Nv, N = case[:4]
    Y, X, V, w = R.lpv_inputs(case, ns=3)
    Phi = L.lpv_regressor(X, V, w, Nv, normalize=True, permuted=True)
    ref = oracle.gram_ld(Phi, Y)
    with L.Problem.lpv_multi(Y, X, V, w, Nv) as p:
        G, _ = p.get_gram()
        B = p.get_rhs()
        Gf, bf = _full(p)
        tm = p.timing()
    assert B.shape == (2 * Nf * Nv, 3) and len({B[:, q].tobytes() for q in range(3)}) == 3
    _assert_instance(tm, "krs", 32, R.plan("krs", 2 * Nf * Nv, N, Nf, Nv), N, "krs-70x2 x 3 signals")
    _assert_entries(G, B, Gf, bf, ref, N, "krs-70x2 x 3 signals")
    assert np.array_equal(G, lpv.run(case)[0])              # the Gram does not depend on the signals


# ---------------------------------------------------------------------------------------------------------------- PANEL
@pytest.mark.parametrize("cid", R.FOURIER_IDS)
def test_fourier_panel_gram_entry_by_entry(L, oracle, cid):
    case = FOURIER[cid]
    _, Nf, zero, weighted, N = case
    y, t, f, W = R.fourier_inputs(case)
    A, zf = L.get_fourier_regressor(t, f)
    n = 2 * Nf - int(zero)
    assert A.shape == (N, n) and bool(zf) == zero
    ref = oracle.gram_ld(A, y, W)
    with L.Problem.fourier(y, t, f, W) as p:
        G, b = p.get_gram()
        Gf, bf = _full(p)
        tm = p.timing()
    _assert_instance(tm, "panel", 16, R.plan("panel", n, N), N, cid)
    _assert_entries(G, b, Gf, bf, ref, N, cid)
    if weighted and N == 1500:                                  # second build: bit identical
        with L.Problem.fourier(y, t, f, W) as p:
            G2, b2 = p.get_gram()
        assert np.array_equal(G, G2) and np.array_equal(b, b2)


@pytest.mark.parametrize("N", [1500, 333])
def test_dense_panel_integer_family_bit_for_bit(L, N):
    """A in {-3 .. 3}, y in {-2 .. 2}: every partial sum is an integer below 2^53, so any summation order is exact and a dropped, repeated or
    pad row shows as an integer."""
    A, y = R.integer_family(N)
    Ai, yi = A.astype(np.int64), y.astype(np.int64)
    with L.Problem.dense(A, y) as p:
        G, b = p.get_gram()
        Gf, bf = _full(p)
        tm = p.timing()
    _assert_instance(tm, "panel", 16, R.plan("panel", 300, N), N, f"dense-{N}")
    assert np.array_equal(G, Ai.T @ Ai) and np.array_equal(b, Ai.T @ yi)
    assert np.array_equal(Gf[:300, :300], G) and not Gf[300:, :].any() and not Gf[:, 300:].any() and not bf[:, 300:].any()
    Wi = np.arange(N) % 3 + 1.0                                 # integer weights: the weighted A operand and W .* y stay exact
    with L.Problem.dense(A, y, Wi) as p:
        Gw, bw = p.get_gram()
    Wl = Wi.astype(np.int64)
    assert np.array_equal(Gw, Ai.T @ (Wl[:, None] * Ai)) and np.array_equal(bw, Ai.T @ (Wl * yi))


def _window_inputs():
    rng = np.random.default_rng(77)
    n, nwin, Nf = 1024, 3, 140
    t = np.cumsum(0.5 + rng.random(n * nwin))
    f = (np.arange(Nf) + 1.0 + 0.35 * rng.uniform(-1, 1, Nf)) * (0.45 / (Nf + 1))          # non-uniform, no two frequencies closer than 0.3 of the mean spacing
    Y = [np.sin(2 * np.pi * f[17 + 40 * q] * t + q) + 0.3 * rng.standard_normal(n * nwin) for q in range(2)]
    return n, nwin, Nf, t, f, Y


def test_weighted_window_grams_entry_by_entry_and_through_the_batch(L, oracle):
    """Three windows of 1024 samples, 280 columns (two tile columns), Hann + 0.1 weights, two signals.  The engine keeps a window's Q, q on the
    device, so they are read the way tests/test_gpu_windows.py reads them -- a single-window handle per window and signal -- and held to the bound
    entry by entry; the batch itself (launch_gram_panel_batch, gram_reduce_kernel over blockIdx.z, rhs_panel_batch_kernel, rhs_reduce_batch_kernel)
    is then held through the dense estimator (Q + lam I) x = q to the solution of the long-double Q_ref, q_ref.  Tolerance, first order in the
    perturbations: with H = Q_ref + lam I, ||dx|| / ||x|| <= cond(H) (||dQ|| / ||H|| + ||dq|| / ||q||) for the Gram's own error, |dQ| <= B_Q and
    |dq| <= B_q entrywise (the bounds above, ||dQ||_2 <= ||B_Q||_F), plus cond(H) n 2^-53 for the explicit inverse and its product with q in doubles."""
    from lpvspectral_jl_amd import api
    n, nwin, Nf, t, f, Y = _window_inputs()
    W = np.asarray(L.hanning(n)) + 0.1
    lam = 1e-3
    eng = dict(estimator=2, lam=lam, prox=(1, 0.0, 0), μ=0.05, tol=0.0, iters=0, sign=1)
    x, _ = L.windows_estimate(Y, t, f, n, 0, W, eng)
    assert x.shape == (2, nwin, Nf) and api.windowpsd_last_timing()["gram_form"] == "dense"
    pl = R.plan("panel", 2 * Nf, n)
    for i in range(nwin):
        ti = t[i * n:(i + 1) * n]
        A, _ = L.get_fourier_regressor(ti, f)
        G_ref, S, B_ref, s = oracle.gram_ld(A, np.stack([yq[i * n:(i + 1) * n] for yq in Y], axis=1), W)
        for q in range(2):
            with L.Problem.fourier(Y[q][i * n:(i + 1) * n], ti, f, W) as p:
                Q, qv = p.get_gram()
                Gf, bf = _full(p)
                tm = p.timing()
            _assert_instance(tm, "panel", 16, pl, n, f"window {i} signal {q}")
            _assert_entries(Q, qv, Gf, bf, (G_ref, S, B_ref[:, q], s[:, q]), n, f"window {i} signal {q}")
            H = G_ref + lam * np.eye(2 * Nf)
            sv = np.linalg.svd(H, compute_uv=False)
            tol = sv[0] / sv[-1] * (np.linalg.norm(R.bound(n, S)) / sv[0] + np.linalg.norm(R.bound(n, s[:, q])) / np.linalg.norm(B_ref[:, q]) + 2 * Nf * R.U)
            xr = np.linalg.solve(H, B_ref[:, q])
            xr = xr[:Nf] + 1j * xr[Nf:]
            e = np.linalg.norm(x[q, i] - xr) / np.linalg.norm(xr)
            print(f"window {i} signal {q}: batch engine (Q + lam I) x = q vs the long-double Q, q: rel-L2 {e:.2e}, bound {tol:.2e} (cond {sv[0] / sv[-1]:.1f})")
            assert e <= tol, (i, q, e, tol)


# ---------------------------------------------------------------------------------------------------------------- structured forms at pair scale
def _struct_forms(L, monkeypatch, make):
    """{mode: (G, form)} for the slot sums evaluated directly (nudft.hip) and by default (nufft.hip where it applies)."""
    out = {}
    for mode in ("direct", None):
        if mode:
            monkeypatch.setenv("LPVS_NUDFT", mode)
        else:
            monkeypatch.delenv("LPVS_NUDFT", raising=False)
        with make() as p:
            out[mode or "default"] = (p.get_gram()[0], p.timing())
    monkeypatch.delenv("LPVS_NUDFT", raising=False)
    return out


@pytest.mark.parametrize("case", R.STRUCT_LPV_CASES, ids=[c[0] for c in R.STRUCT_LPV_CASES])
def test_structured_lpv_gram_at_pair_scale(L, oracle, monkeypatch, case):
    """ap / ap-nufft on a progression grid: every entry within (1e-12 + 4.5e-16 max|w| max|x|) C[j(a)][j(b)] of the long-double Gram whose
    phases are formed in long double, C the weight sum of the activation pair."""
    cid, Nf, Nv, N = case
    y, X, V, w = R.struct_lpv_inputs(case)
    K = L.basis_activation_func(V, Nv)                          # the device's activation table
    G_ref = oracle.gram_phase_ld(X, w, K)
    C = np.abs(K).T @ np.abs(K)
    j = np.arange(2 * Nf * Nv) % Nv
    bnd = R.struct_tol(w.max(), np.abs(X).max()) * C[np.ix_(j, j)]
    if not C.min() > 1e-200:
        precondition_not_met(f"{cid}: a pair scale underflows ({C.min():.3g})")
    res = _struct_forms(L, monkeypatch, lambda: L.Problem.lpv(y, X, V, w, Nv))
    assert res["direct"][1]["gram_form"] == "ap" and res["default"][1]["gram_form"] == "ap-nufft", {k: v[1]["gram_form"] for k, v in res.items()}
    worst = {}
    for mode, (G, tm) in res.items():
        assert tm["gram_stage"] == 0 and tm["gram_ksplit"] == 0
        r = np.abs(G - G_ref) / bnd
        worst[mode] = float(r.max())
        print(f"{cid} {tm['gram_form']} ({mode}): worst |G - G_ref| / pair-scale bound {r.max():.4f} over {r.size} entries")
    for mode, (G, tm) in res.items():
        assert worst[mode] <= 1.0, (cid, mode, worst)
        assert np.array_equal(G, G.T)


@pytest.mark.parametrize("case", R.STRUCT_FOURIER_CASES, ids=[c[0] for c in R.STRUCT_FOURIER_CASES])
def test_structured_fourier_gram_at_weight_scale(L, oracle, monkeypatch, case):
    """The Fourier form of the same: scale sum_k |W_k| / (2 Nf).  Single Fourier handles evaluate their slot sums directly in both modes."""
    cid, Nf, zero, weighted, N = case
    y, t, f, W = R.struct_fourier_inputs(case)
    G_ref = oracle.gram_phase_ld(t, 6.283185307179586 * f, None, zero, W)
    bnd = R.struct_tol(2 * np.pi * f.max(), t.max()) * (N if W is None else np.abs(W).sum()) / (2 * Nf)
    res = _struct_forms(L, monkeypatch, lambda: L.Problem.fourier(y, t, f, W))
    worst = {}
    for mode, (G, tm) in res.items():
        assert tm["gram_form"] == "ap" and tm["gram_stage"] == 0 and tm["gram_ksplit"] == 0, (mode, tm)
        r = np.abs(G - G_ref) / bnd
        worst[mode] = float(r.max())
        print(f"{cid} {tm['gram_form']} ({mode}): worst |G - G_ref| / weight-sum bound {r.max():.4f} over {r.size} entries")
    for mode, (G, tm) in res.items():
        assert worst[mode] <= 1.0, (cid, mode, worst)
        assert np.array_equal(G, G.T)


# ---------------------------------------------------------------------------------------------------------------- structured forms, exact phases
# The cases above keep |w x| <= 1e3 rad, where the low words of the device's phases (the FMA error of omega x, the low word of the
# double-double slot frequency, the first-order use of both) move a phase by 1e-13: below the tolerance.  Here they decide: |w x| reaches
# 3e6 rad (the benchmark's scale), 4e7 rad (Fourier stamps late in a record) and 2^30 rad, against tests/_phase_ref.py, whose phases are
# those of the real products at any magnitude.  Bound (tests/_gram_ref.py): (1e-12 + q) x the weight sum, q <= 1e-13 the squares the kernel
# headers name; nothing grows with |w||x|.  tests/test_phase_ref_host.py shows on the CPU that a kernel which dropped or negated any one low
# word would miss these bounds by a factor of ten or more, term by term.
PHASE_SLOT = {"bench-24x3": (True, 2), "bench-20x8": (True, 2), "bench-24x3-multi": (True, 2), "beyond-24x3": (True, 2), "resid-a=D": (True, 2),
              "resid-a=1.5D": (True, 3), "resid-a=0": (True, 0), "resid-split": (False, None)}


def _phase_tol(w, x, name):
    q = PR.second_order(w, x)
    assert q <= 1e-13, (name, float(q))                          # so that q cannot hide anything
    return 1e-12 + q


@pytest.mark.parametrize("cid", [c[0] for c in R.PHASE_LPV_CASES])
def test_structured_lpv_gram_and_rhs_against_exact_phases(L, monkeypatch, cid):
    """G AND b of ap / ap-nufft, every entry, where the low words of the phases decide: the benchmark's scale with natural rounding
    residuals (one and three signals), 2^30 rad on a dyadic grid, and planted residuals at the admission limit in every slot layout (merged
    with s0 = 2, 3, 0; split, which keeps the direct sums)."""
    case = R.PHASE_LPV[cid]
    _, Nf, Nv, grid, _, a_over_D, resid, ns = case
    Y, X, V, w = R.phase_lpv_inputs(case)
    N, n = R.PHASE_N, 2 * Nf * Nv
    xmax = np.abs(X).max()
    merged, s0, delta = PR.merged_slot(w, xmax)
    assert (merged, s0) == PHASE_SLOT[cid] and (grid != "dyadic" or (delta == 0.0 and not PR.progression(w)[2].any()))
    if resid:
        eps = PR.progression(w)[2]
        assert eps[0] == 0.0 and eps[-1] == 0.0 and 0.85e-7 <= np.abs(eps).max() * xmax <= 1e-7
    tol = _phase_tol(w, X, cid)
    G_ref, b_ref, C, s = PR.lpv_gram_exact(X, w, L.basis_activation_func(V, Nv), Y)     # the device's activation table
    if not (C.min() > 1e-200 and s.min() > 1e-200):
        precondition_not_met(f"{cid}: a scale underflows ({float(C.min()):.3g}, {float(s.min()):.3g})")
    j = np.arange(n) % Nv
    bG, bb = tol * C[np.ix_(j, j)], tol * s[j].reshape(n, -1)
    want = {"direct": "ap", "default": "ap" if not merged else "ap-nufft"}
    worst = {}
    for mode in ("direct", "default"):
        if mode == "direct":
            monkeypatch.setenv("LPVS_NUDFT", "direct")
        else:
            monkeypatch.delenv("LPVS_NUDFT", raising=False)
        with (L.Problem.lpv_multi(Y, X, V, w, Nv) if ns > 1 else L.Problem.lpv(Y, X, V, w, Nv)) as p:
            G, b = p.get_gram()
            if ns > 1:
                b = p.get_rhs()
            tm = p.timing()
        assert tm["gram_form"] == want[mode] and tm["gram_stage"] == 0 and tm["gram_ksplit"] == 0, (cid, mode, tm["gram_form"])
        assert G.shape == (n, n) and np.array_equal(G, G.T)
        rg = np.abs(G.astype(PR.LD) - G_ref) / bG
        rb = np.abs(b.reshape(n, -1).astype(PR.LD) - b_ref.reshape(n, -1)) / bb
        worst[mode] = (float(rg.max()), float(rb.max()))
        print(f"{cid} {tm['gram_form']} ({mode}): max|w x| = {np.abs(w).max() * xmax:.3g} rad, worst |G - G_ref| / bound {rg.max():.4f} over {rg.size} entries, "
              f"worst |b - b_ref| / bound {rb.max():.4f} over {rb.size}")
    monkeypatch.delenv("LPVS_NUDFT", raising=False)
    assert all(r <= 1.0 for pair in worst.values() for r in pair), (cid, worst)


@pytest.mark.parametrize("case", R.STRUCT_FOURIER_CASES, ids=[c[0] for c in R.STRUCT_FOURIER_CASES])
def test_structured_fourier_gram_and_rhs_against_exact_phases(L, monkeypatch, case):
    """Full-mantissa stamps in [2^24, 2^24 + 300]: |w t| = 4e7 rad (nudft_single_kernel, ap_assemble_fourier_kernel, ap_rhs_fourier_kernel)."""
    cid, Nf, zero, weighted, N = case
    y, t, f, W = R.phase_fourier_inputs(case)
    w = 6.283185307179586 * f                                    # as the library rounds it
    tol = _phase_tol(w, t, cid)
    G_ref, b_ref, sG, sb = PR.fourier_gram_exact(t, w, y, zero, W)
    worst = {}
    for mode in ("direct", "default"):
        if mode == "direct":
            monkeypatch.setenv("LPVS_NUDFT", "direct")
        else:
            monkeypatch.delenv("LPVS_NUDFT", raising=False)
        with L.Problem.fourier(y, t, f, W) as p:
            G, b = p.get_gram()
            tm = p.timing()
        assert tm["gram_form"] == "ap" and tm["gram_stage"] == 0 and tm["gram_ksplit"] == 0, (mode, tm)
        assert np.array_equal(G, G.T)
        rg, rb = np.abs(G.astype(PR.LD) - G_ref) / (tol * sG), np.abs(b.astype(PR.LD) - b_ref) / (tol * sb)
        worst[mode] = (float(rg.max()), float(rb.max()))
        print(f"{cid} ap ({mode}): max|w t| = {w.max() * t.max():.3g} rad, worst |G - G_ref| / bound {rg.max():.4f} over {rg.size} entries, "
              f"worst |b - b_ref| / bound {rb.max():.4f} over {rb.size}")
    monkeypatch.delenv("LPVS_NUDFT", raising=False)
    assert all(r <= 1.0 for pair in worst.values() for r in pair), (cid, worst)


def _solve_ld(H, q):
    """H x = q in long double: a double solve refined three times on long-double residuals (cond(H) ~ 1e4: each step gains 12 digits)."""
    Hd = H.astype(np.float64)
    x = np.linalg.solve(Hd, q.astype(np.float64)).astype(PR.LD)
    for _ in range(3):
        x = x + np.linalg.solve(Hd, (q - H @ x).astype(np.float64)).astype(PR.LD)
    return x


def test_window_engine_structured_forms_against_exact_phases(L, monkeypatch):
    """Three Hann windows of 2048 samples late in a long record (t = 2^26 + k / 2 + jitter, full mantissa: |w t| = 2e8 rad), 33 frequencies
    (72 slots), two signals: the engine's structured forms -- nudft with segments (LPVS_NUDFT=direct: ap) and nufft_window_kernel (default:
    ap-nufft) -- through the dense estimator (Q + lam I) x = q, against the long-double solve of the exact-phase Q, q.  The engine returns no
    Gram, so the tolerance is that of test_weighted_window_grams_entry_by_entry_and_through_the_batch with this section's entry bounds in place of
    R.bound: cond(H) (||B_Q||_F / ||H|| + ||B_q|| / ||q|| + n 2^-53), B_Q = (1e-12 + q) sum|W| / (2 Nf) and B_q = (1e-12 + q) sum|W y| / sqrt(2 Nf)
    per entry."""
    from lpvspectral_jl_amd import api
    n, nwin, Nf, t, f, Y = R.phase_window_inputs()
    lam, w = 1e-3, 6.283185307179586 * f
    W = np.asarray(L.hanning(n), dtype=np.float64)
    tol = _phase_tol(w, t, "windows")
    eng = dict(estimator=2, lam=lam, prox=(1, 0.0, 0), μ=0.05, tol=0.0, iters=0, sign=1)
    res = {}
    for mode in ("direct", "default"):
        if mode == "direct":
            monkeypatch.setenv("LPVS_NUDFT", "direct")
        else:
            monkeypatch.delenv("LPVS_NUDFT", raising=False)
        res[mode] = api.windows_estimate(Y, t, f, n, 0, W, eng)[0]
        assert res[mode].shape == (2, nwin, Nf) and api.windowpsd_last_timing()["gram_form"] == ("ap" if mode == "direct" else "ap-nufft")
    monkeypatch.delenv("LPVS_NUDFT", raising=False)
    worst = {"direct": 0.0, "default": 0.0}
    for i in range(nwin):
        ti = t[i * n:(i + 1) * n]
        for q in range(2):
            G_ref, b_ref, sG, sb = PR.fourier_gram_exact(ti, w, Y[q][i * n:(i + 1) * n], False, W)
            H = G_ref + lam * np.eye(2 * Nf)
            sv = np.linalg.svd(H.astype(np.float64), compute_uv=False)
            bound = sv[0] / sv[-1] * (float(tol * sG) * 2 * Nf / sv[0] + float(tol * sb) * np.sqrt(2 * Nf) / float(np.linalg.norm(b_ref.astype(np.float64))) + 2 * Nf * R.U)
            xr = _solve_ld(H, b_ref)
            xr = (xr[:Nf] + 1j * xr[Nf:]).astype(np.complex128)
            for mode, x in res.items():
                e = np.linalg.norm(x[q, i] - xr) / np.linalg.norm(xr)
                worst[mode] = max(worst[mode], e / bound)
                print(f"window {i} signal {q} ({mode}): (Q + lam I) x = q vs the exact-phase long-double solve: rel-L2 {e:.2e}, bound {bound:.2e} (cond {sv[0] / sv[-1]:.1f})")
    assert worst["direct"] <= 1.0 and worst["default"] <= 1.0, worst
