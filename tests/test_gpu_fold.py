"""pdm / aov and conditional_entropy on the GPU against tests/_fold_ref.py: the models (the definition as the device computes it: integers
exactly, doubles within the counted roundings) and the long-double definitions (within the bounds derived there and proven on the host
by tests/test_fold_ref_host.py).

INPUTS follow the bls family (tests/_bls_ref.py: base_case): t in multiples of 2^-10 below 2^9, f in multiples of 2^-6, so f t, the fold
and phi n are exact for every n <= 2048 and the references are unambiguous.  One case more has generic doubles and is held to the
two_product fold.

SHAPES (tests/_fold_ref.py: PDM_CASES, CENT_CASES): N in {1, 255, 256, 257, 1500}; Nf in {1, 70, 1030}; ns in {1, 2, 3, 5}; pdm with
(nbins, covers) in {(2, 1), (5, 2), (10, 1), (100, 1), (8, 4), (512, 4)}, with and without W, centring on and off; conditional entropy
with (nbins, mbins) in {(2, 2), (10, 5), (20, 8), (64, 64), (256, 32), (20, 20)}.  With them every F in {1, 2, 4} and every TS in
{1, 2, 4} the plans can pick is reached, asserted from the timing records; the plan keeps one copy of the count histogram, and 2 and 4
copies are reached through the experiment knob LPVS_CENT_COPIES (4 is halved to 2 where the LDS does not hold it)."""
import ctypes
import functools

import numpy as np
import pytest

from _bls_ref import LD, base_case, device_moments, fold_bins, ld_bins
from _fold_ref import (CENT_CASES, PDM_CASES, aov_of, case_inputs, cent_bound, cent_c, cent_model, cent_ref_ld, pdm_bounds, pdm_model, pdm_ref_ld, pdm_ulps,
                       sawtooth_case, theta_of, U)

pytestmark = pytest.mark.gpu


def _raw_pdm(y, t, f, W, nbins, covers, center_data=True, device_out=False, hists=True):
    """lpvs_pdm_f64 itself.  -> dict of (Nf, ns) arrays, nonempty (Nf,), the histograms and the timing record."""
    import lpvspectral_jl_amd as L
    from lpvspectral_jl_amd._lib import check, lib, out_ptr
    y = np.asfortranarray(np.asarray(y, np.float64).reshape(len(t), -1))
    N, ns = y.shape
    f = np.ascontiguousarray(f, dtype=np.float64)
    Nf, nfine = len(f), max(nbins * covers, 1)
    t = np.ascontiguousarray(t, dtype=np.float64)
    Wa = None if W is None else np.ascontiguousarray(W, dtype=np.float64)
    ex, M, deg = np.full((ns, Nf), -7.0), np.zeros(Nf, np.int32), np.zeros((ns, Nf), np.int32)
    hist, hcount = np.zeros((Nf, 1 + ns, nfine), np.int64), np.zeros((Nf, nfine), np.int32)
    plane = out_ptr(ex)
    if device_out:
        import torch
        dev = torch.full((ns, Nf), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        plane = ctypes.c_void_p(dev.data_ptr())
    check(lib().lpvs_pdm_f64(out_ptr(y), ns, out_ptr(t), N, None if Wa is None else out_ptr(Wa), out_ptr(f), Nf, nbins, covers, int(center_data), 0, plane,
                             out_ptr(M), out_ptr(deg), out_ptr(hist) if hists else None, out_ptr(hcount) if hists else None))
    if device_out:
        ex = dev.cpu().numpy()
    return dict(explained=ex.T, nonempty=M, degenerate=deg.T, hist=hist, hcount=hcount, timing=L.pdm_last_timing())


def _raw_cent(y, t, f, nbins, mbins, device_out=False):
    import lpvspectral_jl_amd as L
    from lpvspectral_jl_amd._lib import check, lib, out_ptr
    y = np.asfortranarray(np.asarray(y, np.float64).reshape(len(t), -1))
    N, ns = y.shape
    f = np.ascontiguousarray(f, dtype=np.float64)
    Nf = len(f)
    t = np.ascontiguousarray(t, dtype=np.float64)
    H, ylim, deg = np.full((ns, Nf), -7.0), np.zeros((ns, 2)), np.zeros(ns, np.int32)
    hist = np.zeros((Nf, ns, max(nbins, 1), max(mbins, 1)), np.int32)
    plane = out_ptr(H)
    if device_out:
        import torch
        dev = torch.full((ns, Nf), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        plane = ctypes.c_void_p(dev.data_ptr())
    check(lib().lpvs_cent_f64(out_ptr(y), ns, out_ptr(t), N, out_ptr(f), Nf, nbins, mbins, 0, plane, out_ptr(ylim), out_ptr(deg), out_ptr(hist)))
    if device_out:
        H = dev.cpu().numpy()
    return dict(entropy=H.T, ylim=ylim, degenerate=deg, hist=hist, timing=L.cent_last_timing())


PDM_KEYS = ("explained", "nonempty", "degenerate", "hist", "hcount")
CENT_KEYS = ("entropy", "ylim", "degenerate", "hist")


def _bits(r, keys):
    return tuple(np.ascontiguousarray(r[k]).tobytes() for k in keys)


@functools.lru_cache(maxsize=None)
def _pdm_inputs(name):
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES[name]
    return case_inputs(N, Nf, ns, weighted)


@functools.lru_cache(maxsize=None)
def _pdm_refs(name):
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES[name]
    t, f, y, W = _pdm_inputs(name)
    return pdm_model(y, t, f, W, nbins, covers, center), pdm_ref_ld(y, t, f, W, nbins, covers, center)


@functools.lru_cache(maxsize=None)
def _pdm_device(name):
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES[name]
    t, f, y, W = _pdm_inputs(name)
    return _raw_pdm(y, t, f, W, nbins, covers, center)


@functools.lru_cache(maxsize=None)
def _cent_inputs(name):
    N, Nf, nbins, mbins, ns, plan = CENT_CASES[name]
    return case_inputs(N, Nf, ns, False)[:3]


@functools.lru_cache(maxsize=None)
def _cent_refs(name):
    N, Nf, nbins, mbins, ns, plan = CENT_CASES[name]
    t, f, y = _cent_inputs(name)
    return cent_model(y, t, f, nbins, mbins), cent_ref_ld(y, t, f, nbins, mbins)


@functools.lru_cache(maxsize=None)
def _cent_device(name):
    N, Nf, nbins, mbins, ns, plan = CENT_CASES[name]
    t, f, y = _cent_inputs(name)
    return _raw_cent(y, t, f, nbins, mbins)


def _check_pdm(d, m, r, y, W, center, nfine):
    assert np.array_equal(d["hist"], m["hist"]), "the integer histograms"
    assert np.array_equal(d["hcount"], m["hcount"]), "the counts per fine bin"
    assert np.array_equal(d["nonempty"], m["nonempty"]) and np.array_equal(d["degenerate"] != 0, m["degenerate"] != 0)
    assert d["timing"]["degenerate"] == m["ndeg"] == int(d["degenerate"].sum())
    assert np.all(np.isfinite(d["explained"])) and np.all(d["explained"] >= 0) and np.all(d["explained"] <= 1)
    tol = pdm_ulps(nfine) * U * np.maximum(m["gross"], m["explained"])
    e = np.abs(d["explained"] - m["explained"])
    print(f"explained: device against model, worst {float((e / np.where(tol > 0, tol, 1)).max()):.3g} of the allowance of {pdm_ulps(nfine)} roundings")
    assert np.all(e <= tol)
    live = d["degenerate"] == 0
    if live.any():
        b = pdm_bounds(y, W, center, m["shy"], nfine, r["explained"])
        e = np.abs(d["explained"].astype(LD) - np.minimum(r["explained"], 1))
        print(f"explained: device against long double, worst error / bound {float((e / b)[live].max()):.3g}")
        assert np.all(e[live] <= b[live])


def _check_cent(d, m, r, cells):
    assert np.array_equal(d["hist"], m["hist"]), "the counts (the value bins with them)"
    assert np.array_equal(d["ylim"], m["ylim"]) and np.array_equal(d["degenerate"], m["degenerate"])
    assert np.all(np.isfinite(d["entropy"])) and np.all(d["entropy"] >= 0)
    for name, ref in (("model", m["entropy"]), ("long double", r)):
        e, b = np.abs(d["entropy"].astype(LD) - ref), cent_bound(cells, ref)
        print(f"entropy: device against {name}, worst error / bound {float((e / b).max()):.3g} (c = {cent_c(cells)})")
        assert np.all(e <= b)


@pytest.mark.parametrize("name", list(PDM_CASES))
def test_pdm_every_shape_against_the_model_and_the_long_double_definition(name):
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES[name]
    t, f, y, W = _pdm_inputs(name)
    m, r = _pdm_refs(name)
    d = _pdm_device(name)
    tm = d["timing"]
    assert (tm["F"], tm["ts"], tm["passes"]) == plan, tm
    assert tm["unit"] == (W is None) and tm["nf"] == len(f) and tm["copies"] == 1 and tm["shift_w"] == (0 if W is None else 60)
    if N > 1:
        assert (tm["shift_y_min"], tm["shift_y_max"]) == (min(m["shy"]), max(m["shy"]))
    _check_pdm(d, m, r, y, W, center, nbins * covers)


@pytest.mark.parametrize("name", list(CENT_CASES))
def test_conditional_entropy_every_shape_against_the_model_and_the_long_double_definition(name):
    N, Nf, nbins, mbins, ns, plan = CENT_CASES[name]
    m, r = _cent_refs(name)
    d = _cent_device(name)
    tm = d["timing"]
    assert (tm["F"], tm["ts"], tm["passes"], tm["copies"]) == plan, tm
    assert tm["nf"] == Nf and tm["degenerate"] == int(m["degenerate"].sum()) and tm["lds_bytes"] == plan[0] * plan[3] * plan[1] * nbins * mbins * 4
    _check_cent(d, m, r, nbins * mbins)


def test_every_plan_value_is_reached():
    assert {c[-1][0] for c in PDM_CASES.values()} == {1, 2, 4} == {c[-1][1] for c in PDM_CASES.values()}
    assert {c[-1][0] for c in CENT_CASES.values()} == {1, 2, 4} == {c[-1][1] for c in CENT_CASES.values()}


@pytest.mark.parametrize("knob,name,copies", [(1, "base10x5", 1), (2, "base10x5", 2), (4, "base10x5", 4), (2, "n255f4", 2), (4, "n255f4", 4), (4, "cells400", 2)])
def test_every_number_of_copies_gives_the_same_bits(monkeypatch, knob, name, copies):
    N, Nf, nbins, mbins, ns, plan = CENT_CASES[name]
    t, f, y = _cent_inputs(name)
    monkeypatch.setenv("LPVS_CENT_COPIES", str(knob))
    d = _raw_cent(y, t, f, nbins, mbins)
    monkeypatch.delenv("LPVS_CENT_COPIES")
    assert d["timing"]["copies"] == copies and d["timing"]["lds_bytes"] == plan[0] * copies * plan[1] * nbins * mbins * 4
    assert _bits(d, CENT_KEYS) == _bits(_cent_device(name), CENT_KEYS)


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES["fine2048w"]
    t, f, y, W = _pdm_inputs("fine2048w")
    assert _bits(_raw_pdm(y, t, f, W, nbins, covers, center), PDM_KEYS) == _bits(_pdm_device("fine2048w"), PDM_KEYS)
    N, Nf, nbins, mbins, ns, plan = CENT_CASES["cells400"]
    t, f, y = _cent_inputs("cells400")
    assert _bits(_raw_cent(y, t, f, nbins, mbins), CENT_KEYS) == _bits(_cent_device("cells400"), CENT_KEYS)


def test_a_frequency_has_the_same_bits_alone_among_others_and_permuted():
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES["f4w"]
    t, f, y, W = _pdm_inputs("f4w")
    full = _pdm_device("f4w")                                                  # F = 4
    perm = np.random.default_rng(5).permutation(len(f))
    p = _raw_pdm(y, t, f[perm], W, nbins, covers, center)
    assert p["timing"]["F"] == 4
    for key in PDM_KEYS:
        assert np.array_equal(p[key], full[key][perm]), key
    for k in (0, 37, 1029):
        a = _raw_pdm(y, t, f[k:k + 1], W, nbins, covers, center)               # alone: F = 1
        assert a["timing"]["F"] == 1
        for key in PDM_KEYS:
            assert np.array_equal(a[key][0], full[key][k]), (k, key)
    N, Nf, nbins, mbins, ns, plan = CENT_CASES["n255f4"]
    t, f, y = _cent_inputs("n255f4")
    full = _cent_device("n255f4")                                              # F = 4
    p = _raw_cent(y, t, f[perm], nbins, mbins)
    assert p["timing"]["F"] == 4 and np.array_equal(p["entropy"], full["entropy"][perm]) and np.array_equal(p["hist"], full["hist"][perm])
    for k in (0, 37, 1029):
        a = _raw_cent(y, t, f[k:k + 1], nbins, mbins)
        assert a["timing"]["F"] == 1 and np.array_equal(a["entropy"][0], full["entropy"][k]) and np.array_equal(a["hist"][0], full["hist"][k])


def test_a_signal_has_the_same_bits_alone_and_among_five():
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES["n256w"]
    t, f, y, W = _pdm_inputs("n256w")
    five = _pdm_device("n256w")
    for c in (0, 3, 4):
        a = _raw_pdm(y[:, c], t, f, W, nbins, covers, center)
        assert np.array_equal(a["explained"][:, 0], five["explained"][:, c]) and np.array_equal(a["degenerate"][:, 0], five["degenerate"][:, c])
        assert np.array_equal(a["hist"][:, 1], five["hist"][:, 1 + c]) and np.array_equal(a["nonempty"], five["nonempty"])
    N, Nf, nbins, mbins, ns, plan = CENT_CASES["n256"]
    t, f, y = _cent_inputs("n256")
    five = _cent_device("n256")
    for c in (0, 3, 4):
        a = _raw_cent(y[:, c], t, f[:70], nbins, mbins)
        assert np.array_equal(a["entropy"][:, 0], five["entropy"][:70, c]) and np.array_equal(a["hist"][:, 0], five["hist"][:70, c])
        assert np.array_equal(a["ylim"][0], five["ylim"][c]) and a["degenerate"][0] == five["degenerate"][c]


def test_a_permutation_of_the_samples_changes_no_bit():
    """Every sum of conditional_entropy is an integer count and its extremes are integer atomics: no output moves.  pdm with W = None and
    center_data = False sums nothing in floating point before the quantisation (tests/test_gpu_bls.py shows on the same record that a
    tree sum of YY WOULD move)."""
    t, f, y = base_case(seed=2)
    perm = np.random.default_rng(0).permutation(len(t))
    tree = [device_moments(v.reshape(-1, 1), None, False)[4][0] for v in (y, y[perm])]
    assert tree[0] != tree[1], "the inputs do not show the property"
    for nbins, covers in ((10, 1), (5, 2), (512, 4)):
        a, b = _raw_pdm(y, t, f, None, nbins, covers, False), _raw_pdm(y[perm], t[perm], f, None, nbins, covers, False)
        assert _bits(a, PDM_KEYS) == _bits(b, PDM_KEYS) and a["timing"]["degenerate"] == 0 and np.all(a["explained"] > 0)
    Y = np.stack([y, y * y, np.cos(y)], axis=1)
    for nbins, mbins in ((10, 5), (64, 64)):
        a, b = _raw_cent(Y, t, f, nbins, mbins), _raw_cent(Y[perm], t[perm], f, nbins, mbins)
        assert _bits(a, CENT_KEYS) == _bits(b, CENT_KEYS) and np.all(a["entropy"] > 0)


def test_the_planes_may_be_device_memory():
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES["n255w"]
    t, f, y, W = _pdm_inputs("n255w")
    assert _bits(_raw_pdm(y, t, f, W, nbins, covers, center, device_out=True), PDM_KEYS) == _bits(_pdm_device("n255w"), PDM_KEYS)
    N, Nf, nbins, mbins, ns, plan = CENT_CASES["n255f4"]
    t, f, y = _cent_inputs("n255f4")
    assert _bits(_raw_cent(y, t, f, nbins, mbins, device_out=True), CENT_KEYS) == _bits(_cent_device("n255f4"), CENT_KEYS)


# ---- generic doubles -----------------------------------------------------------------------------------------------------------------------
def test_generic_doubles_fold_by_the_exact_phase():
    """t and f random, not dyadic: f t is inexact and the bin hangs on its low word.  No phi n lies within 2^-30 of an integer (asserted),
    so the device's phase -- within 2^-52 of the exact one -- falls into the exact phase's bin and the histograms are equal exactly."""
    rng = np.random.default_rng(3)
    N, Nf = 1500, 70
    t = np.sort(rng.random(N) * 4000.0)
    f = np.sort(0.25 + 2.25 * rng.random(Nf))
    y = 0.25 * rng.standard_normal(N) + np.mod(f[40] * t, 1.0)
    W = 0.5 + rng.random(N)
    for n in (100, 10):
        bins_ld, phi = ld_bins(f, t, n)
        x = phi * LD(n)
        assert np.abs(x - np.rint(x)).min() > 2.0 ** -30 and np.array_equal(fold_bins(f, t, n)[0], bins_ld)
    d = _raw_pdm(y, t, f, W, 50, 2, True)
    _check_pdm(d, pdm_model(y, t, f, W, 50, 2, True), pdm_ref_ld(y, t, f, W, 50, 2, True), y, W, True, 100)
    assert int(np.argmax(d["explained"][:, 0])) == 40
    c = _raw_cent(y, t, f, 10, 5)
    _check_cent(c, cent_model(y, t, f, 10, 5), cent_ref_ld(y, t, f, 10, 5), 50)
    assert int(np.argmin(c["entropy"][:, 0])) == 40


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
def test_integer_values_land_in_their_bins_and_the_maximum_in_the_last():
    t, f, _ = base_case(seed=0)
    y = np.random.default_rng(9).integers(0, 5, len(t)).astype(np.float64)     # u 5 = 0, 1.25, 2.5, 3.75, 5; u 4 = y exactly: ties at the edges
    for mbins, want in ((5, y), (4, np.minimum(y, 3))):
        d, m = _raw_cent(y, t, f, 10, mbins), cent_model(y, t, f, 10, mbins)
        assert np.array_equal(m["vbin"][:, 0], want.astype(np.int64))
        assert np.array_equal(d["hist"], m["hist"]) and np.array_equal(d["ylim"], [[0.0, 4.0]]) and d["degenerate"][0] == 0
        assert np.array_equal(d["hist"].sum(axis=(0, 1, 2)), len(f) * np.bincount(want.astype(np.int64), minlength=mbins))
        _check_cent(d, m, cent_ref_ld(y, t, f, 10, mbins), 10 * mbins)


def test_all_samples_in_one_phase_bin_give_flagged_zeros():
    t = np.arange(300.0)
    y = np.random.default_rng(0).standard_normal(300)
    for nbins, covers in ((10, 1), (5, 2), (8, 4)):
        d = _raw_pdm(y, t, np.array([1.0, 2.0]), None, nbins, covers)
        assert np.all(d["hcount"][:, 0] == 300) and np.all(d["hcount"][:, 1:] == 0) and np.all(d["nonempty"] == covers)
        assert np.all(d["explained"] == 0) and np.all(d["degenerate"] == 1) and d["timing"]["degenerate"] == 2
    c = _raw_cent(y, t, np.array([1.0, 2.0]), 10, 5)                           # one phase bin: H is the entropy of the values, no NaN
    assert np.all(c["hist"][:, :, 1:] == 0) and np.all(np.isfinite(c["entropy"])) and np.all(c["entropy"] > 0) and c["degenerate"][0] == 0
    p = np.bincount(cent_model(y, t, [1.0], 10, 5)["vbin"][:, 0], minlength=5) / 300.0
    assert abs(c["entropy"][0, 0] + (p[p > 0] * np.log(p[p > 0])).sum()) < 1e-14


def test_a_constant_signal_and_a_single_sample_give_flagged_zeros():
    import lpvspectral_jl_amd as L
    t, f, y = base_case(seed=0)
    W = 0.5 + np.random.default_rng(1).random(len(t))
    Y = np.stack([y, np.full(len(t), 3.7), np.zeros(len(t))], axis=1)
    for center in (True, False):
        d = _raw_pdm(Y, t, f, W, 10, 1, center)
        assert np.all(np.isfinite(d["explained"])) and np.all(d["explained"][:, 2] == 0) and np.all(d["degenerate"][:, 2] == 1)
        if center:
            assert np.all(d["explained"][:, 1] == 0) and np.all(d["degenerate"][:, 1] == 1)
            assert np.array_equal(d["explained"][:, 0], _raw_pdm(y, t, f, W, 10, 1, True)["explained"][:, 0])
    R = L.pdm(Y, t, f, W=W)
    assert np.all(R.theta[:, 1:] == 1) and np.all(R.aov[:, 1:] == 0) and np.all(np.isfinite(R.theta)) and np.all(np.isfinite(R.aov))
    c = _raw_cent(Y, t, f, 10, 5)
    assert np.array_equal(c["degenerate"], [0, 1, 1]) and np.all(c["entropy"][:, 1:] == 0) and np.all(c["entropy"][:, 0] > 0)
    assert np.array_equal(c["ylim"][1:], [[3.7, 3.7], [0.0, 0.0]]) and np.all(c["hist"][:, 1:, :, 1:] == 0) and c["timing"]["degenerate"] == 2
    for r in (_pdm_device("n1"), ):
        assert np.all(r["explained"] == 0) and np.all(r["degenerate"] == 1) and np.all(r["nonempty"] == 1)
    one = _cent_device("n1")
    assert np.all(one["entropy"] == 0) and one["degenerate"][0] == 1 and one["hist"].sum() == 1
    R1 = L.pdm(np.array([2.0]), np.array([0.5]), np.array([1.0]), nbins=5, covers=2)
    assert R1.theta[0] == 1 and R1.aov is None and R1.degenerate[0] and R1.nonempty[0] == 2


def test_the_planted_period_is_found_by_all_three():
    import lpvspectral_jl_amd as L
    t, f, y = sawtooth_case()
    k0 = int(np.nonzero(f == 1.25)[0][0])
    P = L.pdm(y, t, f, nbins=10, covers=1)
    P2 = L.pdm(y, t, f, nbins=5, covers=2)
    A = L.aov(y, t, f, nbins=10)
    C = L.conditional_entropy(y, t, f, nbins=10, mbins=5)
    print(f"explained {P.explained[k0]:.3f} / {np.delete(P.explained, k0).max():.3f}, (5, 2) {P2.explained[k0]:.3f} / {np.delete(P2.explained, k0).max():.3f}, "
          f"H {C.entropy[k0]:.3f} / {np.delete(C.entropy, k0).min():.3f}")
    assert int(np.argmin(P.theta)) == k0 and int(np.argmin(P2.theta)) == k0 and int(np.argmax(A.aov)) == k0 and int(np.argmin(C.entropy)) == k0
    assert abs(P.explained[k0] - 0.566) < 0.03 and np.delete(P.explained, k0).max() < 0.1
    assert abs(P2.explained[k0] - 0.41) < 0.03 and np.delete(P2.explained, k0).max() < 0.06
    assert C.entropy[k0] < 1.0 and np.delete(C.entropy, k0).min() > 1.2


# ---- the Python surface and the refusals ---------------------------------------------------------------------------------------------------
def test_the_python_surface():
    import lpvspectral_jl_amd as L
    import torch
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES["n255w"]
    t, f, y, W = _pdm_inputs("n255w")
    d = _pdm_device("n255w")
    R = L.pdm(y, t, f, W=W, nbins=nbins, covers=covers, center_data=center, return_hist=True)
    assert isinstance(R, L.PDM) and R.explained.shape == (70, 3) and np.array_equal(R.explained, d["explained"]) and np.array_equal(R.nonempty, d["nonempty"])
    assert np.array_equal(R.hist, d["hist"]) and np.array_equal(R.hcount, d["hcount"]) and R.degenerate.dtype == bool and R.aov is None
    assert (R.nbins, R.covers) == (nbins, covers) and np.array_equal(R.f, f)
    assert np.array_equal(R.theta, theta_of(d["explained"], d["nonempty"], N, covers, d["degenerate"]))
    t1, f1, y1, _ = _pdm_inputs("base10")
    A = L.aov(y1, t1, f1)
    d1 = _pdm_device("base10")
    assert A.aov.shape == (70,) and A.hist is None and np.array_equal(A.explained, d1["explained"][:, 0]) and A.covers == 1
    assert np.array_equal(A.aov, aov_of(d1["explained"], d1["nonempty"], len(t1), d1["degenerate"])[:, 0])
    assert np.array_equal(L.pdm(y1, t1, f1).aov, A.aov) and L.pdm_last_timing()["F"] == 1
    At = L.aov(torch.as_tensor(y1, device="cuda"), torch.as_tensor(t1, device="cuda"), f1)
    assert np.array_equal(At.aov, A.aov) and np.array_equal(At.theta, A.theta)
    with pytest.raises(ValueError, match=r"aov: covers must be 1, got 2"):
        L.aov(y1, t1, f1, covers=2)
    N, Nf, nbins, mbins, ns, plan = CENT_CASES["n255f4"]
    t, f, y = _cent_inputs("n255f4")
    c = _cent_device("n255f4")
    C = L.conditional_entropy(y, t, f, nbins=nbins, mbins=mbins, return_hist=True)
    assert isinstance(C, L.CE) and C.entropy.shape == (1030, 3) and np.array_equal(C.entropy, c["entropy"]) and np.array_equal(C.hist, c["hist"])
    assert np.array_equal(C.ylim, c["ylim"]) and C.degenerate.dtype == bool and not C.degenerate.any() and L.cent_last_timing()["copies"] == 1
    C1 = L.conditional_entropy(torch.as_tensor(y[:, 1], device="cuda"), torch.as_tensor(t, device="cuda"), f, nbins=nbins, mbins=mbins)
    assert C1.entropy.shape == (1030,) and np.array_equal(C1.entropy, c["entropy"][:, 1]) and C1.ylim.shape == (2,) and C1.degenerate is False and C1.hist is None


def test_argument_errors_raise_value_error_with_the_message():
    import lpvspectral_jl_amd as L
    t, f, y, W = _pdm_inputs("base10")
    f = f[:4]
    for nb in (1, 0):
        with pytest.raises(ValueError, match=rf"pdm: nbins must be at least 2, got {nb}"):
            L.pdm(y, t, f, nbins=nb)
    with pytest.raises(ValueError, match=r"pdm: covers must be at least 1, got 0"):
        L.pdm(y, t, f, covers=0)
    with pytest.raises(ValueError, match=r"pdm: nbins covers must lie in 2 \.\. 2048, got 1025 x 2"):
        L.pdm(y, t, f, nbins=1025, covers=2, return_hist=True)
    with pytest.raises(ValueError, match=r"conditional_entropy: nbins must lie in 2 \.\. 256, got 257"):
        L.conditional_entropy(y, t, f, nbins=257)
    with pytest.raises(ValueError, match=r"conditional_entropy: mbins must lie in 2 \.\. 64, got 1"):
        L.conditional_entropy(y, t, f, mbins=1)
    with pytest.raises(ValueError, match=r"conditional_entropy: nbins mbins must be at most 8192, got 256 x 64"):
        L.conditional_entropy(y, t, f, nbins=256, mbins=64, return_hist=True)
    for who, call in (("pdm", L.pdm), ("conditional_entropy", L.conditional_entropy)):
        with pytest.raises(ValueError, match=rf"{who}: a frequency is not finite"):
            call(y, t, np.array([1.0, np.inf]))
        for bad in (0.0, -1.0):
            with pytest.raises(ValueError, match=rf"{who}: frequency 1 is not positive"):
                call(y, t, np.array([1.0, bad]))
        with pytest.raises(ValueError, match=r"y has 1500 samples, t has 1499"):
            call(y, t[:-1], f)
    with pytest.raises(ValueError, match=r"y has 1500 samples, W has 3"):
        L.pdm(y, t, f, W=np.ones(3))


N_REC, NS_REC = 600, 2
NOT_FINITE = "{}: t, y or W holds a value that is not finite"
ENTRY = {
    "pdm": (lambda L, t, y, W: L.pdm(y, t, np.arange(16, 48) / 64.0, W=W, nbins=5, covers=2), "pdm", True),
    "aov": (lambda L, t, y, W: L.aov(y, t, np.arange(16, 48) / 64.0, W=W), "pdm", True),
    "conditional_entropy": (lambda L, t, y, W: L.conditional_entropy(y, t, np.arange(16, 48) / 64.0), "conditional_entropy", False),
}


def _nan_in_t(t, y, W):
    t[N_REC - 1] = np.nan


def _inf_in_y(t, y, W):
    y[0, 1] = np.inf


def _nan_in_w(t, y, W):
    W[300] = np.nan


def _negative_weight(t, y, W):
    W[599] = -0.5


def _zero_weights(t, y, W):
    W[:] = 0.0


def _nan_and_negative_weight(t, y, W):
    W[0] = -1.0
    y[N_REC - 1, 1] = np.nan


# fault -> (what it does to the record, the message, whether it is a fault of the weights alone)
FAULTS = {
    "nan-in-t-at-599": (_nan_in_t, NOT_FINITE, False),
    "inf-in-second-signal-at-0": (_inf_in_y, NOT_FINITE, False),
    "nan-in-W": (_nan_in_w, NOT_FINITE, True),
    "negative-weight": (_negative_weight, "{}: a weight is negative", True),
    "zero-weights": (_zero_weights, "{}: the weights sum to 0", True),
    "nan-and-negative-weight": (_nan_and_negative_weight, NOT_FINITE, False),
}


@pytest.mark.parametrize("entry,fault", [(e, k) for e in ENTRY for k in FAULTS])
def test_record_refusals(L, entry, fault):
    """In the manner of tests/test_gpu_record_refusals.py: the exception type and the WHOLE message.  conditional_entropy takes no W, so a
    fault of the weights alone does not reach it: the record is taken."""
    call, prefix, weighted = ENTRY[entry]
    spoil, message, weights_only = FAULTS[fault]
    rng = np.random.default_rng(600)
    t = np.sort(rng.integers(0, 40 * 1024, N_REC)) / 1024.0
    y = np.cos(2 * np.pi * 1.25 * t[:, None] + np.arange(NS_REC)[None, :]) + 0.5 * rng.standard_normal((N_REC, NS_REC)) + 0.75
    W = rng.uniform(0.5, 2.0, N_REC)
    call(L, t, y, W)                                                           # the record itself is taken
    spoil(t, y, W)
    if weights_only and not weighted:
        assert np.all(np.isfinite(call(L, t, y, W).entropy))
        return
    with pytest.raises(ValueError) as e:
        call(L, t, y, W)
    assert str(e.value) == message.format(prefix)


# ---- no result depends on what a reused device block held ----------------------------------------------------------------------------------
def _pool_pdm(L, mp):
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES["n255w"]
    t, f, y, W = _pdm_inputs("n255w")
    r = L.pdm(y, t, f, W=W, nbins=nbins, covers=covers, center_data=center, return_hist=True)
    tm = L.pdm_last_timing()
    assert (tm["F"], tm["ts"], tm["passes"]) == plan
    return r, tm


def _pool_cent(L, mp):
    N, Nf, nbins, mbins, ns, plan = CENT_CASES["cells400"]
    t, f, y = _cent_inputs("cells400")
    r = L.conditional_entropy(y, t, f[:300], nbins=nbins, mbins=mbins, return_hist=True)
    return r, L.cent_last_timing()


@pytest.mark.parametrize("case", [_pool_pdm, _pool_cent])
def test_same_bytes_whatever_the_block_held(L, monkeypatch, case):
    """One pdm and one conditional_entropy call with LPVS_POOL_FILL unset / 00 / ff / 55: byte-equal, by the helper of
    tests/test_gpu_pool_fill.py."""
    from test_gpu_pool_fill import same_bytes_whatever_the_block_held
    same_bytes_whatever_the_block_held(case, L, monkeypatch)
