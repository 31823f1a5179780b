"""bls on the GPU against tests/_bls_ref.py: bls_model (the definition as the device computes it: integers exactly, doubles to 4 ulp) and
bls_ref_ld (the definition in long double: within the bounds derived in tests/_bls_ref.py, proven on the host by
tests/test_bls_ref_host.py).

INPUTS follow the family: t in multiples of 2^-10 (below 2^9), f in multiples of 2^-6, so f t, the fold and the bin are exact for any
nbins and the reference is unambiguous; the base case of tests/_bls_ref.py: base_case (1500 samples over 375 units, 70 frequencies in
[1/4, 2.41], noise of sigma 1/4, a dip of depth 0.5 and q = 0.05 at f = 1.25 that straddles phase 0).  One case more has generic doubles.

SHAPES: N in {255, 256, 257, 1500, 3000}; Nf in {1, 70, 1030} -- with nbins and the weights they reach every F in {1, 2, 4} and every
TS in {1, 2, 4} the plan can pick, asserted from the timing record --; nbins in {8, 64, 100, 2048}; widths 1 .. 1, 2 .. 12 and
1 .. nbins / 2; ns in {1, 3, 5}; with and without W; center_data on and off; both normalisations.

NEAR-TIES.  A (frequency, signal) whose model gap -- best objective against the best one of a box with other integer sums -- is at most
8 ulp need not return the model's box (the device's quotients may differ from numpy's in the last place).  There the device's box,
evaluated by the long-double reference, must lie within 2 B of the reference's maximum (B bounds the objective of EVERY box, so a box
that is best for one is within 2 B of the other's best), and its power, depth and depth_err are held to the reference's values of THAT
box.  At most 2 frequencies per case may hold a near-tie: asserted on the inputs (they hold none).

COMPLEMENT TIES (tests/_bls_ref.py: complement_case, half_case).  With dips_only = False a box and its complement -- the sums (R - r, S - s)
-- have the same objective BIT FOR BIT: the two quotients change places and their sum commutes.  That is an exact tie, which the rule
decides (narrowest, then earliest), not a near-tie; so for these cases a frequency is clear when the model's SECOND gap (gap2: the boxes
with the complement's sums set aside as well) exceeds 8 ulp, and the exemption above stays for the others, with its cap of 2.  The
library takes widths up to nbins / 2, so the complements that are searched are those of the boxes of width nbins / 2 (the model with
every width up to nbins - 1 has gap 0 at all 70 frequencies and the same winners, tests/test_bls_ref_host.py); the "half" record makes
such a box the maximum at f = 1 for nbins in {8, 64, 128, 256, 512}."""
import functools

import numpy as np
import pytest

from _bls_ref import (COMPLEMENT_NBINS, HALF_K, LD, base_case, bls_bounds, bls_model, bls_ref_ld, complement_case, device_moments, fold_bins, half_case, ld_bins,
                      ref_at_box)

pytestmark = pytest.mark.gpu

# name -> (N, Nf, nbins, kmin, kmax, ns, weighted, center_data, normalization, dips_only, (F, TS, passes))
CASES = {
    "base64": (1500, 70, 64, 1, 8, 1, False, True, "standard", True, (1, 1, 1)),
    "base100w": (1500, 70, 100, 2, 12, 1, True, True, "chi2", True, (1, 1, 1)),
    "n255": (255, 70, 8, 1, 4, 3, True, False, "standard", True, (1, 4, 1)),
    "n256": (256, 70, 64, 1, 32, 5, False, True, "chi2", True, (1, 4, 2)),
    "n257": (257, 70, 100, 1, 1, 1, True, True, "standard", False, (1, 1, 1)),
    "n3000": (3000, 70, 2048, 2, 12, 1, True, True, "standard", True, (1, 1, 1)),
    "one": (1500, 1, 64, 2, 12, 1, False, True, "standard", True, (1, 1, 1)),
    "f4": (1500, 1030, 64, 2, 12, 1, False, True, "standard", True, (4, 1, 1)),
    "f2": (1500, 1030, 2048, 2, 6, 1, False, False, "standard", False, (2, 1, 1)),
    "ts2": (1500, 70, 2048, 2, 12, 3, True, True, "standard", True, (1, 2, 2)),
    "f4w": (1500, 1030, 8, 1, 4, 3, True, True, "chi2", True, (4, 4, 1)),
}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    N, Nf, nbins, kmin, kmax, ns, weighted, center, norm, dips, plan = CASES[name]
    t, f, y = base_case(seed=0, N=N, span=375.0 if N >= 1000 else 64.0, Nf=70, ns=ns)
    if Nf == 1:
        f = f[32:33]
    elif Nf != 70:
        f = 0.25 + np.arange(Nf) / 64.0
    W = None
    if weighted:
        W = 0.5 + np.random.default_rng(100 + N).random(N)
    return t, f, y, W


@functools.lru_cache(maxsize=None)
def _model(name):
    N, Nf, nbins, kmin, kmax, ns, weighted, center, norm, dips, plan = CASES[name]
    t, f, y, W = _inputs(name)
    kw = dict(nbins=nbins, kmin=kmin, kmax=kmax, min_count=1, dips_only=dips, center_data=center, normalization=norm)
    return bls_model(y, t, f, W, **kw), bls_ref_ld(y, t, f, W, **kw), kw


def _raw(y, t, f, W, nbins, kmin, kmax, min_count=1, dips_only=True, center_data=True, normalization="standard", device_out=False):
    """lpvs_bls_f64 itself, with the widths given in bins.  -> dict of (Nf, ns) arrays and the histograms.  device_out: power_out,
    depth_out and depth_err_out are device memory (torch tensors), read back afterwards."""
    import lpvspectral_jl_amd as L
    from lpvspectral_jl_amd._lib import check, lib, out_ptr
    y = np.asfortranarray(np.asarray(y, np.float64).reshape(len(t), -1))
    N, ns = y.shape
    f = np.ascontiguousarray(f, dtype=np.float64)
    Nf = len(f)
    k0 = np.ascontiguousarray(np.broadcast_to(np.asarray(kmin, np.int32), (Nf,)))
    k1 = np.ascontiguousarray(np.broadcast_to(np.asarray(kmax, np.int32), (Nf,)))
    t = np.ascontiguousarray(t, dtype=np.float64)
    Wa = None if W is None else np.ascontiguousarray(W, dtype=np.float64)
    dbl, ints, cnt = np.zeros((3, ns, Nf)), np.zeros((3, ns, Nf), np.int32), np.zeros((ns, Nf), np.int64)
    hist, hcount = np.zeros((Nf, 1 + ns, max(nbins, 1)), np.int64), np.zeros((Nf, max(nbins, 1)), np.int32)
    planes = [out_ptr(dbl[i]) for i in range(3)]
    if device_out:
        import ctypes
        import torch
        dev = torch.full((3, ns, Nf), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        planes = [ctypes.c_void_p(dev[i].data_ptr()) for i in range(3)]
    check(lib().lpvs_bls_f64(out_ptr(y), ns, out_ptr(t), N, None if Wa is None else out_ptr(Wa), out_ptr(f), Nf, nbins, out_ptr(k0), out_ptr(k1), min_count,
                             int(dips_only), int(center_data), {"standard": 0, "chi2": 1}.get(normalization, normalization), 0, planes[0], planes[1],
                             planes[2], out_ptr(ints[0]), out_ptr(ints[1]), out_ptr(cnt), out_ptr(ints[2]), out_ptr(hist), out_ptr(hcount)))
    if device_out:
        dbl = dev.cpu().numpy()
    return dict(power=dbl[0].T, depth=dbl[1].T, depth_err=dbl[2].T, start=ints[0].T, width=ints[1].T, degenerate=ints[2].T, count=cnt.T, hist=hist,
                hcount=hcount, timing=L.bls_last_timing())


@functools.lru_cache(maxsize=None)
def _device(name):
    t, f, y, W = _inputs(name)
    return _raw(y, t, f, W, **_model(name)[2])


def _bits(r):
    return tuple(np.ascontiguousarray(r[k]).tobytes() for k in ("power", "depth", "depth_err", "start", "width", "degenerate", "count", "hist", "hcount"))


def _within_ulp(a, b, n=4):
    return np.all(np.abs(a - b) <= n * np.spacing(np.abs(b)))


WORST = {}


def _check_against_refs(name, d, m, r, t, f, y, W, kw, gap="gap"):
    """The assertions of one case (module docstring).  gap: the model's gap that says where a near-tie is ("gap2" for the complement ties)."""
    Nf, ns = m["power"].shape
    assert np.array_equal(d["hist"], m["hist"]), "the integer histograms"
    assert np.array_equal(d["hcount"], m["hcount"]), "the counts per bin"
    assert d["timing"]["degenerate"] == m["ndeg"] == int(d["degenerate"].sum())
    assert np.array_equal(d["degenerate"] != 0, m["degenerate"] != 0)
    for key in ("power", "depth", "depth_err"):
        assert np.all(np.isfinite(d[key])), key
    near = m[gap] <= 8
    assert near.any(axis=1).sum() <= 2, f"{near.any(axis=1).sum()} frequencies with a near-tie in the inputs of {name}"
    clear = ~near
    for key in ("start", "width", "count"):
        assert np.array_equal(d[key][clear], m[key][clear]), key
    same = clear | ((d["start"] == m["start"]) & (d["width"] == m["width"]))
    for key in ("power", "depth", "depth_err"):
        assert _within_ulp(d[key][same], m[key][same]), f"{key}: more than 4 ulp from the model"
    # ... and the long-double definition, within the derived bounds
    bd = bls_bounds(y, W, kw["center_data"], m["shy"])
    live = d["degenerate"] == 0
    for c in range(ns):
        for k in np.nonzero(live[:, c])[0]:
            if d["start"][k, c] == r["start"][k, c] and d["width"][k, c] == r["width"][k, c]:
                ref = {key: r[key][k, c] for key in ("power", "depth", "depth_err", "r", "rc")}
            else:                                                              # another box: the reference's values of THAT box, and its objective against the best
                one = bls_ref_ld(y.reshape(len(t), -1)[:, c], t, f[k:k + 1], W, keep_table=True, **kw)
                ref = ref_at_box(one, d["width"][k, c], d["start"][k, c], kw["normalization"])
                assert ref["valid"] and ref["delta"] >= one["delta"][0, 0] - 2 * bd.B[c], f"{name}: the box at frequency {k}, signal {c} is not a best box"
            for key, b in (("power", bd.power(c, ref["power"], kw["normalization"])), ("depth", bd.depth(c, ref["r"], ref["rc"])),
                           ("depth_err", bd.depth_err_rel(ref["r"], ref["rc"]) * ref["depth_err"])):
                e = abs(LD(d[key][k, c]) - ref[key])
                WORST[key] = max(WORST.get(key, 0.0), float(e / b))
                assert e <= b, f"{name} {key} at frequency {k}, signal {c}: {float(e):.3e} > {float(b):.3e}"


@pytest.mark.parametrize("name", list(CASES))
def test_every_shape_against_the_model_and_the_long_double_definition(name):
    m, r, kw = _model(name)
    d = _device(name)
    t, f, y, W = _inputs(name)
    F, TS, passes = CASES[name][10]
    tm = d["timing"]
    assert (tm["F"], tm["ts"], tm["passes"]) == (F, TS, passes), tm
    assert tm["unit"] == (W is None) and tm["nf"] == len(f) and tm["boxes"] == len(f) * kw["nbins"] * (kw["kmax"] - kw["kmin"] + 1)
    live_shy = [s for s in m["shy"]]
    assert (tm["shift_y_min"], tm["shift_y_max"]) == (min(live_shy), max(live_shy)) and tm["shift_w"] == (0 if W is None else 60)
    _check_against_refs(name, d, m, r, t, f, y, W, kw)
    print(f"{name}: worst error / bound so far {WORST}")


# ---- complement ties ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _complement(record, nbins, weighted):
    t, f, y, W = (complement_case if record == "base" else half_case)(weighted)
    kw = dict(nbins=nbins, kmin=1, kmax=nbins // 2, min_count=1, dips_only=False, center_data=True, normalization="standard")
    return (t, f, y, W), kw, bls_model(y, t, f, W, **kw), bls_ref_ld(y, t, f, W, **kw)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nbins", COMPLEMENT_NBINS)
@pytest.mark.parametrize("record", ["base", "half"])
def test_a_box_and_its_complement_tie_and_the_rule_decides(record, nbins, weighted):
    """dips_only = False and every width the library takes, 1 .. nbins / 2 (module docstring, NEAR-TIES): the boxes of width nbins / 2
    have their complements among the boxes searched, nbins / 2 starts further on -- in the same wave (nbins 8, 64), the next one (128),
    two waves on (256), the same thread's next stride (512) -- with bit-equal objectives.  On the "half" record that tie is the
    maximum at f = 1, and the earlier start the only right answer."""
    (t, f, y, W), kw, m, r = _complement(record, nbins, weighted)
    d = _raw(y, t, f, W, **kw)
    assert d["timing"]["boxes"] == len(f) * nbins * (nbins // 2)
    clear = m["gap2"] > 8
    print(f"{record} nbins {nbins} W={weighted}: {int((m['gap'] == 0).sum())} of {len(f)} frequencies with an exact tie at the maximum, "
          f"{int((~clear).sum())} near-ties, widest box {int(d['width'].max())}")
    for key in ("start", "width", "count"):
        assert np.array_equal(d[key][clear], m[key][clear]), key
    assert np.all(d["width"] <= nbins // 2)
    _check_against_refs(f"{record}{nbins}", d, m, r, t, f, y, W, kw, gap="gap2")
    if record == "half":
        k = HALF_K
        assert m["gap"][k, 0] == 0 and clear[k, 0]
        assert (d["start"][k, 0], d["width"][k, 0], d["count"][k, 0]) == (nbins // 4, nbins // 2, 256) and d["depth"][k, 0] > 1.9


def test_the_planted_dip_is_found_and_wraps():
    t, f, y, W = _inputs("base64")
    for name, box in (("base64", (62, 3)), ("base100w", (97, 5))):
        d = _device(name)
        k = int(np.argmax(d["power"][:, 0]))
        assert f[k] == 1.25 and (d["start"][k, 0], d["width"][k, 0]) == box
        assert abs(d["depth"][k, 0] - 0.5) < 0.1


def test_the_python_surface():
    import lpvspectral_jl_amd as L
    t, f, y, W = _inputs("base100w")
    R = L.bls(y, t, f, W=W, nbins=100, q=(0.02, 0.12), normalization="chi2", return_hist=True)
    d = _device("base100w")
    assert R.power.shape == (70,) and np.array_equal(R.power, d["power"][:, 0]) and np.array_equal(R.start, d["start"][:, 0])
    assert np.array_equal(R.hist, d["hist"]) and np.array_equal(R.hcount, d["hcount"]) and R.degenerate.dtype == bool
    assert np.array_equal(R.q, R.width / 100.0) and np.array_equal(R.duration, R.q / f)
    assert np.array_equal(R.transit_time, (R.start + R.width / 2.0) / 100.0 / f) and np.array_equal(R.snr, R.depth / R.depth_err)
    k = int(np.argmax(R.power))
    assert abs(R.power[k] - R.snr[k] ** 2) < 1e-6 * R.power[k]                  # chi2 = snr^2 up to the weights' total (R = 1 up to 2^-41)
    # duration: the widths per frequency, q = d f
    R2 = L.bls(y, t, f[32:34], W=W, nbins=100, duration=(0.021 / f[32], 0.119 / f[32]), normalization="chi2")
    assert R2.power[0] == R.power[32] and R2.power.shape == (2,)
    g = L.bls_frequencies(t, 0.25, 2.5, 0.05, oversample=3)
    span = t.max() - t.min()
    assert g[0] == 0.25 and g[-1] <= 2.5 and np.allclose(np.diff(g), 0.05 / (3 * span), rtol=1e-9, atol=0) and g[-1] + 0.05 / (3 * span) > 2.5
    Y5 = base_case(seed=0, ns=5)[2]
    R5 = L.bls(Y5, t, f, nbins=64, q=(1 / 64, 8 / 64))
    assert R5.power.shape == (70, 5) and R5.hist is None
    import torch
    Rt = L.bls(torch.as_tensor(Y5, device="cuda"), torch.as_tensor(t, device="cuda"), f, nbins=64, q=(1 / 64, 8 / 64))
    assert np.array_equal(Rt.power, R5.power) and np.array_equal(Rt.start, R5.start)


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    t, f, y, W = _inputs("ts2")
    assert _bits(_raw(y, t, f, W, **_model("ts2")[2])) == _bits(_device("ts2"))


def test_a_frequency_has_the_same_bits_alone_among_others_and_permuted_whatever_f_is():
    t, f, y, W = _inputs("f4")
    kw = _model("f4")[2]
    full = _device("f4")                                                       # F = 4
    perm = np.random.default_rng(5).permutation(len(f))
    p = _raw(y, t, f[perm], W, **kw)                                           # F = 4, other neighbours
    assert p["timing"]["F"] == 4
    for key in ("power", "depth", "depth_err", "start", "width", "count", "degenerate", "hist", "hcount"):
        assert np.array_equal(p[key], full[key][perm]), key
    for k in (0, 37, 515, 1029):
        a = _raw(y, t, f[k:k + 1], W, **kw)                                    # alone: F = 1
        assert a["timing"]["F"] == 1
        for key in ("power", "depth", "depth_err", "start", "width", "count", "degenerate", "hist", "hcount"):
            assert np.array_equal(a[key][0], full[key][k]), (k, key)
    few = _raw(y, t, f[500:570], W, **kw)                                      # 70 of them: F = 1
    assert few["timing"]["F"] == 1 and np.array_equal(few["power"], full["power"][500:570]) and np.array_equal(few["hist"], full["hist"][500:570])


def test_a_signal_has_the_same_bits_alone_and_among_five():
    t, f, y, W = _inputs("n256")
    kw = _model("n256")[2]
    five = _device("n256")
    for c in (0, 3, 4):
        a = _raw(y[:, c], t, f, W, **kw)
        for key in ("power", "depth", "depth_err", "start", "width", "count", "degenerate"):
            assert np.array_equal(a[key][:, 0], five[key][:, c]), (c, key)
        assert np.array_equal(a["hist"][:, 1], five["hist"][:, 1 + c])


@pytest.mark.parametrize("normalization", ["standard", "chi2"])
def test_a_permutation_of_the_samples_changes_no_bit(normalization):
    """W = None and center_data = False: nothing is summed in floating point before the quantisation, the integer atomics make the
    histograms independent of the order of the samples, and YY -- the divisor of the standard power -- is an integer sum of its terms
    too.  The inputs are chosen so that a floating-point YY WOULD change: the tree sum of the moment kernels (tests/_bls_ref.py:
    device_moments) has other bits for the permuted record, asserted here."""
    t, f, y = base_case(seed=2)
    perm = np.random.default_rng(0).permutation(len(t))
    tree = [device_moments(v.reshape(-1, 1), None, False)[4][0] for v in (y, y[perm])]
    assert tree[0] != tree[1], "the inputs do not show the property: a tree sum of YY has the same bits in both orders"
    kw = dict(nbins=100, kmin=2, kmax=12, dips_only=True, center_data=False, normalization=normalization)
    a, b = _raw(y, t, f, None, **kw), _raw(y[perm], t[perm], f, None, **kw)
    assert _bits(a) == _bits(b) and a["timing"]["degenerate"] == 0 and np.all(a["power"] > 0)
    m = bls_model(y, t, f, None, **kw)
    assert np.array_equal(a["start"], m["start"]) and _within_ulp(a["power"], m["power"])


def test_the_planes_may_be_device_memory():
    """power_out, depth_out and depth_err_out in device memory: the same bits as through the host staging."""
    t, f, y, W = _inputs("n255")
    kw = _model("n255")[2]
    assert _bits(_raw(y, t, f, W, device_out=True, **kw)) == _bits(_device("n255"))


# ---- generic doubles -----------------------------------------------------------------------------------------------------------------------
def test_generic_doubles_fold_by_the_exact_phase():
    """t and f random, not dyadic: f t is inexact and the bin hangs on its low word.  The seed is chosen so that no phi nbins lies within
    2^-30 of an integer (asserted): the device's phase -- (p - rint(p)) + e, within 2^-52 of the exact one -- then falls into the exact
    phase's bin, and the histograms have to be equal exactly."""
    rng = np.random.default_rng(3)
    N, Nf, nbins = 1500, 70, 100
    t = np.sort(rng.random(N) * 4000.0)
    f = np.sort(0.25 + 2.25 * rng.random(Nf))
    y = 0.25 * rng.standard_normal(N)
    y[np.mod(f[40] * t, 1.0) < 0.04] -= 0.5
    W = 0.5 + rng.random(N)
    bins_ld, phi = ld_bins(f, t, nbins)
    x = phi * LD(nbins)
    assert np.abs(x - np.rint(x)).min() > 2.0 ** -30
    assert np.array_equal(fold_bins(f, t, nbins)[0], bins_ld)
    kw = dict(nbins=nbins, kmin=2, kmax=12, min_count=1, dips_only=True, center_data=True, normalization="standard")
    m, r, d = bls_model(y, t, f, W, **kw), bls_ref_ld(y, t, f, W, **kw), _raw(y, t, f, W, **kw)
    _check_against_refs("generic", d, m, r, t, f, y, W, kw)
    assert int(np.argmax(d["power"][:, 0])) == 40


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------
def test_all_samples_in_one_bin_give_flagged_zeros():
    t = np.arange(300.0)
    y = np.random.default_rng(0).standard_normal(300)
    d = _raw(y, t, np.array([1.0, 2.0]), None, 64, 1, 8)
    assert np.all(d["hcount"][:, 0] == 300) and np.all(d["hcount"][:, 1:] == 0)
    for key in ("power", "depth", "depth_err", "start", "width", "count"):
        assert np.all(d[key] == 0), key
    assert np.all(d["degenerate"] == 1) and d["timing"]["degenerate"] == 2


def test_a_constant_signal_has_power_zero():
    t, f, y, W = _inputs("base100w")
    Y = np.stack([y, np.full(len(t), 3.7), np.zeros(len(t))], axis=1)
    for center in (True, False):
        d = _raw(Y, t, f, W, 100, 2, 12, center_data=center)
        assert np.all(np.isfinite(d["power"])) and np.all(d["power"][:, 2] == 0) and np.all(d["degenerate"][:, 2] == 1)
        if center:
            assert np.all(d["power"][:, 1] == 0) and np.all(d["degenerate"][:, 1] == 1) and np.array_equal(d["power"][:, 0], _raw(y, t, f, W, 100, 2, 12)["power"][:, 0])


def test_an_exact_noiseless_box_has_standard_power_one():
    t, f, y, W = _inputs("base64")
    ph = np.mod(1.25 * t, 1.0)
    yb = np.where((ph >= 60 / 64) | (ph < 2 / 64), -1.0, 0.0)                   # the bins 60 .. 63, 0, 1
    d = _raw(yb, t, f, None, 64, 1, 8)
    b = bls_bounds(yb, None, True, bls_model(yb, t, f[32:33], None, 64, 1, 8)["shy"])
    assert (d["start"][32, 0], d["width"][32, 0]) == (60, 6)
    assert abs(d["power"][32, 0] - 1.0) <= float(b.power(0, 1.0, "standard")) and d["power"][32, 0] <= 1.0
    assert abs(d["depth"][32, 0] - 1.0) <= float(b.depth(0, LD(d["count"][32, 0]) / len(t), 1 - LD(d["count"][32, 0]) / len(t)))


def test_argument_errors_raise_value_error_with_the_message():
    import lpvspectral_jl_amd as L
    t, f, y, W = _inputs("base100w")
    f = f[:4]
    for nb in (7, 2049):
        with pytest.raises(ValueError, match=rf"bls: nbins must lie in 8 \.\. 2048, got {nb}"):
            L.bls(y, t, f, nbins=nb)
    with pytest.raises(ValueError, match=r"bls: kmax of frequency 0 is 33, above nbins / 2 = 32"):
        _raw(y, t, f, W, 64, 1, 33)
    with pytest.raises(ValueError, match=r"bls: kmin of frequency 0 is 30, above its kmax 10"):
        L.bls(y, t, f, nbins=100, q=(0.3, 0.1))
    with pytest.raises(ValueError, match=r"bls: kmin of frequency 2 is 0, below 1"):
        _raw(y, t, f, W, 64, np.array([1, 1, 0, 1]), 8)
    tb = t.copy(); tb[7] = np.nan
    yb = y.copy(); yb[9] = np.inf
    Wb = W.copy(); Wb[3] = -np.inf
    for args in ((y, tb, f, W), (yb, t, f, W), (y, t, f, Wb)):
        with pytest.raises(ValueError, match=r"bls: t, y or W holds a value that is not finite"):
            L.bls(args[0], args[1], args[2], W=args[3])
    with pytest.raises(ValueError, match=r"bls: a frequency is not finite"):
        L.bls(y, t, np.array([1.0, np.inf]))
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match=r"bls: frequency 1 is not positive"):
            L.bls(y, t, np.array([1.0, bad]))
    Wn = W.copy(); Wn[5] = -1.0
    with pytest.raises(ValueError, match=r"bls: a weight is negative"):
        L.bls(y, t, f, W=Wn)
    with pytest.raises(ValueError, match=r"bls: the weights sum to 0"):
        L.bls(y, t, f, W=np.zeros(len(t)))
    with pytest.raises(ValueError, match=r"bls: min_count must be at least 1, got 0"):
        L.bls(y, t, f, min_count=0)
    with pytest.raises(ValueError, match=r"normalization: unknown value 'psd'"):
        L.bls(y, t, f, normalization="psd")
    with pytest.raises(ValueError, match=r"bls: normalization must be 0 \(standard\) or 1 \(chi2\), got 2"):
        _raw(y, t, f, W, 64, 1, 8, normalization=2)
    with pytest.raises(ValueError, match=r"y has 1500 samples, t has 1499"):
        L.bls(y, t[:-1], f)
