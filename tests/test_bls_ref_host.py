"""The references of bls (tests/_bls_ref.py) held to each other on the CPU, before the GPU tests lean on them: the model (the definition as
the device computes it, from 64-bit integers) against the definition in long double, within the bounds derived in tests/_bls_ref.py
(n / 2 quanta per sum, three roundings per wy, the error of the mean, to first order through Delta, depth and power; u = 2^-53, nothing
fitted); the planted box; dips_only; invariance under a shift of y and a scaling of W; binned against brute-force membership; the shift
rule at its limit.  CPU only."""
import numpy as np
import pytest

from _bls_ref import (COMPLEMENT_NBINS, HALF_K, LD, U, base_case, bls_bounds, bls_model, bls_ref_ld, complement_case, device_moments, device_sum, fold_bins,
                      half_case, ld_bins, order_free_yy, quantise, ref_at_box, shift_y)


def _compare(y, t, f, W, kw, m=None, r=None, y_ref=None, skip=()):
    """model against long double: same boxes (no near-tie in these inputs: asserted), every double within its bound.  -> worst ratios."""
    m = bls_model(y, t, f, W, **kw) if m is None else m
    r = bls_ref_ld(y if y_ref is None else y_ref, t, f, W, **kw) if r is None else r
    bd = bls_bounds(y, W, kw.get("center_data", True), m["shy"])
    assert (m["gap"] > 8).all()
    assert np.array_equal(m["start"], r["start"]) and np.array_equal(m["width"], r["width"]) and np.array_equal(m["count"], r["count"])
    assert np.array_equal(m["degenerate"], r["none"])
    worst = {}
    Nf, ns = m["power"].shape
    for c in range(ns):
        for k in range(Nf):
            if m["degenerate"][k, c]:
                continue
            rr, rc = r["r"][k, c], r["rc"][k, c]
            for key, b in (("power", bd.power(c, r["power"][k, c], kw.get("normalization", "standard"))), ("depth", bd.depth(c, rr, rc)),
                           ("depth_err", bd.depth_err_rel(rr, rc) * r["depth_err"][k, c])):
                if key in skip:
                    continue
                e = abs(LD(m[key][k, c]) - r[key][k, c])
                assert e <= b, f"{key} at frequency {k}, signal {c}: {float(e):.3e} > {float(b):.3e}"
                worst[key] = max(worst.get(key, 0.0), float(e / b))
    return worst


@pytest.mark.parametrize("nbins,kmin,kmax,weighted,center,norm,ns", [(64, 1, 8, False, True, "standard", 1), (100, 2, 12, True, True, "chi2", 1),
                                                                      (100, 2, 12, False, False, "standard", 3), (8, 1, 4, True, True, "standard", 3),
                                                                      (2048, 2, 12, True, True, "chi2", 1)])
def test_model_against_the_long_double_definition(nbins, kmin, kmax, weighted, center, norm, ns):
    t, f, y = base_case(ns=ns)
    W = 0.5 + np.random.default_rng(1).random(len(t)) if weighted else None
    worst = _compare(y, t, f, W, dict(nbins=nbins, kmin=kmin, kmax=kmax, center_data=center, normalization=norm))
    assert worst and max(worst.values()) < 1.0


def test_the_planted_box_is_the_global_maximum_and_wraps():
    t, f, y = base_case()
    for nbins, (k0, k1), box in ((64, (1, 8), (62, 3)), (100, (2, 12), (97, 5))):
        for res in (bls_model(y, t, f, None, nbins, k0, k1), bls_ref_ld(y, t, f, None, nbins, k0, k1)):
            k = int(np.argmax(res["power"][:, 0]))
            assert f[k] == 1.25 and (res["start"][k, 0], res["width"][k, 0]) == box
            assert abs(float(res["depth"][k, 0]) - 0.5) < 0.1
    # at 100 bins the box IS the planted bins: its count is the number of planted samples
    ph = np.mod(1.25 * t, 1.0)
    assert bls_model(y, t, f, None, 100, 2, 12)["count"][32, 0] == int(((ph >= 0.97) | (ph < 0.02)).sum())


def test_dips_only_hides_a_bump():
    t, f, y = base_case(bump=True)
    hidden, shown = bls_model(y, t, f, None, 100, 2, 12, dips_only=True), bls_model(y, t, f, None, 100, 2, 12, dips_only=False)
    k = int(np.argmax(shown["power"][:, 0]))
    assert f[k] == 1.25 and (shown["start"][k, 0], shown["width"][k, 0]) == (97, 5) and shown["depth"][k, 0] < -0.4
    assert int(np.argmax(hidden["power"][:, 0])) != k or (hidden["start"][k, 0], hidden["width"][k, 0]) != (97, 5)
    assert hidden["power"][32, 0] < 0.5 * shown["power"][32, 0] and (hidden["depth"] >= 0).all()
    r = bls_ref_ld(y, t, f, None, 100, 2, 12, dips_only=False)
    assert (r["start"][32, 0], r["width"][32, 0]) == (97, 5)


def test_a_shift_of_y_and_a_scaling_of_w_change_nothing_beyond_the_bound():
    t, f, y = base_case()
    W = 0.5 + np.random.default_rng(1).random(len(t))
    kw = dict(nbins=100, kmin=2, kmax=12)
    r = bls_ref_ld(y, t, f, W, **kw)
    # y + 10^6: the mean's error grows with sum w |y| and the bound with it (em); the long-double reference of the UNSHIFTED record is
    # the truth for both (its own error, 2^-64 of 10^6 per term, is 2^-11 of that bound)
    big = _compare(y + 1e6, t, f, W, kw, r=r)
    same = _compare(y, t, f, 3.0 * W, kw, r=r, skip=("depth_err",))             # (depth_err is that of the weights: 1 / sqrt(3) of it, below)
    assert max(big.values()) < 1.0 and max(same.values()) < 1.0
    assert float(bls_bounds(y + 1e6, W, True, [60]).em[0]) > 1e5 * float(bls_bounds(y, W, True, [60]).em[0])
    # the chi2 power scales with W, nothing else does
    a, b = bls_model(y, t, f, W, normalization="chi2", **kw), bls_model(y, t, f, 3.0 * W, normalization="chi2", **kw)
    assert np.allclose(b["power"], 3.0 * a["power"], rtol=1e-9) and np.allclose(b["depth"], a["depth"], rtol=1e-9)
    assert np.allclose(b["depth_err"] * np.sqrt(3.0), a["depth_err"], rtol=1e-12) and np.array_equal(a["start"], b["start"])


def test_binned_membership_is_brute_force_membership():
    """On the exact family a sample is in the box (k, b) iff its exact phase lies in [b / nbins, (b + k) / nbins) modulo 1: the sums of
    the model's integer histograms equal the sums over the samples picked that way."""
    t, f, y = base_case()
    N = len(t)
    sumW, w, mean, wy, YY, Rg = device_moments(y.reshape(N, 1), None, True)
    sh = shift_y(np.abs(wy).max(), N)
    qy = quantise(wy[0], sh)
    for nbins in (64, 100, 7 * 13):
        m = bls_model(y, t, f, None, nbins, 1, nbins // 2)
        bins, x = fold_bins(f, t, nbins)
        assert np.array_equal(bins, ld_bins(f, t, nbins)[0])
        rng = np.random.default_rng(nbins)
        for _ in range(40):
            k, b, width = rng.integers(len(f)), rng.integers(nbins), rng.integers(1, nbins // 2 + 1)
            phase = np.mod(LD(f[k]) * t.astype(LD), 1)                         # exact: 22 bits at most
            rel = np.mod(phase - LD(b) / nbins, 1)
            inside = rel < LD(width) / nbins
            sel = np.mod(bins[k] - b, nbins) < width
            assert np.array_equal(inside, sel)
            h = np.concatenate([m["hist"][k, 1], m["hist"][k, 1]])[b:b + width].sum()
            assert h == qy[inside].sum() and np.concatenate([m["hcount"][k]] * 2)[b:b + width].sum() == inside.sum()


def test_the_shift_rule_cannot_overflow():
    """2^24 samples all equal to the largest: their quantised sum, and the difference of two such sums, stay inside 63 bits."""
    N = 1 << 24
    for A in (1.0, 0.999, 1.9999999, 3e-310, 1e300, 2.0 ** -10):
        sh = shift_y(A, N)
        q = int(quantise(np.array([A]), sh)[0])
        assert 2 ** 36 <= q <= 2 ** 37 and N * q <= 2 ** 61 and 2 * N * q < 2 ** 63
        assert int(np.int64(N * q)) == N * q
    Nmax = 1 << 30
    q = int(quantise(np.array([1.9999999]), shift_y(1.9999999, Nmax))[0])
    assert Nmax * q <= 2 ** 61
    w = int(quantise(np.array([1.0 / 3]), 60)[0])
    assert 3 * w <= 2 ** 60 + 2


def test_the_order_free_yy_is_order_free_where_the_tree_sum_is_not():
    """order_free_yy (csrc/bls_plan.h: bls_yy_words, bls_yy): the same bits under permutations that change the tree sum, and within 2 u of
    the exact sum of the rounded terms (the tree sum: within (N + 16) u)."""
    t, f, y = base_case(seed=2)
    N = len(t)
    v = (y / N) * y
    exact = float(v.astype(LD).sum())
    trees, frees = set(), set()
    for p in range(8):
        perm = np.random.default_rng(p).permutation(N)
        trees.add(device_sum(v[perm])); frees.add(order_free_yy(v[perm], N))
    assert len(frees) == 1 and len(trees) > 1
    assert abs(frees.pop() - exact) <= 2 * U * exact and all(abs(x - exact) <= (N + 16) * U * exact for x in trees)
    assert order_free_yy(np.zeros(5), 5) == 0.0 and order_free_yy(np.array([1.0, np.inf]), 2) == np.inf
    assert order_free_yy(np.full(1 << 12, 0.1), 1 << 12) == float(LD(0.1) * 4096)
    bm = bls_model(y, t, f[:3], None, 64, 1, 8, center_data=False)
    assert bm["YY"][0] == order_free_yy((y / N) * y, N) and abs(bm["YY"][0] - bm["YY_tree"][0]) <= (N + 16) * U * exact


def test_the_reference_evaluates_any_box():
    """ref_at_box at the reference's own best box gives the reference's values; at another box a smaller objective."""
    t, f, y = base_case()
    one = bls_ref_ld(y, t, f[32:33], None, 100, 2, 12, keep_table=True)
    at = ref_at_box(one, one["width"][0, 0], one["start"][0, 0])
    assert at["valid"] and all(at[k] == one[k][0, 0] for k in ("power", "depth", "depth_err", "r", "rc")) and at["delta"] == one["delta"][0, 0]
    other = ref_at_box(one, 4, 97)
    assert other["valid"] and other["delta"] < at["delta"] and other["r"] < at["r"] and 0 < other["power"] < at["power"]


def test_device_sum_is_the_fixed_tree():
    """device_sum restates the moment kernels' order: slabs of 256 by a halving tree, then the slabs t, t + 256, ... and the same tree."""
    x = np.random.default_rng(0).standard_normal(70000)
    assert abs(device_sum(x) - float(x.astype(LD).sum())) <= 40 * U * np.abs(x).sum()
    assert device_sum(np.ones(1500)) == 1500.0 and device_sum(np.arange(300.0)) == 44850.0
    a = np.zeros(512); a[0], a[1], a[128], a[256] = 1.0, 2.0 ** -53, 2.0 ** -53, 2.0 ** -53
    # (1 + 2^-53 a[128]) first: the tree pairs i with i + 128, so 1 + 2^-53 rounds to 1, and again with a[1]; slab 1 joins last
    assert device_sum(a) == 1.0


# ---- complement ties: the inputs of tests/test_gpu_bls.py's planted cases ------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nbins", COMPLEMENT_NBINS)
def test_a_box_ties_with_its_complement_and_the_narrower_wins(nbins, weighted):
    """dips_only = False, every width 1 .. nbins - 1: each box has its complement among the boxes, with other sums and the same
    objective bit for bit -- the first gap is 0 at ALL 70 frequencies -- and the rule gives the narrower of the two, so no winner is
    wider than nbins / 2 and the search over 1 .. nbins / 2 (the widest the library takes: kmax <= nbins / 2) returns the same boxes
    and the same second gap.  The second gap leaves at most 2 frequencies with a near-tie (it leaves none)."""
    t, f, y, W = complement_case(weighted)
    kw = dict(nbins=nbins, kmin=1, min_count=1, dips_only=False, center_data=True, normalization="standard")
    full, half = bls_model(y, t, f, W, kmax=nbins - 1, **kw), bls_model(y, t, f, W, kmax=nbins // 2, **kw)
    assert full["ndeg"] == 0 and np.all(full["gap"] == 0) and full["gap"].shape == (70, 1)
    assert full["width"].max() <= nbins // 2 and np.all(full["gap2"] > 0)
    for key in ("start", "width", "count", "power", "depth", "depth_err", "gap2"):
        assert np.array_equal(full[key], half[key]), key
    near = (half["gap2"] <= 8).any(axis=1).sum()
    print(f"nbins {nbins} W={weighted}: widest winner {full['width'].max()}, smallest second gap {half['gap2'].min():.3g} ulp, {near} near-ties")
    assert near <= 2
    r = bls_ref_ld(y, t, f, W, kmax=nbins // 2, **kw)
    clear = half["gap2"] > 8                                                  # the long-double definition has the same near-exact tie: equal boxes or complements
    same = (half["start"] == r["start"]) & (half["width"] == r["width"])
    comp = (np.mod(half["start"] + half["width"], nbins) == r["start"]) & (half["width"] + r["width"] == nbins)
    assert np.all((same | comp)[clear])


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("nbins", COMPLEMENT_NBINS)
def test_the_half_period_record_makes_the_tie_decide(nbins, weighted):
    """At f = 1 the model's box is nbins / 2 wide and starts at nbins / 4; the first gap is 0 (the complement, nbins / 2 further on, is
    searched too) and the second is far from a near-tie: the earlier start is the answer because of the rule alone."""
    t, f, y, W = half_case(weighted)
    m = bls_model(y, t, f, W, nbins=nbins, kmin=1, kmax=nbins // 2, min_count=1, dips_only=False, center_data=True, normalization="standard")
    k = HALF_K
    assert f[k] == 1.0 and (m["start"][k, 0], m["width"][k, 0]) == (nbins // 4, nbins // 2) and m["count"][k, 0] == 256
    assert m["gap"][k, 0] == 0 and m["gap2"][k, 0] > 1e6 and m["depth"][k, 0] > 1.9 and m["ndeg"] == 0
    assert (m["gap2"] <= 8).any(axis=1).sum() <= 2
