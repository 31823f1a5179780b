"""The references of the fold statistics (tests/_fold_ref.py) proven on the CPU: the models -- the definition as the device computes it
-- against the definition in long double within the bounds derived there, on every case of tests/test_gpu_fold.py; theta against
Stellingwerf's formula evaluated from per-bin sample variances; aov against the textbook between / within F ratio; the entropy against
sum p_ij ln(p_i / p_ij) evaluated directly; the planted period; and the condition on the inputs of the conditional entropy that makes
its value bins unambiguous.  Runs anywhere."""
import functools

import numpy as np
import pytest

from _bls_ref import LD, base_case, fold_bins, ld_bins
from _fold_ref import (CENT_CASES, PDM_CASES, aov_of, case_inputs, cent_bound, cent_model, cent_ref_ld, pdm_bounds, pdm_model, pdm_ref_ld, sawtooth_case, theta_of,
                       value_bins)


@functools.lru_cache(maxsize=None)
def pdm_refs(name):
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES[name]
    t, f, y, W = case_inputs(N, Nf, ns, weighted)
    return pdm_model(y, t, f, W, nbins, covers, center), pdm_ref_ld(y, t, f, W, nbins, covers, center)


@functools.lru_cache(maxsize=None)
def cent_refs(name):
    N, Nf, nbins, mbins, ns, plan = CENT_CASES[name]
    t, f, y, W = case_inputs(N, Nf, ns, False)
    return cent_model(y, t, f, nbins, mbins), cent_ref_ld(y, t, f, nbins, mbins)


@pytest.mark.parametrize("name", list(PDM_CASES))
def test_the_pdm_model_lies_within_the_derived_bound_of_the_long_double_definition(name):
    N, Nf, nbins, covers, ns, weighted, center, plan = PDM_CASES[name]
    t, f, y, W = case_inputs(N, Nf, ns, weighted)
    m, r = pdm_refs(name)
    assert np.array_equal(fold_bins(f, t, nbins * covers)[0], ld_bins(f, t, nbins * covers)[0])
    assert np.array_equal(m["nonempty"], r["nonempty"]) and np.all(np.isfinite(m["explained"]))
    live = m["degenerate"] == 0
    if N == 1:
        assert not live.any() and np.all(m["explained"] == 0)
        return
    assert live.all()
    b = pdm_bounds(y, W, center, m["shy"], nbins * covers, r["explained"])
    e = np.abs(m["explained"].astype(LD) - np.minimum(r["explained"], 1))
    print(f"{name}: worst error / bound {float((e / b).max()):.3g}")
    assert np.all(e <= b)


@pytest.mark.parametrize("name", list(CENT_CASES))
def test_the_entropy_model_lies_within_the_derived_bound_of_the_long_double_definition(name):
    N, Nf, nbins, mbins, ns, plan = CENT_CASES[name]
    m, r = cent_refs(name)
    b = cent_bound(nbins * mbins, r)
    e = np.abs(m["entropy"].astype(LD) - r)
    print(f"{name}: worst error / bound {float((e / b).max()):.3g}")
    assert np.all(e <= b) and np.all(m["entropy"] >= 0) and np.all(m["entropy"] <= np.log(mbins) * (1 + 1e-15))


@pytest.mark.parametrize("nbins,covers", [(10, 1), (5, 2), (8, 4)])
def test_theta_is_stellingwerfs_pooled_variance_ratio(nbins, covers):
    """theta = s^2 / sigma^2, s^2 = sum_j (n_j - 1) s_j^2 / (sum_j n_j - M) over the M non-empty bins of ALL covers (s_j^2: the sample
    variance of bin j), sigma^2 the sample variance of the record -- evaluated here sample by sample, no histogram."""
    t, f, y = base_case(seed=1, N=400, span=64.0)
    f = f[::7]
    m = pdm_model(y, t, f, None, nbins, covers, True)
    theta = theta_of(m["explained"], m["nonempty"], len(t), covers, m["degenerate"])[:, 0]
    nfine = nbins * covers
    bins = ld_bins(f, t, nfine)[0]
    sigma2 = np.var(y.astype(LD), ddof=1)
    for k in range(len(f)):
        num, den, M = LD(0), 0, 0
        for j in range(nfine):
            inside = ((bins[k] - j) % nfine) < covers
            n = int(inside.sum())
            if n == 0:
                continue
            M += 1
            den += n
            num += ((y[inside].astype(LD) - y[inside].astype(LD).mean()) ** 2).sum()      # (n_j - 1) s_j^2
        assert M == m["nonempty"][k] and den == covers * len(t)
        want = num / (den - M) / sigma2
        assert abs(theta[k] - want) <= 1e-12 * want, (k, theta[k], want)


def test_aov_is_the_between_within_f_ratio():
    t, f, y = base_case(seed=1, N=400, span=64.0)
    f = f[::7]
    m = pdm_model(y, t, f, None, 10, 1, True)
    F = aov_of(m["explained"], m["nonempty"], len(t), m["degenerate"])[:, 0]
    bins = ld_bins(f, t, 10)[0]
    yl = y.astype(LD)
    for k in range(len(f)):
        groups = [yl[bins[k] == j] for j in range(10) if np.any(bins[k] == j)]
        M = len(groups)
        between = sum(len(g) * (g.mean() - yl.mean()) ** 2 for g in groups) / (M - 1)
        within = sum(((g - g.mean()) ** 2).sum() for g in groups) / (len(t) - M)
        assert abs(F[k] - between / within) <= 1e-12 * (between / within)


def test_the_entropy_is_the_conditional_shannon_entropy_of_the_counts():
    t, f, y = base_case(seed=1, N=400, span=64.0)
    f = f[::7]
    m = cent_model(y, t, f, 10, 5)
    p = m["hist"][:, 0].astype(LD) / len(t)
    for k in range(len(f)):
        H = LD(0)
        for i in range(10):
            for j in range(5):
                if p[k, i, j] > 0:
                    H += p[k, i, j] * np.log(p[k, i].sum() / p[k, i, j])
        assert abs(m["entropy"][k, 0] - H) <= 1e-12 * H


def test_the_planted_sawtooth_is_found_by_all_three():
    """A unit sawtooth at f0 = 1.25 (variance 1 / 12) under noise of sigma 1 / 4: the bins of (10, 1) explain (1 / 12)(1 - 1 / 100) /
    (1 / 12 + 1 / 16) = 0.566 of the variance at f0; with (5, 2) the cover whose bin straddles the jump loses that bin and the share is
    about 0.41.  Away from f0 (no harmonic relation on this grid) the folds explain a few per cent."""
    t, f, y = sawtooth_case()
    k0 = int(np.nonzero(f == 1.25)[0][0])
    for (nbins, covers), at, others in (((10, 1), 0.566, 0.1), ((5, 2), 0.41, 0.06)):
        m = pdm_model(y, t, f, None, nbins, covers, True)
        e = m["explained"][:, 0]
        print(f"pdm ({nbins}, {covers}): {e[k0]:.3f} at f0, at most {np.delete(e, k0).max():.3f} elsewhere")
        assert int(np.argmax(e)) == k0 and abs(e[k0] - at) < 0.03 and np.delete(e, k0).max() < others
        theta = theta_of(m["explained"], m["nonempty"], len(t), covers, m["degenerate"])[:, 0]
        assert int(np.argmin(theta)) == k0
        if covers == 1:
            assert int(np.argmax(aov_of(m["explained"], m["nonempty"], len(t), m["degenerate"])[:, 0])) == k0
    H = cent_model(y, t, f, 10, 5)["entropy"][:, 0]
    print(f"conditional entropy (10, 5): {H[k0]:.3f} at f0, at least {np.delete(H, k0).min():.3f} elsewhere")
    assert int(np.argmin(H)) == k0 and H[k0] < 1.0 and np.delete(H, k0).min() > 1.2


def test_no_sample_but_the_extremes_lies_at_the_edge_of_a_value_bin():
    """u mbins within 2^-40 of an integer would leave the bin to the last place of the quotient: none does (a cap of ZERO samples), on
    every case of the GPU file and on the planted one.  The two extremes (u = 0 and u = 1, exact) are the exception."""
    records = [(case_inputs(c[0], c[1], c[4], False)[2], c[3]) for c in CENT_CASES.values()] + [(sawtooth_case()[2], 5)]
    nearest = np.inf
    for y, mbins in records:
        y = np.asarray(y, np.float64).reshape(len(y), -1)
        if len(y) == 1:
            continue
        j, ylim, deg, x = value_bins(y, mbins)
        inner = (y != ylim[:, 0]) & (y != ylim[:, 1])
        d = np.abs(x - np.rint(x))[inner]
        nearest = min(nearest, d.min())
        assert (d <= 2.0 ** -40).sum() == 0
    print(f"the nearest u mbins to an integer: {nearest:.3g}")
