"""Gather-form NUFFT spreading (csrc/nufft.hip: samples sorted by cell, one thread per cell, no atomics), the tiled assembly of the
structured Gram (csrc/nudft.hip) and the pad-only zero fill (csrc/api.hip) against the in-tree control LPVS_NUFFT_SPREAD=scatter (the
LDS-atomic scatter kernel) -- BIT FOR BIT: the grid is an integer sum, so any kernel that takes every addend once gives the same grid.
GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 0.731


def _problem(L, monkeypatch, Y, X, V, w, Nv, spread=None, nudft=None):
    """(G, b, gram_form) of a fresh handle; b is n x ns for several signals."""
    for name, value in (("LPVS_NUFFT_SPREAD", spread), ("LPVS_NUDFT", nudft)):
        if value:
            monkeypatch.setenv(name, value)
        else:
            monkeypatch.delenv(name, raising=False)
    Y = np.asarray(Y)
    make = L.Problem.lpv_multi if Y.ndim == 2 else L.Problem.lpv
    with make(Y, X, V, w, Nv) as p:
        G, _ = p.get_gram()
        b = p.get_rhs()
        form = p.timing()["gram_form"]
    return G, b, form


def _data(N, Nf, ns=1, sort=True, seed=None):
    rng = np.random.default_rng(N if seed is None else seed)
    X = rng.random(N) * 400.0 - 100.0
    if sort:
        X = np.sort(X)
    V = rng.random(N) * 2 - 0.5
    w = D * (1.0 + np.arange(Nf))                         # w = D (1 .. Nf): s0 is even, the right-hand sides go by NUFFT too
    Y = rng.standard_normal(N) if ns == 1 else rng.standard_normal((N, ns))
    return Y, X, V, w


@pytest.mark.parametrize("N,Nf,Nv,ns,sort", [(4096, 24, 3, 1, True),
                                             (20000, 130, 4, 1, False),     # shuffled abscissae
                                             (32769, 64, 8, 1, True),       # one sample into a second chunk
                                             (9000, 1000, 2, 1, True),      # fine grid of 8192 cells
                                             (6000, 20, 3, 3, True)])       # three signals: the rhs calls reuse the coordinates and their binning
def test_gather_equals_scatter_bit_for_bit(L, N, Nf, Nv, ns, sort, monkeypatch):
    Y, X, V, w = _data(N, Nf, ns, sort)
    Gg, bg, fg = _problem(L, monkeypatch, Y, X, V, w, Nv)
    Gs, bs, fs = _problem(L, monkeypatch, Y, X, V, w, Nv, spread="scatter")
    assert fg == "ap-nufft" and fs == "ap-nufft"
    assert np.array_equal(Gg, Gs)
    assert np.array_equal(bg, bs)
    assert np.abs(bg).max() > 0 and np.abs(Gg).max() > 0


@pytest.mark.parametrize("N", [4096, 20000])
def test_sample_order_does_not_change_a_bit(L, N, monkeypatch):
    """(y, X, V) permuted together: other bins per run, other chunk partials -- the same integer sums, so the same G and b."""
    Y, X, V, w = _data(N, 40, sort=True)
    G0, b0, f0 = _problem(L, monkeypatch, Y, X, V, w, 3)
    assert f0 == "ap-nufft"
    for perm in (np.random.default_rng(1).permutation(N), np.arange(N)[::-1]):
        G1, b1, _ = _problem(L, monkeypatch, np.ascontiguousarray(Y[perm]), np.ascontiguousarray(X[perm]), np.ascontiguousarray(V[perm]), w, 3)
        assert np.array_equal(G1, G0)
        assert np.array_equal(b1, b0)


@pytest.mark.parametrize("all_equal", [False, True])
def test_clustered_abscissae(L, all_equal, monkeypatch):
    """Half of the samples (or all of them) at ONE abscissa: one bin of every sorted run holds them, a cell's thread walks up to a
    whole run per stage -- the same code path, the same bits, and the direct sums to the bound of tests/test_gpu_nufft.py."""
    N, Nf, Nv = 8192, 24, 3
    Y, X, V, w = _data(N, Nf, sort=False)
    if all_equal:
        X[:] = 37.25
    else:
        X[::2] = 37.25
    Gg, bg, fg = _problem(L, monkeypatch, Y, X, V, w, Nv)
    Gs, bs, fs = _problem(L, monkeypatch, Y, X, V, w, Nv, spread="scatter")
    Gd, bd, fd = _problem(L, monkeypatch, Y, X, V, w, Nv, nudft="direct")
    assert fg == "ap-nufft" and fs == "ap-nufft" and fd == "ap"
    assert np.array_equal(Gg, Gs) and np.array_equal(bg, bs)
    assert np.abs(Gg - Gd).max() <= 1e-12 * np.abs(Gd).max(), np.abs(Gg - Gd).max() / np.abs(Gd).max()
    assert np.abs(bg - bd).max() <= 1e-12 * np.abs(bd).max(), np.abs(bg - bd).max() / np.abs(bd).max()


def _iterates(L, Y, X, V, w, Nv, iters):
    with L.Problem.lpv(Y, X, V, w, Nv) as p:
        p.set_prox(L.SlicedSeparableSum.frequency_groups(5.0, len(w), 2 * Nv))
        p.admm_init(None, μ=0.05, tol=0.0)
        p.admm_run(iters)
        return p.admm_get()


@pytest.mark.parametrize("Nf,Nv,n,n_pad", [(37, 3, 222, 256), (65, 2, 260, 384)])
def test_tiled_assembly_and_pad_only_zero_fill(L, Nf, Nv, n, n_pad, monkeypatch):
    """n is no multiple of the 32-wide tile and smaller than the padded size: ragged tiles on the diagonal and at the edge, and pad
    strips that only the trimmed zero fill writes."""
    N = 4096
    Y, X, V, w = _data(N, Nf, sort=True, seed=Nf)
    # a handle whose Gram reaches into what is pad for the handles below goes back to the pool first: stale, non-zero memory of their size
    Yo, Xo, Vo, wo = _data(N, n_pad // (2 * Nv), sort=True, seed=99)
    _problem(L, monkeypatch, Yo, Xo, Vo, wo, Nv)
    Gs, bs, fs = _problem(L, monkeypatch, Y, X, V, w, Nv, spread="scatter")
    monkeypatch.delenv("LPVS_NUFFT_SPREAD", raising=False)
    with L.Problem.lpv(Y, X, V, w, Nv) as p:
        assert p.n == n and p.timing()["gram_form"] == "ap-nufft" and fs == "ap-nufft"
        G, b = p.get_gram()
        Gt, bt = p.device_gram()
        assert tuple(Gt.shape) == (n_pad, n_pad)
        Gdev = Gt.cpu().numpy()
    assert np.array_equal(G, G.T)
    assert np.array_equal(G, Gs) and np.array_equal(b, bs)
    assert np.array_equal(Gdev[:n, :n], G) or np.array_equal(Gdev[:n, :n], G.T)
    assert not Gdev[n:, :].any() and not Gdev[:, n:].any()
    if n == 222:   # no stale pad reaches the factorisation: two handles iterate alike
        a, c = _iterates(L, Y, X, V, w, Nv, 20), _iterates(L, Y, X, V, w, Nv, 20)
        for u, v in zip(a, c):
            assert np.array_equal(u, v)
        assert np.isfinite(a[0]).all()
