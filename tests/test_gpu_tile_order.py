"""The mirrored tile order of the one-launch ADMM iteration (csrc/tile_order.h; the default of single-problem handles) against the same
order on every launch (LPVS_TILE_ORDER=forward): the tile sums are added as 64-bit integers, so any bijection of tiles onto workgroups
gives the same bits -- x, z, u, the iteration count and ||x - z|| are compared with np.array_equal, over sizes (n = 2304: 153 tiles
below the diagonal, not a multiple of 8), prox operators and storages, across the ramped nibble refreshes of the 32-bit reads (every launch
at first, every 16th by iteration 128) and the x-update corrections after iterations 16 and 128, and under any chunking of the run.  GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ITERS = 200


def _signal(N, Nf, rng):
    X = np.sort(rng.random(N) * (10.0 * N / 500)); V = np.linspace(0, 1, N)
    w = 2 * np.pi * (np.arange(Nf) + 1.0) * 25.0 / Nf
    y = 2 * V ** 2 * np.cos(w[Nf // 10] * X) + 2 / (5 * V + 1) * np.cos(w[Nf // 3] * X - 0.3) + 0.1 * rng.standard_normal(N)
    return y, X, V, w


@pytest.fixture(scope="module")
def problems():
    # n = 2 Nf Nv: 2048 (16 row blocks), 2304 (18 row blocks), 8192 (64 row blocks, the benchmark's size); enough samples for the mixed storage to hold
    out = {}
    for n, N, Nf in ((2048, 1 << 18, 128), (2304, 1 << 18, 144), (8192, 1 << 20, 512)):
        out[n] = (N, Nf, 8) + _signal(N, Nf, np.random.default_rng(n))
    return out


def _run(L, problem, kind, storage, chunks, monkeypatch, order):
    N, Nf, Nv, y, X, V, w = problem
    if order is None:
        monkeypatch.delenv("LPVS_TILE_ORDER", raising=False)
    else:
        monkeypatch.setenv("LPVS_TILE_ORDER", order)
    if storage == "f32":
        y, X, V, w = (a.astype(np.float32) for a in (y, X, V, w))
    prox = L.SlicedSeparableSum.frequency_groups(2.0, Nf, 2 * Nv) if kind == "group" else L.NormL1(0.5)
    with L.Problem.lpv(y, X, V, w, Nv) as p:
        if storage == "mixed":
            p.set_option("storage", "mixed")                 # by name: all 36 bits of the fixed-point tiles are read
        p.set_prox(prox)
        p.admm_init(None, μ=0.05, tol=0.0)
        info = p.matvec_info()
        assert info["kernel"] == "admm_iter_mixed_kernel" and info["one_launch_iteration"], info
        if storage == "mixed32":
            assert "32 leading bits" in info["storage"], info
        if storage == "mixed":
            assert "32 leading bits" not in info["storage"], info
        for c in chunks:
            it, nxz, conv = p.admm_run(c)
        return (it, nxz, conv) + p.admm_get()


@pytest.mark.parametrize("storage", ["mixed32", "mixed", "f32"])
@pytest.mark.parametrize("kind", ["group", "l1"])
@pytest.mark.parametrize("n", [2048, 2304, 8192])
def test_mirrored_tile_order_gives_the_bits_of_the_forward_order(L, problems, n, kind, storage, monkeypatch):
    a = _run(L, problems[n], kind, storage, [ITERS], monkeypatch, "forward")
    b = _run(L, problems[n], kind, storage, [ITERS], monkeypatch, None)
    c = _run(L, problems[n], kind, storage, [ITERS], monkeypatch, "mirror")
    for r in (b, c):
        assert a[0] == r[0] == ITERS and a[1] == r[1] and a[2] == r[2]
        for va, vb in zip(a[3:6], r[3:6]):                   # x, z, u
            assert np.array_equal(va, vb), np.abs(va - vb).max()
    assert np.isfinite(a[1]) and np.count_nonzero(a[4]) > 0  # (a run that did something)


@pytest.mark.parametrize("n", [2048, 2304, 8192])
def test_mirrored_tile_order_does_not_depend_on_chunking(L, problems, n, monkeypatch):
    """The parity is that of the absolute iteration index: chunks of odd length start on either parity."""
    ref = _run(L, problems[n], "group", "mixed32", [ITERS], monkeypatch, None)
    for size in (7, 1, 64, 128):
        chunks = [size] * (ITERS // size) + ([ITERS % size] if ITERS % size else [])
        r = _run(L, problems[n], "group", "mixed32", chunks, monkeypatch, None)
        assert r[0] == ref[0] == ITERS and r[1] == ref[1]
        for a, b in zip(r[3:6], ref[3:6]):
            assert np.array_equal(a, b), (size, np.abs(a - b).max())
