"""The factorisation M = (G + shift I)^-1 of csrc/linalg.hip, checked EXACTLY through every schedule.

On the integer family of tests/_sweep_ref.py (H = L L', L unit lower triangular: every pivot is 1, every partially swept matrix
is integer, every intermediate < 2^20 -- proven on the host by tests/test_sweep_ref_host.py) the blocked sweep commits no rounding,
whatever the pivot kernel, the block width, the grouping of the panels or the order of the updates: the device must return the
closed-form inverse bit for bit.  A lost or doubled update, a tile that misses a panel, a band launch that overtakes the pass it
depends on shows at the exact entry, not as 1e-10 under an absolute bound.

    1  the exact inverse at every size that takes another path, under every knob set (tests/_sweep_ref.py: KNOB_SETS)
    2  the same scaled by powers of two: entries over 2^-40 .. 2^54, pivots 2^-40 .. 2^40
    3  three factorisations of a real-valued matrix on one handle and one on a fresh handle: the same bits
    4  a non-positive pivot in the first / a later / the last block is reported by every pivot kernel, and the handle recovers
    5  graded real matrices against the extended-precision inverse, componentwise, within 8 x what LAPACK achieves

G travels to the device bit for bit (test_gpu_parity.py::test_gram_dense_and_explicit), G = H - s I with an integer s >= 1 and
get_inverse(s) hand the sweep exactly H."""
import contextlib
import functools

import numpy as np
import pytest

import _sweep_ref as R

pytestmark = pytest.mark.gpu

SHIFT = 3.0                                   # G = H - 3 I: integer, exact; the device adds it back on the diagonal
SOME = [{}, {"LPVS_PIVOT": "regs"}, {"LPVS_PIVOT": "sweep64"}, {"LPVS_FACTOR": "sweep64"}]


def _set(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@contextlib.contextmanager
def _problem(L, G, knobs=()):
    """A Gram handle on G.  LPVS_RESERVE_CUS is read when a handle's stream bundle factorises for the first time, and bundles are
    recycled through a per-process cache of at most eight (api.hip: bundle_acquire): for a knob set that names it, eight placeholder
    handles empty that cache first, so that this handle's bundle is new -- and they are closed before it, so that the cache is full
    again and the bundle made under the knob is destroyed instead of being handed to a later test."""
    b = np.zeros(G.shape[0])
    if "LPVS_RESERVE_CUS" not in knobs:
        with L.Problem.gram(G, b) as p:
            yield p
        return
    hold = [L.Problem.gram(np.eye(8), np.zeros(8)) for _ in range(8)]
    try:
        p = L.Problem.gram(G, b)
    finally:
        for q in hold:
            q.close()
    try:
        yield p
    finally:
        p.close()


def _assert_exact(M, ref, what):
    if not np.array_equal(M, ref):
        cnt, blk = R.first_mismatch(M, ref)
        r, c = np.argwhere(M != ref)[0]
        pytest.fail(f"{what}: {cnt} of {M.size} entries differ, first in 128-block (row, column) = {blk}: "
                    f"M[{r}, {c}] = {M[r, c]!r}, exact {ref[r, c]!r}")


@functools.lru_cache(maxsize=None)
def _integer_system(n):
    H, Hinv = R.unimodular_spd(n)
    G = np.array(H)
    G[np.arange(n), np.arange(n)] -= SHIFT
    G.setflags(write=False)
    return G.T, Hinv                                            # (symmetric; the column-major view is what the wrapper hands over without a copy)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
#   n     np    path
#   200   256   single-level sweep (diag_inverse / panel / sweep_update kernels)
#   640   640   single-level sweep; five 128-tiles, an odd count
#   1000  1024  first two-level size, padded: steps schedule with look-ahead (pivot_inverse_kernel<128>, rank_update_kernel which = 1 / 2)
#   1100  1152  two-level below the group schedule, ragged
#   2100  2176  group schedule, 17 pivot blocks: groups 2 + 2 + ... + 1
#   2300  2304  group schedule, 18 blocks
#   2500  2560  group schedule, 20 blocks
@pytest.mark.parametrize("knobs", R.KNOB_SETS, ids=R.knob_id)
@pytest.mark.parametrize("n", [200, 640, 1000, 1100, 2100, 2300, 2500])
def test_integer_inverse_is_exact_under_every_schedule(L, n, knobs, monkeypatch):
    _set(monkeypatch, knobs)
    G, Hinv = _integer_system(n)
    with _problem(L, G, knobs) as p:
        M = p.get_inverse(SHIFT)
    _assert_exact(M, Hinv, f"n = {n}, {R.knob_id(knobs)}")


@pytest.mark.parametrize("knobs", [{}, {"LPVS_FACTOR_SCHEME": "steps"}, {"LPVS_FACTOR_SCHEME": "steps", "LPVS_LOOKAHEAD": "1"}, {"LPVS_KW": "256"}],
                         ids=R.knob_id)
def test_integer_inverse_is_exact_above_the_depth_two_threshold(L, knobs, monkeypatch):
    """n = 6200 (np = 6272 >= 6144): the steps schedule takes the depth-2 look-ahead (three panel buffers, rank_update_kernel which = 3 / 4),
    LPVS_LOOKAHEAD=1 the depth-one schedule at the same size, the default the group schedule with 49 pivot blocks.  The host model at
    n = 6200, 128-wide blocks: exact, largest intermediate 2^15.4 (half a minute of numpy: run once, not part of the suite)."""
    _set(monkeypatch, knobs)
    G, Hinv = _integer_system(6200)
    with _problem(L, G, knobs) as p:
        M = p.get_inverse(SHIFT)
    _assert_exact(M, Hinv, f"n = 6200, {R.knob_id(knobs)}")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", SOME + [R.LARGE_DEFAULTS], ids=R.knob_id)
@pytest.mark.parametrize("n", [1100, 2300])
def test_power_of_two_scaling_is_exact(L, n, knobs, monkeypatch):
    """D H D with D = 2^e, e in [-20, 20], handed over as it stands with shift = 0 (get_inverse accepts a zero shift: the diagonal gets
    + 0.0): D^-1 H^-1 D^-1 bit for bit."""
    _set(monkeypatch, knobs)
    H, Hinv = R.unimodular_spd(n)
    Hs, His, _ = R.scaled(H, Hinv)
    with _problem(L, Hs, knobs) as p:
        M = p.get_inverse(0.0)
    _assert_exact(M, His, f"scaled, n = {n}, {R.knob_id(knobs)}")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gaussian_gram(n):
    rng = np.random.default_rng(n)                              # the matrix of test_gpu_edges.py::test_factorisation_variants_give_the_inverse
    A = rng.standard_normal((n + 50, n))
    G = A.T @ A
    G.setflags(write=False)
    return G


@pytest.mark.parametrize("knobs", [{}, {"LPVS_FACTOR_GROUP": "4", "LPVS_RU_STAGE": "8"}, {"LPVS_FACTOR_SCHEME": "steps"}, {"LPVS_RESERVE_CUS": "0"}],
                         ids=R.knob_id)
def test_refactorisation_gives_the_same_bits(L, knobs, monkeypatch):
    """The band launches on the side stream and the deep pass on the CU-masked stream are ordered by events alone: a missing wait shows
    as a tile with one update too few on some runs.  get_inverse(21) evicts the cached inverse, so the handle factorises three times."""
    _set(monkeypatch, knobs)
    G = _gaussian_gram(2300)
    with _problem(L, G, knobs) as p:
        M1 = p.get_inverse(20.0)
        M2 = p.get_inverse(21.0)
        M3 = p.get_inverse(20.0)
    with _problem(L, G, knobs) as p:
        M4 = p.get_inverse(20.0)
    assert not np.array_equal(M1, M2)
    _assert_exact(M3, M1, f"third against first factorisation, {R.knob_id(knobs)}")
    _assert_exact(M4, M1, f"fresh handle against first factorisation, {R.knob_id(knobs)}")
    assert np.abs(M1 @ (G + 20.0 * np.eye(2300)) - np.eye(2300)).max() <= 5e-13


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", SOME + [{"LPVS_KW": "256"}], ids=R.knob_id)
@pytest.mark.parametrize("n", [1100, 2300])
def test_non_positive_pivot_is_reported_and_the_handle_recovers(L, n, knobs, monkeypatch):
    """H[j, j] -= 2^20: pivot j is 1 - 2^20 and everything after it stays finite.  j = 0 / 127: first and last pivot of the first 128-wide
    block, 128 * 3 + 5: a block whose chain runs on the side stream, n - 1: the ragged last block.  The default inverts the block with
    pivot_inverse_mfma_kernel (n = 2300) / pivot_inverse_kernel<128> (n = 1100), regs with pivot_inverse_kernel<128>, sweep64 and KW = 256
    with diag_inverse_kernel.  The refusal is repeated when asked again (no stale M_valid); the clean G written into the SAME handle
    then gives the exact inverse (no leftover status flag); the bad entry written back is refused again although an inverse for that
    shift was cached."""
    import torch
    _set(monkeypatch, knobs)
    G, Hinv = _integer_system(n)
    clean = torch.from_numpy(np.array(G))
    for j in (0, 127, 128 * 3 + 5, n - 1):
        Gbad = np.array(G)
        Gbad[j, j] -= 2.0 ** 20
        with _problem(L, Gbad, knobs) as p:
            for _ in range(2):
                with pytest.raises(L.NumericError, match="not positive definite"):
                    p.get_inverse(SHIFT)
            Gd, _ = p.device_gram()
            assert Gd.shape == (R.padded_size(n), R.padded_size(n))
            Gd[:n, :n].copy_(clean)                                # (symmetric: row- and column-major agree)
            torch.cuda.synchronize()
            p.gram_modified()
            _assert_exact(p.get_inverse(SHIFT), Hinv, f"after a refusal at pivot {j}, n = {n}, {R.knob_id(knobs)}")
            Gd[j, j] -= 2.0 ** 20
            torch.cuda.synchronize()
            p.gram_modified()
            with pytest.raises(L.NumericError, match="not positive definite"):
                p.get_inverse(SHIFT)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
GRADED = [(1100, 0), (1100, 4), (1100, 6), (2300, 0)]            # (the extended-precision reference of n = 2300 takes 20 s on the host: k = 0 only)


@functools.lru_cache(maxsize=None)
def _graded(n, k):
    """G = A'A, A Gaussian (n + 50) x n with column j scaled by 10^(-k j / n); H = G + shift I, shift = 1e-6 max diag(G), rounded as
    the device rounds it; M_ld = H^-1 from the extended-precision Cholesky factor; E = |M_ld| |H| |M_ld|, the first-order componentwise
    error bound (in units of the rounding unit) of ANY inversion method; r_host = the ratio of LAPACK's double-precision inverse."""
    from oracle import oracle
    rng = np.random.default_rng([n, k])
    A = rng.standard_normal((n + 50, n)) * 10.0 ** (-k * np.arange(n) / n)[None, :]
    G = A.T @ A
    shift = 1e-6 * G.diagonal().max()
    H = G + shift * np.eye(n)
    M_ld = oracle.inverse_ld(H, 1e300)                           # (+ 1e-300 on the diagonal: nothing)
    E = np.abs(M_ld) @ np.abs(H) @ np.abs(M_ld)
    assert E.min() > 0
    r_host = (np.abs(np.linalg.inv(H) - M_ld) / E).max()
    for a in (G, M_ld, E):
        a.setflags(write=False)
    return G, shift, M_ld, E, r_host


@pytest.mark.parametrize("knobs", [{}, {"LPVS_PIVOT": "regs"}, {"LPVS_FACTOR": "sweep64"}, R.LARGE_DEFAULTS], ids=R.knob_id)
@pytest.mark.parametrize("n,k", GRADED)
def test_graded_matrices_componentwise_against_extended_precision(L, n, k, knobs, monkeypatch):
    """r(M) = max |M - M_ld| / E  <=  8 max(r_host, 2^-53): the margin over LAPACK's Cholesky-based inverse (three triangular passes) is
    for np/64 .. np/128 dependent block updates of an equally stable algorithm, and it is taken from the reference side.  Measured
    ratios: DESIGN.md 4.4.1."""
    _set(monkeypatch, knobs)
    G, shift, M_ld, E, r_host = _graded(n, k)
    with _problem(L, G, knobs) as p:
        M = p.get_inverse(shift)
    r_dev = (np.abs(M - M_ld) / E).max()
    print(f"graded n={n} k={k} {R.knob_id(knobs)}: r_host = {r_host * 2.0 ** 53:.3f} u, r_dev = {r_dev * 2.0 ** 53:.3f} u (u = 2^-53)")
    assert np.array_equal(M, M.T)
    assert r_dev <= 8 * max(r_host, 2.0 ** -53), (r_dev * 2.0 ** 53, r_host * 2.0 ** 53)
