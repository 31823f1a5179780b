"""Host side of the factorisation's exact tests, numpy only: a family of SPD matrices on which the blocked
symmetric sweep of csrc/linalg.hip commits NO rounding at all, their inverses in closed form, and a numpy model of the sweep that
proves it (and the cap on the intermediates that keeps it true) without a GPU.

The family.  L = L1 L2 unit lower triangular with small integers, H = L L':
    L1 = I + diag(eps, -1), eps in {-1, +1}                      (bidiagonal: L1^-1 is a full lower triangle of +-1)
    L2 = I + N, N = 3n entries from {-2 .. 2} at random places with row >= n/2 > column    (N^2 = 0: L2^-1 = I - N)
Every leading principal minor of H is 1, so every scalar pivot the sweep meets is exactly 1 and every partially swept matrix
(-A11^-1, A11^-1 A12, the Schur complement; A11 unimodular) is an integer matrix.  1.0 / d, products, FMAs and f64 matrix
instructions are exact on integers below 2^53, whatever the block width, the grouping or the order of the updates:
H^-1 = L^-T L^-1 comes back bit for bit.  D H D with D = diag(2^e) keeps every operation exact (pivots 2^(2e), result
D^-1 H^-1 D^-1) and spreads the entries over many decades.

All matrix products here are float64 BLAS: exact at these magnitudes (products < 2^28, sums of < 2^13 of them < 2^41)."""
import functools

import numpy as np

# Every schedule / kernel selection of spd_inverse_two_level the GPU tests run (csrc/linalg.hip; the first 17 are the list of
# test_gpu_edges.py::test_factorisation_variants_give_the_inverse), then the defaults of np >= 12288 -- groups of four, 8-pivot
# stages, pivot kernel without its LDS padding -- which no test size reaches on its own, without and with the 128-wide band tiles
# that are the default from np = 8192.
LARGE_DEFAULTS = {"LPVS_FACTOR_GROUP": "4", "LPVS_RU_STAGE": "8", "LPVS_PIVOT_ALONE": "0"}
KNOB_SETS = [{}, {"LPVS_KW": "256"}, {"LPVS_KW": "256", "LPVS_LOOKAHEAD": "0"}, {"LPVS_LOOKAHEAD": "0"},
             {"LPVS_PIVOT": "sweep64"}, {"LPVS_FACTOR": "sweep64"}, {"LPVS_FACTOR_SCHEME": "steps"},
             {"LPVS_CHAIN": "split"}, {"LPVS_PIVOT": "regs"}, {"LPVS_FACTOR_GROUP": "1"}, {"LPVS_FACTOR_GROUP": "2"},
             {"LPVS_FACTOR_GROUP": "3"}, {"LPVS_FACTOR_GROUP": "4", "LPVS_RU_STAGE": "8"}, {"LPVS_RESERVE_CUS": "0"},
             {"LPVS_BAND_TILE": "128"}, {"LPVS_BAND_TILE": "64", "LPVS_FACTOR_GROUP": "4"}, {"LPVS_PIVOT_ALONE": "0"},
             dict(LARGE_DEFAULTS), dict(LARGE_DEFAULTS, LPVS_BAND_TILE="128")]

CAP = 2.0 ** 20                      # bound on every intermediate of the sweep that the tests rely on (measured: < 2^14)


def knob_id(knobs):
    return ",".join(f"{k[5:]}={v}" for k, v in knobs.items()) or "default"


def padded_size(n):
    return -(-int(n) // 128) * 128


def _solve_l1t(V, eps):
    """L1^-T V for L1 = I + diag(eps, -1), by the recurrence of the upper bidiagonal L1': U[i] = V[i] - eps[i] U[i+1]."""
    U = np.array(V, dtype=np.float64)
    for i in range(U.shape[0] - 2, -1, -1):
        U[i] -= eps[i] * U[i + 1]
    return U


@functools.lru_cache(maxsize=None)
def _unimodular_spd(n, seed):
    rng = np.random.default_rng([int(n), int(seed)])
    eps = rng.choice([-1.0, 1.0], size=n - 1)
    h = n // 2
    N = np.zeros((n, n))
    N[rng.integers(h, n, size=3 * n), rng.integers(0, h, size=3 * n)] = rng.integers(-2, 3, size=3 * n).astype(np.float64)
    Nb = N[h:, :h]                                                 # the only non-zero block of N
    # H = L1 W L1' with W = (I + N)(I + N)' = I + N + N' + N N'; the bidiagonal L1 is applied as row / column operations
    W = np.eye(n) + N + N.T
    W[h:, h:] += Nb @ Nb.T
    W[1:] += eps[:, None] * W[:-1].copy()                          # L1 W
    W[:, 1:] += eps[None, :] * W[:, :-1].copy()                    # (L1 W) L1'
    H = W
    # H^-1 = L1^-T V L1^-1 with V = (I - N)'(I - N) = I - N - N' + N' N; L1 is inverted by its recurrence, from both sides
    V = np.eye(n) - N - N.T
    V[:h, :h] += Nb.T @ Nb
    Hinv = _solve_l1t(_solve_l1t(V, eps).T, eps)
    assert np.array_equal(H, H.T) and np.array_equal(Hinv, Hinv.T)
    assert np.abs(Hinv).max() < 2.0 ** 30                        # (integers throughout: every operation above is exact)
    assert np.array_equal(Hinv @ H, np.eye(n)), "the closed-form inverse is not the inverse"
    H.setflags(write=False); Hinv.setflags(write=False)
    return H, Hinv


def unimodular_spd(n, seed=0):
    """(H, H^-1): float64 arrays holding integers, read-only (cached by (n, seed))."""
    return _unimodular_spd(int(n), int(seed))


def scaled(H, Hinv, seed=0, emax=20):
    """(D H D, D^-1 H^-1 D^-1, D) with D = 2^e, e uniform integers in [-emax, emax]: every entry is scaled by a power of two."""
    n = H.shape[0]
    e = np.random.default_rng([n, int(seed), 77]).integers(-emax, emax + 1, size=n)
    D = np.ldexp(1.0, e)
    return D[:, None] * H * D[None, :], Hinv / D[:, None] / D[None, :], D


def pad_identity(A, n_pad):
    """A with the identity on the pad diagonal, as the device pads (G + shift I) to a multiple of 128."""
    n = A.shape[0]
    P = np.eye(n_pad)
    P[:n, :n] = A
    return P


def blocked_sweep(H, nb, D=None, stop_at_bad=False):
    """The numpy model of the header of csrc/linalg.hip: for every nb-wide pivot block k (a ragged last one included)
        P = A_kk^-1 by nb scalar symmetric sweeps;  B = A[:, k] (block k zeroed);  C = B P;  A -= C B';
        A[:, k] = C, A[k, :] = C', A_kk = -P;        after all blocks A = -H^-1.
    Returns (H^-1 as the model computes it, the largest |intermediate| -- the stored matrix after every block step, which holds
    the panels C, and the pivot block after every scalar sweep --, the index of the first pivot d with not (d > 0), or None).
    With D (the diagonal of `scaled`) the intermediates are measured in the units of the unscaled matrix: a partially swept
    D H D is T A T with A the partially swept H and T = D on the rows still to sweep, D^-1 on the swept ones.
    stop_at_bad: return (None, largest so far, index) at the first such pivot instead of sweeping on."""
    A = np.array(H, dtype=np.float64)
    n = A.shape[0]
    t = np.ones(n) if D is None else np.array(D, dtype=np.float64)
    size = (lambda X, tr, tc: np.abs(X).max()) if D is None else (lambda X, tr, tc: np.abs(X / tr[:, None] / tc[None, :]).max())
    big, bad = size(A, t, t), None
    for k0 in range(0, n, nb):
        k1 = min(k0 + nb, n)
        S = A[k0:k1, k0:k1].copy()
        ts = t[k0:k1].copy()
        for p in range(k1 - k0):                                   # scalar sweeps: S -> -S^-1
            d = S[p, p]
            if bad is None and not d > 0:
                bad = k0 + p
                if stop_at_bad:
                    return None, float(big), bad
            inv = 1.0 / d
            w = S[:, p].copy()
            S -= np.outer(w, w * inv)
            S[:, p] = w * inv
            S[p, :] = w * inv
            S[p, p] = -inv
            ts[p] = 1.0 / ts[p]
            big = max(big, size(S, ts, ts))
        P = -S
        B = A[:, k0:k1].copy()
        B[k0:k1] = 0.0
        C = B @ P
        A -= C @ B.T
        A[:, k0:k1] = C
        A[k0:k1, :] = C.T
        A[k0:k1, k0:k1] = -P
        t[k0:k1] = ts
        big = max(big, size(A, t, t))
    return -A, float(big), bad


def plant_negative_pivot(H, j):
    """H with H[j, j] -= 2^20: the pivots before j stay 1, pivot j is 1 - 2^20 (every later operation stays finite)."""
    Hb = np.array(H, dtype=np.float64)
    Hb[j, j] -= 2.0 ** 20
    return Hb


def first_mismatch(M, ref, blk=128):
    """(count of differing entries, (row block, column block) of the first one in row-major order) or (0, None)."""
    ne = M != ref
    cnt = int(np.count_nonzero(ne))
    if cnt == 0:
        return 0, None
    r, c = np.unravel_index(int(np.argmax(ne)), ne.shape)
    return cnt, (int(r) // blk, int(c) // blk)
