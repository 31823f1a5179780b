"""The host models of the packed inverse (tests/_packed_ref.py) and the extended-precision model of a handle's iterates
(oracle lpvo_admm_minv_ld) against the properties DESIGN.md 4.1 states for each storage.  CPU only: the GPU module
tests/test_gpu_packed_inverse.py holds the device to these models entry by entry, so the models themselves are checked here."""
import numpy as np
import pytest

import _packed_ref as R


def _inverse_like(n, seed, offdiag=2.0 ** -12, mu=2.0 ** -4):
    """A symmetric matrix shaped like a diagonally dominant inverse: diagonal near mu, everything else `offdiag` of it and spread
    over many binades (so that fixed-point rows of very different steps occur)."""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n)) * offdiag * mu * np.exp2(-6 * rng.random((n, 1)))
    A = np.tril(A, -1)
    A = A + A.T
    A[np.diag_indices(n)] = mu * (0.5 + 0.5 * rng.random(n))
    return A


def _adversarial_values():
    """Doubles that stress the 6-byte format: every binade edge, mantissas of all ones (the carry runs into the exponent), exact ties
    in both signs, values outside the float range, zeros of both signs, subnormals."""
    v = []
    for e in (-130, -121, -120, -119, -60, -1, 0, 1, 60, 126, 127, 128, 300):
        for mant in (0, 1, (1 << 12) - 1, 1 << 12, (1 << 12) + 1, (1 << 13) - 1, 1 << 13, 3 << 12, (1 << 52) - 1, (1 << 52) - (1 << 12),
                     (1 << 52) - (1 << 12) - 1, 0x5555555555555 & ((1 << 52) - 1)):
            bits = np.uint64(((e + 1023) << 52) | mant)
            x = np.array([bits], dtype=np.uint64).view(np.float64)[0]
            v += [x, -x]
    v += [0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1040]
    return np.array(v)


def test_split_round_error_ties_and_range():
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.standard_normal(1 << 16) * np.exp2(rng.integers(-100, 100, 1 << 16)), _adversarial_values()])
    r = R.split_round(a)
    assert np.array_equal(R.split_round(r), r)                                     # idempotent
    inside = (np.abs(a) >= 2.0 ** -120) & (np.abs(a) < 2.0 ** 127)
    assert inside.sum() > 60000 and (~inside).sum() > 20
    assert np.all(np.abs(r[inside] - a[inside]) <= 2.0 ** -40 * np.abs(a[inside]))
    assert np.all(r[a == 0] == 0)
    # the 48 leading bits: the low 13 of the result are clear, so a float head and a 16-bit tail hold it exactly
    assert np.all((r[inside].view(np.uint64) & np.uint64((1 << 13) - 1)) == 0)
    head = r[inside].view(np.uint64) & ~np.uint64((1 << 29) - 1)
    assert np.array_equal(head.view(np.float64).astype(np.float32).astype(np.float64), head.view(np.float64))
    # ties go up in magnitude, by exactly 2^12 units of the last place of the input's binade
    t = R.split_ties(a) & inside
    assert t.sum() >= 20
    assert np.all(np.abs(r[t]) > np.abs(a[t]))
    assert np.all(r[t].view(np.uint64) - a[t].view(np.uint64) == np.uint64(1 << 12))
    # ... and everything else goes to the nearer neighbour
    low = (a.view(np.uint64) & np.uint64((1 << 13) - 1)).astype(np.int64)
    dn, up = inside & (low < (1 << 12)), inside & (low > (1 << 12))
    assert np.all(np.abs(r[dn]) <= np.abs(a[dn])) and np.all(np.abs(r[up]) > np.abs(a[up]))
    # outside the float range: one rounding to float (overflow to inf, flush of what a float cannot hold)
    with np.errstate(over="ignore"):
        assert np.array_equal(r[~inside], a[~inside].astype(np.float32).astype(np.float64), equal_nan=True)
    # a mantissa of all ones carries into the exponent: the next power of two
    x = np.nextafter(2.0, 0.0)
    assert R.split_round(np.array([x, -x])).tolist() == [2.0, -2.0]


def test_ties_occur_at_the_expected_rate_in_an_inverse():
    """The low 13 bits of an inverse's doubles are uniform: 2048^2 / 8192 = 512 ties expected (binomial, sigma 22.6): counted, and
    every one of them rounded away from zero."""
    rng = np.random.default_rng(2)
    n = 2048
    B = rng.standard_normal((n, 16)) * 0.05
    M = np.linalg.inv(np.diag(np.linspace(1.0, 40.0, n)) + B @ B.T + 16.0 * np.eye(n))
    M = np.tril(M) + np.tril(M, -1).T                      # (LAPACK's two triangles differ in the last bits)
    t = R.split_ties(M)
    cnt = int(t.sum())
    print(f"ties in a 2048^2 inverse: {cnt} (expected 512)")
    assert 512 - 5 * 23 <= cnt <= 512 + 5 * 23, cnt
    r = R.split_round(M)
    assert np.all(np.abs(r[t]) > np.abs(M[t])) and np.all(np.abs(r - M) <= 2.0 ** -40 * np.abs(M))
    m = R.packed_model(M, n, storage="split")
    assert np.array_equal(m["Mt"], r) and m["bytes"] == 6 * 2048 * (2048 + 128) // 2


@pytest.mark.parametrize("n,ns", [(2048, 1), (2096, 1), (2048, 3)])
def test_mixed_model_properties(n, ns):
    A = _inverse_like(n, 3 + n + ns)
    A[5, 700] = A[700, 5] = 0.0                                                     # exact zeros inside fixed-point tiles
    A[1500:1628, 0:128] = 0.0; A[0:128, 1500:1628] = 0.0                            # ... and all-zero rows of a tile
    A[300, :] *= 2.0 ** -4; A[:, 300] *= 2.0 ** -4
    A[300, 301] = A[301, 300] = np.nextafter(2.0 ** -14, 0.0)                       # a row maximum one ulp under its power of two: the clamp
    np_ = R.padded_size(n)
    m = R.packed_model(A, n, ns=ns, storage="mixed")
    types = m["types"]
    tiles = R.tile_list(np_)
    assert m["storage"] == "mixed" and len(types) == len(tiles)
    nd = sum(1 for t, (I, J) in enumerate(tiles) if I == J and types[t] == R.FIXED_DIAG)
    assert np.all(types[[t for t, (I, J) in enumerate(tiles) if I != J]] == R.FIXED)
    assert nd == (0 if ns > 1 else np_ // 128)                                      # ns > 1: diagonal tiles always float-head
    assert m["bytes"] == (len(tiles) - np_ // 128) * 74240 + (np_ // 128) * (98304 if ns > 1 else 75264)
    Mt = m["Mt"]
    off = np.ones((n, n), dtype=bool)                                               # symmetric across tiles; inside a fixed diagonal tile
    for I in range(np_ // 128):                                                     # the two mirror entries carry their own rows' steps
        off[128 * I:128 * (I + 1), 128 * I:128 * (I + 1)] = False
    assert np.array_equal(Mt[off], Mt.T[off]) and np.all(Mt[A == 0] == 0)
    # idempotent: the packed matrix packs to itself, with the same map
    m2 = R.packed_model(Mt, n, ns=ns, storage="mixed")
    assert np.array_equal(m2["Mt"], Mt) and np.array_equal(m2["types"], types)
    # element error: step/2 in fixed-point tiles (a clamped element: one step), 2^-40 relative in float-head tiles, diagonals of fixed tiles exact
    P, Pt = R.pad_device(A, n, np_), R.pad_device(Mt, n, np_)
    clamped = 0
    for t, (I, J) in enumerate(tiles):
        T, Tt = P[I * 128:(I + 1) * 128, J * 128:(J + 1) * 128], Pt[I * 128:(I + 1) * 128, J * 128:(J + 1) * 128]
        if types[t] == R.FLOAT_HEAD:
            assert np.all(np.abs(Tt - T) <= 2.0 ** -40 * np.abs(T))
            continue
        step, e, rmax = R.row_steps(T, I == J)
        assert np.all(step[rmax > 0] <= m["limit"]) and np.all(step[rmax > 0] > 2.0 ** -36 * rmax[rmax > 0])
        err = np.abs(Tt - T)
        if I == J:
            assert np.array_equal(np.diag(Tt), np.diag(T))
            np.fill_diagonal(err, 0.0)
        cl = np.abs(T) > (2.0 ** 35 - 1) * step[:, None]
        if I == J:
            np.fill_diagonal(cl, False)
        clamped += int(cl.sum())
        assert np.all(err[~cl] <= step[:, None].repeat(128, 1)[~cl] / 2) and np.all(err[cl] <= step[:, None].repeat(128, 1)[cl])
    assert clamped >= (1 if ns == 1 else 0)
    # mixed32: the 32 leading bits and the nibble planes together are the 36-bit matrix, nibbles in [0, 15] steps
    m32 = R.packed_model(A, n, ns=ns, storage="mixed32")
    assert np.array_equal(m32["Mt"], Mt) and np.array_equal(m32["M32"] + m32["N"], Mt)
    assert np.all(m32["N"] >= 0) and m32["bytes"] == m["bytes"] - 8192 * int(np.count_nonzero(types))
    assert np.count_nonzero(m32["N"]) > 0.8 * np.count_nonzero(Mt) * (1 - (np_ // 128 if ns > 1 else 0) * 128 * 128 / n ** 2) - n
    P32 = R.pad_device(m32["M32"], n, np_)
    for t, (I, J) in enumerate(tiles):
        if types[t] and I != J:
            step, _, _ = R.row_steps(P[I * 128:(I + 1) * 128, J * 128:(J + 1) * 128], False)
            k = P32[I * 128:(I + 1) * 128, J * 128:(J + 1) * 128] / np.where(step > 0, step, 1.0)[:, None]
            assert np.array_equal(np.mod(k, 16.0), np.zeros_like(k))               # multiples of 16 steps (bias 2^35 is one)
            break


def test_mixed_admission_uses_the_valid_rows_and_falls_back_to_split():
    """max|M| of the admission rule is taken over the n valid rows: the ones on the pad diagonal must not loosen it.  Off-diagonal
    entries at 2^-7 of a diagonal of mu = 2^-10 are too large for fixed point (the rule wants < 2^-8 at np = 2048 ... 2176) but would
    pass against the pad's 1.0; with every off-diagonal tile refused fewer than half are fixed and the whole matrix is `split`."""
    n = 2096
    A = _inverse_like(n, 11, offdiag=2.0 ** -7, mu=2.0 ** -10)
    v = R.packed_model(A, n, storage="mixed", absmax="valid")
    p = R.packed_model(A, n, storage="mixed", absmax="padded")
    assert v["absmax"] <= 2.0 ** -10 and p["absmax"] == 1.0
    assert v["storage"] == "split" and not v["types"].any() and v["bytes"] == 6 * 2176 * (2176 + 128) // 2
    assert p["storage"] == "mixed" and p["types"].all()
    assert R.fixed_tile_steps(A, n, p["types"]).max() > R.admission_limit(v["absmax"], 2176)    # what the padded rule lets through
    assert np.array_equal(v["Mt"], R.split_round(A))
    # an unpadded size: both conventions are the same rule
    A = _inverse_like(2048, 12)
    a, b = R.packed_model(A, 2048, storage="mixed", absmax="valid"), R.packed_model(A, 2048, storage="mixed", absmax="padded")
    assert np.array_equal(a["types"], b["types"]) and np.array_equal(a["Mt"], b["Mt"]) and a["types"].all()


def test_f64_f32_and_small_models():
    A = _inverse_like(2048, 5)
    A[np.triu_indices(2048, 1)] *= 1 + 2.0 ** -50          # an inverse whose two triangles differ in the last bits: tiles below the diagonal serve both
    f = R.packed_model(A, 2048, storage="f64")
    assert np.array_equal(np.tril(f["Mt"]), np.tril(A)) and f["bytes"] == 8 * 2048 * (2048 + 128) // 2
    for I in range(16):                                     # across tiles the lower triangle wins, inside a diagonal tile both stand
        s = slice(128 * I, 128 * (I + 1))
        assert np.array_equal(f["Mt"][s, s], A[s, s])
    assert np.array_equal(f["Mt"][0:128, 128:256], A[128:256, 0:128].T)
    g = R.packed_model(f["Mt"], 2048, storage="f32")
    assert np.array_equal(g["Mt"], f["Mt"].astype(np.float32).astype(np.float64)) and g["bytes"] == 4 * 2048 * (2048 + 128) // 2
    assert np.array_equal(R.packed_model(g["Mt"], 2048, storage="f32")["Mt"], g["Mt"])
    s = R.packed_model(A[:1000, :1000], 1000, storage="mixed")
    assert s["storage"] == "full" and np.array_equal(s["Mt"], A[:1000, :1000]) and s["bytes"] == 8 * 1024 * 1024


def test_one_launch_quantum_rule():
    A = np.array([[0.5, 0.25], [0.25, 0.125]])
    assert R.one_launch_quantum(A, 2, 1.0) == 2.0 ** (0 - 62)       # R V = 0.75 < 2^0
    assert R.one_launch_quantum(A, 2, 2.0) == 2.0 ** (1 - 62)       # 1.5 < 2^1
    assert R.one_launch_quantum(A, 2, 4.0 / 3.0) == 2.0 ** (1 - 62)  # the factor 1.000001 takes 1.0 over the edge


@pytest.mark.parametrize("kind", ["l1", "l0", "ball", "group"])
def test_minv_model_reproduces_the_extended_precision_adjudicator(oracle, kind):
    """lpvo_admm_minv_ld with M = the extended-precision inverse rounded to double once and xb = M b solved in extended precision is
    the same recursion as lpvo_admm_gram_ld up to that one rounding of M: 2^-53 = 1.1e-16 per element, i.e. a relative perturbation
    of that size in every x-update.  The dual variable integrates it over the 150 iterations and the map's slow modes amplify it --
    by no more than cond(G + I/mu) < 1e3 here -- so the floor is 150 x 1.1e-16 x (a factor below 10): the bound is 1e-13 (measured
    <= 3.8e-15).  A dropped xb_lo (2^-53 of xb in every x-update, never averaged out) or products carried in double (n 2^-53 per row)
    sit well above it only after amplification; the fl32 check below shows the test's sensitivity to the matrix itself."""
    rng = np.random.default_rng(7)
    m, n = 900, 192
    A = rng.standard_normal((m, n)) * np.logspace(0, -1.5, n)[None, :]
    xt = np.zeros(n); xt[rng.choice(n, 12, replace=False)] = 3 * rng.standard_normal(12)
    y = A @ xt + 0.05 * rng.standard_normal(m)
    G, b = A.T @ A, A.T @ y
    pg = {"l1": oracle.NormL1(0.3), "l0": oracle.NormL0(0.05), "ball": oracle.IndBallL0(10), "group": oracle.GroupL2(0.4, 16)}[kind]
    snaps = [1, 40, 150]
    M, hi, lo = oracle.inverse_ld(G, 0.05, b)
    assert np.abs(M @ (G + np.eye(n) / 0.05) - np.eye(n)).max() <= 1e-13 and np.abs(lo).max() <= 2.0 ** -52 * np.abs(hi).max()
    ld = oracle.admm_gram_ld(G, b, pg, snaps, mu=0.05)
    mv = oracle.admm_minv_ld(M, hi, pg, snaps, xb_lo=lo, mu=0.05)
    for c in snaps:
        for k, name in enumerate(("x", "z", "u")):
            d = np.linalg.norm(mv[c][k] - ld[c][k]) / max(np.linalg.norm(ld[c][k]), 1e-300)
            print(f"{kind} iteration {c} {name}: minv model vs adjudicator {d:.2e}")
            assert d <= 1e-13, (kind, c, name, d)
        assert np.array_equal(mv[c][1] != 0, ld[c][1] != 0), (kind, c)
    # the matrix matters: a single-precision copy moves the iterates by about 2^-24, far above that floor
    m32 = oracle.admm_minv_ld(M.astype(np.float32).astype(np.float64), hi, pg, [40], xb_lo=lo, mu=0.05)[40]
    d32 = np.linalg.norm(m32[0] - ld[40][0]) / np.linalg.norm(ld[40][0])
    assert 1e-10 < d32 < 1e-5, d32
    # a start vector is honoured as by the adjudicator
    x0 = rng.standard_normal(n)
    a = oracle.admm_minv_ld(M, hi, pg, [5], xb_lo=lo, x0=x0, mu=0.05)[5]
    g = oracle.admm_gram_ld(G, b, pg, [5], x0=x0, mu=0.05)[5]
    assert np.linalg.norm(a[1] - g[1]) <= 1e-13 * max(np.linalg.norm(g[1]), 1.0)
