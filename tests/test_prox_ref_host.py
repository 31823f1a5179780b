"""The host model of the prox / dual update (tests/_prox_ref.py) against two independent statements of the same thing: the CPU oracle's
C prox operators, bit for bit, on every input generator the GPU tests use, and the definitions (the exact minimiser in rationals for
L1 / L0, the sorted order for the ball, long double for the group prox).  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import _prox_ref as P

SIZES = (130, 1900, 2112)


def _same(a, b):
    assert not np.isnan(a).any() and not np.isnan(b).any()
    return np.array_equal(a, b)                          # == semantics: -0.0 == 0.0


def _oprox(oracle, kind, param, gl=0):
    return {P.L1: oracle.NormL1, P.L0: oracle.NormL0}[kind](param) if kind in (P.L1, P.L0) else \
        (oracle.IndBallL0(int(param)) if kind == P.BALL else oracle.GroupL2(param, gl))


def _elementwise_inputs(n, rng):
    yield "dyadic", P.dyadic(n, rng)
    yield "l1-cuts", P.cuts(n, rng, 0.25)[0]
    yield "l0-cuts", P.cuts(n, rng, 0.5, shift=3)[0]
    yield "wide", P.wide_values(n, rng)


@pytest.mark.parametrize("n", SIZES)
def test_l1_l0_equal_the_oracle_bit_for_bit(oracle, n):
    rng = np.random.default_rng(n)
    for name, v in _elementwise_inputs(n, rng):
        for c in (P.L1_CUT, P.L0_CUT, dict(kind=P.L1, mu=2.0 ** -3, param=1.0), dict(kind=P.L0, mu=2.0 ** -4, param=4.0)):
            assert _same(P.prox(c["kind"], v, c["param"], c["mu"]), oracle.prox(_oprox(oracle, c["kind"], c["param"]), v, c["mu"])), (name, c)


@pytest.mark.parametrize("gl", [1, 2, 3, 64, 128, 200, 256, 300])
@pytest.mark.parametrize("n", SIZES)
def test_group_equals_the_oracle_bit_for_bit(oracle, n, gl):
    if gl > n:
        gl = n // 2
    rng = np.random.default_rng(n + gl)
    for name, v in (("special", P.group_input(n, gl, rng)[0]), ("no-next", P.group_input(n, gl, rng, with_next=False)[0]),
                    ("wide", P.wide_group(n, gl, rng)), ("dyadic", P.dyadic(n, rng))):
        z = P.prox(P.GROUP, v, P.GROUP_LAM, P.GROUP_MU, gl)
        zo = oracle.prox(oracle.GroupL2(P.GROUP_LAM, gl), v, P.GROUP_MU)
        assert _same(z, zo), (name, n, gl, int((z != zo).sum()))
        # the oracle's wrapper starts from z = 0: the entries beyond the last whole group are what the caller handed in
        zp = rng.standard_normal(n)
        z2 = P.prox(P.GROUP, v, P.GROUP_LAM, P.GROUP_MU, gl, z_prev=zp)
        ng = n // gl
        assert _same(z2[:ng * gl], zo[:ng * gl]) and _same(z2[ng * gl:], zp[ng * gl:])


def test_group_special_groups_do_what_they_are_there_for():
    """norm == lambda mu exactly gives 0; the next s2 above it is that: the next double; a zero group gives 0 without NaN."""
    t = P.GROUP_LAM * P.GROUP_MU
    for gl in (2, 3, 64):
        e = np.zeros(gl); e[0], e[-1] = 3 * t / 5, -4 * t / 5
        assert P.group_s2(e, gl)[0] == t * t and not P.prox(P.GROUP, e, P.GROUP_LAM, P.GROUP_MU, gl).any()
        if gl >= 3:
            e[1] = 2.0 ** -28
            assert P.group_s2(e, gl)[0] == np.nextafter(t * t, 1.0)
    z = P.prox(P.GROUP, np.zeros(8), P.GROUP_LAM, P.GROUP_MU, 4)
    assert not z.any() and not np.isnan(z).any()
    v = P.wide_group(512, 64, np.random.default_rng(0))
    z = P.prox(P.GROUP, v, P.GROUP_LAM, P.GROUP_MU, 64)
    assert np.array_equal(z[64:128], v[64:128]) and not z[-64:].any() and v[-64:].all()      # s2 = inf: scale 1; s2 = 0: scale 0


@pytest.mark.parametrize("n", [1900, 2112, 8320])
def test_ball_equals_the_oracle_and_the_definition(oracle, n):
    rng = np.random.default_rng(n)
    for label, v, rs, _ in P.ball_inputs(n, rng) + P.wide_ball(n, rng):
        order = sorted(range(n), key=lambda i: (-abs(v[i]), i))
        for r in rs:
            keep = P.ball_keep(v, r)
            assert int(keep.sum()) == min(r, n), (label, r)
            assert set(np.flatnonzero(keep)) == set(order[:r]), (label, r)
            if r <= 64 or n <= 2112:                    # (the oracle's selection is O(n r))
                assert _same(P.prox(P.BALL, v, r, 0.05), oracle.prox(oracle.IndBallL0(r), v, 0.05)), (label, r)


def test_ball_inputs_hold_what_their_labels_say():
    rng = np.random.default_rng(1)
    cases = {c[0]: c for c in P.ball_inputs(8320, rng)}
    f32 = lambda v: np.abs(v).astype(np.float32)
    for m in (1023, 1024):
        for name in (f"float-key-{m}", f"float-key-ties-{m}"):
            assert int((f32(cases[name][1]) == np.float32(1.0)).sum()) == m
        v = cases[f"bin11-{m}"][1]
        assert int(((f32(v).view(np.uint32) >> 20) == (np.float32(1.0).view(np.uint32) >> 20)).sum()) == m
        assert np.unique(np.abs(cases[f"float-key-{m}"][1])).size > m                    # distinct doubles
        v, rs = cases[f"float-key-ties-{m}"][1:3]
        a = np.abs(v)
        thr = np.sort(a)[::-1][rs[0] - 1]
        tie = np.flatnonzero(a == thr)
        keep = P.ball_keep(v, rs[0])
        assert tie.size == 4 and 0 < keep[tie].sum() < 4 and tie[1] < 8192 <= tie[-1]      # the cut inside a quadruple, across the passes
        assert keep[tie[tie < 8192]].all() and not keep[tie[-1]]
    v = cases["one-float-key-3"][1]
    i3 = np.flatnonzero(f32(v) == np.float32(2.0))
    assert i3.size == 3 and np.all(np.diff(np.abs(v[i3])) > 0)                           # the larger, the higher its index
    v = cases["sparse"][1]
    assert np.count_nonzero(v) == 40 and (v == 0).sum() >= 1100
    for label, v, rs, cnt in P.wide_ball(1900, rng):
        with np.errstate(over="ignore"):
            k = f32(v)
        assert int(np.isinf(k).sum()) == 6 if label.startswith("above") else int(((k == 0) & (v != 0)).sum()) == 8


def _objective(kind, z, v, lam, mu):
    z, v = Fraction(z), Fraction(v)
    pen = Fraction(lam) * abs(z) if kind == P.L1 else (Fraction(lam) if z != 0 else Fraction(0))
    return pen + (z - v) ** 2 / (2 * Fraction(mu))


@pytest.mark.parametrize("case", [P.L1_CUT, P.L0_CUT], ids=["l1", "l0"])
def test_l1_l0_attain_the_exact_minimum(case):
    """In rationals: z_i minimises lambda |z| + (z - v_i)^2 / (2 mu) (L1), lambda [z != 0] + (z - v_i)^2 / (2 mu) (L0) over the
    candidates {z_i, 0, v_i, v_i +- g, z_i +- 2^-30}.  At the L0 tie |v| == sqrt(2 mu lambda) both 0 and v are minimisers; the model --
    as the reference's strict > -- takes 0."""
    rng = np.random.default_rng(3)
    kind, mu, lam = case["kind"], case["mu"], case["param"]
    g = mu * lam
    c = 0.25 if kind == P.L1 else 0.5
    v = np.concatenate([P.cuts(300, rng, c)[0], P.dyadic(200, rng, bits=40)])
    z = P.prox(kind, v, lam, mu)
    ties = 0
    for vi, zi in zip(v, z):
        best = _objective(kind, zi, vi, lam, mu)
        for cand in (0.0, vi, vi + g, vi - g, zi + 2.0 ** -30, zi - 2.0 ** -30):
            assert best <= _objective(kind, cand, vi, lam, mu), (vi, zi, cand)
        if kind == P.L0 and abs(vi) == c:
            assert zi == 0.0 and _objective(kind, vi, vi, lam, mu) == best
            ties += 1
    assert kind == P.L1 or ties >= 2


@pytest.mark.parametrize("gl", [1, 2, 3, 64, 200])
def test_group_is_within_4_ulp_of_the_definition(gl):
    rng = np.random.default_rng(gl)
    n = 1900
    v = P.group_input(n, gl, rng, with_next=False)[0]
    z = P.prox(P.GROUP, v, P.GROUP_LAM, P.GROUP_MU, gl)
    ng = n // gl
    vl = v[:ng * gl].astype(np.longdouble).reshape(ng, gl)
    nrm = np.sqrt((vl * vl).sum(axis=1))
    with np.errstate(divide="ignore"):
        sc = np.where(nrm > 0, np.maximum(0, 1 - np.longdouble(P.GROUP_LAM * P.GROUP_MU) / np.where(nrm > 0, nrm, 1)), 0)
    ref = (sc[:, None] * vl).reshape(-1)
    err = np.abs(z[:ng * gl].astype(np.longdouble) - ref).astype(np.float64)
    assert np.all(err <= 4 * np.spacing(np.abs(ref.astype(np.float64))))


@pytest.mark.parametrize("kind,param,gl", [(P.L1, 4.0, 0), (P.L0, 1.0, 0), (P.BALL, 32, 0), (P.GROUP, 5.0, 3), (P.GROUP, 5.0, 200)])
def test_iterate_is_the_reference_loop_around_the_oracles_prox(oracle, kind, param, gl):
    """The oracle's ADMM entry points take x0 only (z = u = 0), so the loop of src/lasso.jl:152-164 is restated here around the ORACLE's
    prox with M = mu I: x = z - u, z = prox(x + u), u += x - z, stop when norm(x - z) < tol."""
    rng = np.random.default_rng(int(param) + gl)
    n, mu = 1900, 2.0 ** -4
    z0, u0 = P.dyadic(n, rng), P.dyadic(n, rng)
    tol = 0.0
    for iters in (1, 2, 3):
        m = P.iterate(z0, u0, mu, kind, param, gl, tol=tol, iters=iters)
        z, u = z0.copy(), u0.copy()
        for _ in range(iters):
            x = mu * ((z - u) / mu)
            zo = oracle.prox(_oprox(oracle, kind, param, gl), x + u, mu)
            zo[(n // gl) * gl if gl else n:] = z[(n // gl) * gl if gl else n:]           # (prox! leaves the entries outside every slice)
            z, u = zo, u + (x - zo)
        assert _same(m["x"], x) and _same(m["z"], z) and _same(m["u"], u) and m["iters"] == iters and not m["converged"]
        assert abs(m["nxz"] - float(np.linalg.norm(x - z))) <= P.nxz_bound(n) * m["nxz"]


def test_iterate_stops_with_strict_less_than():
    n, mu = 300, 2.0 ** -4
    z0 = np.zeros(n); z0[1], z0[n - 2] = 3 * 2.0 ** -5, -4 * 2.0 ** -5
    nxz = 5 * 2.0 ** -5
    a = P.iterate(z0, np.zeros(n), mu, P.L1, 4.0, tol=nxz, iters=2)                   # (x2 = -d, z2 = 0: the same norm twice)
    assert a["hist"][0]["nxz_exact"] and [h["nxz"] for h in a["hist"]] == [nxz, nxz] and a["iters"] == 2 and not a["converged"]
    a = P.iterate(z0, np.zeros(n), mu, P.L1, 4.0, tol=nxz, iters=5)                   # (u2 = 0: iteration 3 finds x = z = 0 and stops)
    assert a["iters"] == 3 and a["converged"] and a["nxz"] == 0.0
    b = P.iterate(z0, np.zeros(n), mu, P.L1, 4.0, tol=np.nextafter(nxz, np.inf), iters=3)
    assert b["iters"] == 1 and b["converged"] and _same(b["u"], z0) and not b["z"].any()


def test_sum_is_exact_is_conservative():
    assert P.sum_is_exact(np.array([3.0, -4.0, 0.0]) * 2.0 ** -5)
    assert not P.sum_is_exact(np.array([1.0, 2.0 ** -40]))                              # the square of 1 + 2^-40 does not fit
    assert not P.sum_is_exact(P.dyadic(1000, np.random.default_rng(0)))
    d = P.dyadic(4096, np.random.default_rng(0), bits=9, hi=32.0)
    assert P.sum_is_exact(d) and float(np.sum(d * d)) == float(sum(Fraction(x) ** 2 for x in d))
